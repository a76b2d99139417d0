"""Which cache policy an averaging launch takes from the bytes it touches (dpwa_amd/csrc/policy.hpp):
host code with no HIP in it, compiled here with g++ under AddressSanitizer + UndefinedBehaviorSanitizer
together with tests/native/policy_check.cpp, which checks the rule below, on and above the threshold,
the sum over a batch's entries, DPWA_LERP_POLICY and DPWA_CACHE_FIT_BYTES and their parsing, and `0`."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_policy_selection_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "policy_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *SAN,
           os.path.join(ROOT, "tests/native/policy_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    # verify_asan_link_order=0: the environment may preload a library of its own ahead of ASan's
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "policy check ok" in r.stdout
