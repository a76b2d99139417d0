"""The trimmed consensus without a device: the new C-ABI entries exist with the header's arities, argument
errors are DPWA_ERR_ARG naming the function, and ``trim``'s ValueErrors come before a device is touched."""
import ctypes
import re

import pytest

from dpwa_amd import DpwaConnection, _lib
from dpwa_amd.consensus import effective_trim
from dpwa_amd.group import LocalGroup
from tests.test_distance_host import expect_arg_error, layout, write_cfg


def test_new_symbols_exist_with_the_headers_arities():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(dpwa_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in ("dpwa_consensus_trimmed", "dpwa_consensus_trimmed_mixed", "dpwa_learner_consensus_trimmed"):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == decls[name].count(",") + 1, name
    assert lib.dpwa_abi_version() == 11


def test_bad_arguments_are_reported_without_a_device():
    """Non-NULL pointers here are host addresses no entry may touch: every call must fail first."""
    buf = (ctypes.c_char * (1 << 16))()
    addr = (ctypes.addressof(buf) + 15) & ~15
    out, ws, rec = (ctypes.c_void_p(addr + (5 + k) * 4096) for k in range(3))
    srcs = (ctypes.c_void_p * 5)(*[addr + k * 4096 for k in range(5)])
    ok = [_lib.F32, srcs, 5, 2, 8, out, ws, rec, None, None, None]
    okm = [ctypes.byref(layout((_lib.F16, 0, 4096))), srcs, 5, 2, out, ws, rec, None, None, None]
    # count 2 and 9, trim 0 / negative / 2 * trim = count and beyond, then what dpwa_consensus refuses too
    bad = [(2, 2), (2, 9), (3, 0), (3, -1), (3, 3), (2, 4), (0, 7), (0, _lib.MIXED), (1, None), (4, -1),
           (5, ctypes.c_void_p(addr + 5 * 4096 + 4)), (5, ctypes.c_void_p(addr + 16)), (6, None), (7, None), (9, out)]
    badm = [(0, None), (2, 2), (3, 0), (3, 3), (4, ctypes.c_void_p(addr + 5 * 4096 + 8)), (5, None)]
    for name, base, cases in (("dpwa_consensus_trimmed", ok, bad), ("dpwa_consensus_trimmed_mixed", okm, badm)):
        for i, v in cases:
            expect_arg_error(name, *(base[:i] + [v] + base[i + 1:]))
    ids = (ctypes.c_int32 * 3)(-1, 0, 1)
    expect_arg_error("dpwa_learner_consensus_trimmed", None, ids, 3, 1, 1, out, rec, None)


def test_pythons_trim_errors_are_raised_before_anything_is_launched(tmp_path):
    assert [effective_trim(t, 5) for t in (0, 1, 2, "median")] == [0, 1, 2, 2]
    assert [effective_trim("median", G) for G in range(1, 9)] == [0, 0, 1, 1, 2, 2, 3, 3]
    for t, G, most in ((2, 4, 1), (1, 2, 0), (4, 8, 3)):
        with pytest.raises(ValueError, match=r"G = %d members: the largest trim is %d" % (G, most)):
            effective_trim(t, G)
    cfg = tmp_path / "c.yaml"
    write_cfg(cfg)
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup())
    for wrong in (-1, "mean", 1.0, True, None):           # before the connection's state is looked at
        with pytest.raises(ValueError, match="'median'"):
            conn.consensus(trim=wrong)
    with pytest.raises(RuntimeError, match="update_send"):
        conn.consensus(trim="median")
    conn.close()
