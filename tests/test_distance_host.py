"""The distance to the peer without a device: the new C-ABI entries exist with the header's arities,
the record is 32 bytes, the workspace is reported and small, bad arguments are DPWA_ERR_ARG naming the
function, the ABI version stays 11, the Python switches refuse ``relay-avg``, and the tolerance of
tests/dist_ref.py is neither vacuous nor too tight for the inputs the GPU tests use."""
import ctypes
import re

import numpy as np
import pytest

from dpwa_amd import DpwaConnection, _lib
from tests import dist_ref as ref

NEW = ["dpwa_distance_workspace", "dpwa_measure_distance", "dpwa_measure_distance_mixed", "dpwa_average_tracked",
       "dpwa_distance_finish", "dpwa_learner_set_distance", "dpwa_learner_distance"]


def workspace_bytes():
    b = ctypes.c_int64()
    _lib.call("dpwa_distance_workspace", ctypes.byref(b))
    return b.value


def test_new_symbols_exist_with_the_headers_arities():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(dpwa_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in decls and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == decls[name].count(",") + 1, name
    assert "dpwa_distance" not in decls          # the struct's name is no function's
    assert lib.dpwa_abi_version() == 11 and _lib.ABI_VERSION == 11


def test_record_is_32_bytes_and_the_workspace_is_small():
    assert ctypes.sizeof(_lib.Distance) == 32
    assert [f[0] for f in _lib.Distance._fields_] == ["dist2", "norm2", "clock", "n"]
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"typedef struct dpwa_distance \{\s*double dist2;\s*double norm2;\s*double clock;\s*int64_t n;\s*\}",
                     text)
    stride = int(re.search(r"#define DPWA_DISTANCE_ACC_STRIDE (\d+)", text).group(1))
    assert stride == _lib.DISTANCE_ACC_STRIDE
    b = workspace_bytes()
    assert 0 < b <= 1 << 20 and b % stride == 0 and b // stride >= 64


def layout(*segs):
    lay = _lib.Layout()
    lay.count = len(segs)
    for i, (dtype, off, length) in enumerate(segs):
        lay.seg[i] = _lib.Segment(dtype, 0, off, length)
    return lay


def expect_arg_error(name, *args):
    lib = _lib.load()
    assert getattr(lib, name)(*args) == _lib.ERR_ARG, name
    assert name.encode() in lib.dpwa_last_error(), (name, lib.dpwa_last_error())


def test_bad_arguments_are_reported_without_a_device():
    """Non-NULL pointers here are host addresses no entry may touch: every call must fail first."""
    buf = (ctypes.c_char * 4096)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = ctypes.c_void_p(addr)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    expect_arg_error("dpwa_distance_workspace", None)
    # dpwa_measure_distance: NULL operands, NULL workspace / record, n < 0, unknown dtype, MIXED, misaligned workspace
    expect_arg_error("dpwa_measure_distance", _lib.F32, None, a, 8, a, a, None)
    expect_arg_error("dpwa_measure_distance", _lib.F32, a, None, 8, a, a, None)
    expect_arg_error("dpwa_measure_distance", _lib.F32, a, a, 8, None, a, None)
    expect_arg_error("dpwa_measure_distance", _lib.F32, a, a, 8, a, None, None)
    expect_arg_error("dpwa_measure_distance", _lib.F32, a, a, -1, a, a, None)
    expect_arg_error("dpwa_measure_distance", 7, a, a, 8, a, a, None)
    expect_arg_error("dpwa_measure_distance", _lib.F64, a, a, 8, a, a, None)
    expect_arg_error("dpwa_measure_distance", _lib.MIXED, a, a, 8, a, a, None)
    expect_arg_error("dpwa_measure_distance", _lib.F32, a, a, 8, ctypes.c_void_p(addr + 8), a, None)
    expect_arg_error("dpwa_measure_distance", _lib.F32, ctypes.c_void_p(addr + 2), a, 8, a, a, None)
    # dpwa_measure_distance_mixed: NULL, malformed layouts, misaligned payload
    good = layout((_lib.F32, 0, 4096), (_lib.F16, 4096, 8192))
    expect_arg_error("dpwa_measure_distance_mixed", None, a, a, a, a, None)
    expect_arg_error("dpwa_measure_distance_mixed", ctypes.byref(good), None, a, a, a, None)
    expect_arg_error("dpwa_measure_distance_mixed", ctypes.byref(good), a, a, None, a, None)
    expect_arg_error("dpwa_measure_distance_mixed", ctypes.byref(good), a, a, a, None, None)
    expect_arg_error("dpwa_measure_distance_mixed", ctypes.byref(good), ctypes.c_void_p(addr + 4), a, a, a, None)
    for bad in (layout(), layout((_lib.F32, 0, 100)), layout((_lib.F32, 4096, 4096)),
                layout((_lib.F32, 0, 4096), (_lib.F32, 4096, 4096)), layout((_lib.F64, 0, 4096)),
                layout((_lib.F32, 0, 4096), (_lib.BF16, 8192, 4096))):
        expect_arg_error("dpwa_measure_distance_mixed", ctypes.byref(bad), a, a, a, a, None)
    # dpwa_average_tracked: dpwa_average's checks, and the two new buffers
    ok = [_lib.F32, a, a, 8, ctypes.byref(cfg), a, 1.0, a, None, a, a, None, None, None]

    def with_(i, v):
        args = list(ok)
        args[i] = v
        return args
    for i, v in ((0, 9), (0, _lib.MIXED), (1, None), (2, None), (3, -1), (4, None), (5, None), (7, None), (9, None),
                 (10, None), (9, ctypes.c_void_p(addr + 4)), (12, a)):
        expect_arg_error("dpwa_average_tracked", *with_(i, v))
    bad_cfg = _lib.Interp(5, 0, 0.5, 0.0)
    expect_arg_error("dpwa_average_tracked", *with_(4, ctypes.byref(bad_cfg)))
    # dpwa_distance_finish
    expect_arg_error("dpwa_distance_finish", None, a, None, 8, None, None, None)
    expect_arg_error("dpwa_distance_finish", a, None, None, 8, None, None, None)
    expect_arg_error("dpwa_distance_finish", a, a, None, -1, None, None, None)
    expect_arg_error("dpwa_distance_finish", a, a, None, 8, None, a, None)
    # the learner entries
    expect_arg_error("dpwa_learner_set_distance", None, 1)
    expect_arg_error("dpwa_learner_distance", None, None)


def write_cfg(path):
    path.write_text("\n".join([
        "- nodes:", "  - {name: w1, host: localhost, port: 48310}", "  - {name: w2, host: localhost, port: 48311}",
        "- fetch_probability: 1.0", "- timeout_ms: 2500", "- interpolation: constant", "- divergence_threshold: 0",
        "- constant: { value: 0.5 }", "- clock: 0", "- loss: 0"]) + "\n")


def test_connection_switches_without_a_device(tmp_path):
    """A connection is made without a device (its learner is bound at the first update_send):
    last_distance is None, and relay-avg with tracking is refused by name, at construction and later."""
    from dpwa_amd.group import LocalGroup
    cfg = tmp_path / "d.yaml"
    write_cfg(cfg)
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), track_distance=True)
    assert conn.last_distance is None
    with pytest.raises(ValueError) as err:
        conn.set_pull("relay-avg")
    assert "relay-avg" in str(err.value) and "track_distance" in str(err.value)
    with pytest.raises(ValueError):
        conn.set_pull("relay-avg:32")
    conn.set_pull("kernel")                     # every other transport stays available
    conn.close()
    with pytest.raises(ValueError) as err:
        DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), pull="relay-avg", track_distance=True)
    assert "relay-avg" in str(err.value) and "track_distance" in str(err.value)
    plain = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup())          # off by default
    assert plain.last_distance is None and plain._track_distance is False
    plain.close()


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_bound_holds_for_a_plain_sum_of_the_same_terms(dtype):
    """For every input set of the GPU tests: numpy's own sum of the reference's terms (pairwise, another
    order than fsum's) stays inside the derived bound of the exactly rounded sum, and a sum carried
    in float32 does not -- so the bound is met by an honest fp64 sum in some other order and is not
    so wide that a narrower accumulation would pass."""
    accs = workspace_bytes() // _lib.DISTANCE_ACC_STRIDE
    narrow_fails = 0
    for n in ref.SIZES[dtype] + [ref.many_spans(dtype, accs)]:
        for name, p, q in ref.cases(dtype, n, accs):
            d, m = ref.terms(dtype, p, q)
            want = ref.reference(dtype, p, q)
            with np.errstate(all="ignore"):
                got = float(np.sum(d)), float(np.sum(m))
                narrow = float(np.sum(d.astype(np.float32), dtype=np.float32))
            for g, w in zip(got, want):
                assert ref.problem(g, w, n) is None, (dtype, n, name, ref.problem(g, w, n))
            if name == "normal" and n >= 100_000 and ref.problem(narrow, want[0], n) is not None:
                narrow_fails += 1
    assert narrow_fails >= 2, "a float32 accumulation passes the bound: it is too wide"
