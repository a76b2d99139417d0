"""The per-parameter distance without a device: ``FlatParameters.parameter_ranges()``, every rule of
dpwa_param_range through the C entry, the sizes entry, the Python switches, and tests/pdist_ref.py
itself -- its tolerance is neither vacuous nor too tight, and every wrong kernel it models is told
from the right one by an input the GPU tests run."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, _lib
from dpwa_amd.flat import FlatParameters, c_param_ranges
from tests import dist_ref
from tests import pdist_ref as ref

NEW = ["dpwa_param_ranges_check", "dpwa_param_distance_sizes", "dpwa_param_distance_table",
       "dpwa_measure_param_distance", "dpwa_param_distance_finish", "dpwa_learner_set_param_distance",
       "dpwa_learner_param_distance", "dpwa_learner_param_distance_rounds"]
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MAX_ROWS = 1024   # what the sizes entry reports (checked below)


def model_of(sizes_by_dtype):
    """An nn.Module whose parameters have these sizes, the dtypes interleaved as given."""
    net = torch.nn.Module()
    for i, (dtype, n) in enumerate(sizes_by_dtype):
        net.register_parameter("p%d" % i, torch.nn.Parameter(torch.randn(n).to(TORCH[dtype])))
    return net


def c_ranges(ranges):
    arr = (_lib.ParamRange * max(1, len(ranges)))()
    for i, (off, length, dtype) in enumerate(ranges):
        arr[i] = _lib.ParamRange(off, length, dtype, 0)
    return arr


def check(ranges, dtype, n, layout=None):
    lib = _lib.load()
    rc = lib.dpwa_param_ranges_check(c_ranges(ranges), len(ranges), dtype, n,
                                     ctypes.byref(layout) if layout is not None else None)
    return rc, lib.dpwa_last_error().decode()


def test_new_symbols_exist_with_the_headers_arities():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(dpwa_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in decls and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == decls[name].count(",") + 1, name
    assert lib.dpwa_abi_version() == 11 and _lib.ABI_VERSION == 11
    assert ctypes.sizeof(_lib.ParamRange) == 24 and ctypes.sizeof(_lib.ParamSizes) == 32
    assert re.search(r"typedef struct dpwa_param_range \{\s*int64_t byte_offset;\s*int64_t byte_length;\s*"
                     r"int32_t dtype;\s*int32_t reserved;\s*\}", open(_lib.HEADER_PATH).read())


def test_parameter_ranges_single_dtype():
    for dtype, sizes in (("f32", ref.A_SIZES), ("bf16", ref.A16_SIZES), ("f16", ref.A16_SIZES)):
        net = model_of([(dtype, n) for n in sizes])
        fp = FlatParameters(net.named_parameters())
        got = fp.parameter_ranges()
        assert [r[0] for r in got] == [name for name, _ in net.named_parameters()]
        lay = ref.single("x", dtype, sizes)
        assert [(r[2], r[3]) for r in got] == [(t[2], t[3]) for t in lay.tensors]
        assert all(r[1] == TORCH[dtype] for r in got)
        esize = fp.buffer.element_size()
        assert lay.total_bytes == fp.numel * esize
        for name, _, off, length in got:
            v = fp.view(name)
            assert off == v.storage_offset() * esize and length == v.numel() * esize   # (an empty view has no data_ptr)
            assert off % 256 == 0


def test_parameter_ranges_mixed():
    order = [("bf16", 129), ("f32", 1), ("f16", 1), ("bf16", 512), ("f32", 65)]   # interleaved, as a model's are
    net = model_of(order)
    fp = FlatParameters(net.named_parameters())
    got = fp.parameter_ranges()
    assert [r[0] for r in got] == [name for name, _ in net.named_parameters()]
    for (name, dtype, off, length), (d, n) in zip(got, order):
        v = fp.view(name)
        assert dtype == TORCH[d] and length == n * v.element_size()
        assert off == v.storage_offset() * v.element_size() and off % 256 == 0
    # sorted by offset they are tests/pdist_ref.py's layout M, which the GPU tests run
    lay = ref.layout_m()
    assert sorted((r[2], r[3]) for r in got) == [(t[2], t[3]) for t in lay.tensors]
    assert lay.total_bytes == fp.numel
    assert [(dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[d], o, b) for d, o, b in lay.segments] \
        == list(fp.layout)
    arr, where = c_param_ranges(got)
    assert [arr[k].byte_offset for k in range(len(got))] == sorted(r[2] for r in got)
    assert [arr[where[i]].byte_offset for i in range(len(got))] == [r[2] for r in got]
    lay_c = _lib.Layout()
    lay_c.count = len(fp.layout)
    for i, (d, o, b) in enumerate(lay.segments):
        lay_c.seg[i] = _lib.Segment(dist_ref.CODE[d], 0, o, b)
    assert _lib.load().dpwa_param_ranges_check(arr, len(got), _lib.MIXED, fp.numel, ctypes.byref(lay_c)) == _lib.OK


def test_every_rule_of_a_range_is_checked_without_a_device():
    F32, BF16 = _lib.F32, _lib.BF16
    assert check([(0, 4, F32), (256, 252, F32), (512, 0, F32), (512, 8, F32)], F32, 130)[0] == _lib.OK
    assert check([], F32, 0)[0] == _lib.OK
    bad = [
        ([(0, 8, F32), (0, 8, F32)], F32, 100, "ascending"),                 # overlapping
        ([(256, 8, F32), (0, 8, F32)], F32, 100, "ascending"),               # descending
        ([(0, 260, F32), (256, 8, F32)], F32, 100, "ascending"),             # the first runs into the second
        ([(128, 8, F32)], F32, 100, "multiple of 256"),
        ([(-256, 8, F32)], F32, 100, "multiple of 256"),
        ([(0, 6, F32)], F32, 100, "element size"),
        ([(0, 3, BF16)], BF16, 100, "element size"),
        ([(0, -4, F32)], F32, 100, "element size"),
        ([(0, 8, 2)], F32, 100, "dtype"),                                    # DPWA_F64
        ([(0, 8, _lib.MIXED)], F32, 100, "dtype"),
        ([(0, 8, BF16)], F32, 100, "payload of dtype"),                      # not the payload's
        ([(256, 148, F32)], F32, 100, "outside the payload"),                # ends at byte 404 of 400
        ([(0, 8, F32)], 9, 100, "dtype"),
        ([(0, 8, F32)], F32, -1, "n < 0"),
        ([(0, 8, F32)], _lib.MIXED, 8192, "layout"),                         # MIXED without its layout
    ]
    for ranges, dtype, n, word in bad:
        rc, msg = check(ranges, dtype, n)
        assert rc == _lib.ERR_ARG and "dpwa_param_ranges_check" in msg and word in msg, (ranges, msg)
    arr = c_ranges([(0, 8, F32)])
    arr[0].reserved = 1
    lib = _lib.load()
    assert lib.dpwa_param_ranges_check(arr, 1, F32, 100, None) == _lib.ERR_ARG and b"reserved" in lib.dpwa_last_error()
    assert lib.dpwa_param_ranges_check(None, 1, F32, 100, None) == _lib.ERR_ARG
    # a DPWA_MIXED payload: wholly inside the segment of its dtype
    lay = _lib.Layout()
    lay.count = 2
    lay.seg[0] = _lib.Segment(F32, 0, 0, 4096)
    lay.seg[1] = _lib.Segment(BF16, 0, 4096, 4096)
    assert check([(0, 8, F32), (3840, 256, F32), (4096, 2, BF16), (8192 - 256, 256, BF16)], _lib.MIXED, 8192, lay)[0] == _lib.OK
    for ranges in ([(0, 8, BF16)], [(4096, 8, F32)], [(3840, 260, F32)], [(8192, 2, BF16)], [(7936, 258, BF16)]):
        rc, msg = check(ranges, _lib.MIXED, 8192, lay)
        assert rc == _lib.ERR_ARG and "inside the segment" in msg, (ranges, msg)
    lay.seg[1] = _lib.Segment(BF16, 0, 4000, 4096)   # an invalid layout
    assert check([(0, 8, F32)], _lib.MIXED, 8192, lay)[0] == _lib.ERR_ARG


def sizes_of(lay):
    z = _lib.ParamSizes()
    arr = c_ranges([(off, length, dist_ref.CODE[d]) for _, d, off, length in lay.tensors])
    _lib.call("dpwa_param_distance_sizes", arr, len(lay.tensors), ctypes.byref(z))
    return z


def test_the_sizes_entry():
    for lay in ref.small_layouts() + [ref.layout_b(MAX_ROWS)]:
        z = sizes_of(lay)
        assert z.max_rows == MAX_ROWS
        table, total = ref.rows_of(lay, z.max_rows)
        assert z.table_bytes == 32 * len(lay.tensors)
        assert z.workspace_bytes == _lib.DISTANCE_ACC_STRIDE * total
        assert z.record_bytes == 16 + 16 * len(lay.tensors)
    # layout A: 1 + 1 + 1 + 2 (a span boundary inside it) + 0 (empty) + 2 + 2 rows
    assert [r for _, r in ref.rows_of(ref.layout_a(), MAX_ROWS)[0]] == [1, 1, 1, 2, 0, 2, 2]
    assert ref.rows_of(ref.layout_b(MAX_ROWS), MAX_ROWS)[0] == [(0, MAX_ROWS), (MAX_ROWS, 1)]
    lib = _lib.load()
    z = _lib.ParamSizes()
    assert lib.dpwa_param_distance_sizes(c_ranges([(128, 8, 0)]), 1, ctypes.byref(z)) == _lib.ERR_ARG
    assert b"dpwa_param_distance_sizes" in lib.dpwa_last_error()
    assert lib.dpwa_param_distance_sizes(c_ranges([(0, 8, 0)]), 1, None) == _lib.ERR_ARG
    # the stateless launches check their arguments before they touch a device
    assert lib.dpwa_param_distance_table(c_ranges([(0, 8, 0)]), 1, None) == _lib.ERR_ARG
    assert lib.dpwa_measure_param_distance(None, 1, None, None, 16, None, None, None, None, None) == _lib.ERR_ARG
    assert b"dpwa_measure_param_distance" in lib.dpwa_last_error()
    assert lib.dpwa_param_distance_finish(None, 1, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.dpwa_learner_set_param_distance(None, None, 0, 1) == _lib.ERR_ARG
    assert lib.dpwa_learner_param_distance(None, None, None) == _lib.ERR_ARG
    assert lib.dpwa_learner_param_distance_rounds(None, None, None) == _lib.ERR_ARG


def test_the_python_switches(tmp_path):
    cfg = tmp_path / "c.yaml"
    cfg.write_text("- nodes:\n  - {name: w1, host: localhost, port: 45000}\n  - {name: w2, host: localhost, port: 45001}\n"
                   "- fetch_probability: 1\n- timeout_ms: 2500\n- interpolation: constant\n"
                   "- divergence_threshold: 0\n- constant: { value: 0.5 }\n- clock: 0\n- loss: 0\n")
    ranges = [("w", torch.float32, 0, 16)]
    with pytest.raises(ValueError, match="parameter_ranges"):
        DpwaConnection("w1", str(cfg), track_distance="per_parameter")
    with pytest.raises(ValueError, match="per_parameter"):
        DpwaConnection("w1", str(cfg), track_distance="per-tensor")
    with pytest.raises(ValueError, match="distance_every"):
        DpwaConnection("w1", str(cfg), track_distance="per_parameter", parameter_ranges=ranges, distance_every=0)
    with pytest.raises(ValueError, match="relay-avg"):
        DpwaConnection("w1", str(cfg), track_distance="per_parameter", parameter_ranges=ranges, pull="relay-avg")
    conn = DpwaConnection("w1", str(cfg), track_distance="per_parameter", parameter_ranges=ranges, distance_every=3)
    with pytest.raises(ValueError, match="relay-avg"):
        conn.set_pull("relay-avg")
    assert conn.last_distance is None
    conn.close()
    for off in (True, False):       # the two old values keep their meaning
        conn = DpwaConnection("w1", str(cfg), track_distance=off)
        assert conn._track_distance is off and not conn._per_parameter
        conn.close()


# ---------------------------------------------------------------- the reference and its tolerance
def gpu_input_sets(lay):
    """The (name, param bytes, peer bytes, gap fill) the GPU tests run on a small layout."""
    out = []
    for case in ref.CASE_NAMES:
        p, q = ref.inputs(lay, case)
        out.append((case, p, q))
    live = [t for t in range(len(lay.tensors)) if lay.elements(t)]
    for t in live:
        for case, base in (("last-element", "equal"), ("one-nan", "normal"), ("one-inf", "normal")):
            p, q = ref.inputs(lay, case, victim=t, base=base)
            out.append(("%s in tensor %d" % (case, t), p, q))
    p, q = ref.inputs(lay, "normal", fill=0xff)
    out.append(("nan-gaps", p, q))
    return out


def test_pairwise_float64_meets_the_bound_and_float32_does_not():
    for lay in ref.small_layouts():
        failed32 = 0
        for name, p, q in gpu_input_sets(lay):
            want = ref.reference(lay, p, q)
            got, _ = ref.model(lay, p, q, MAX_ROWS)
            assert not ref.problems(lay, got, want), (lay.name, name)
            got32 = []
            for t, (_, dtype, _, _) in enumerate(lay.tensors):
                d, n = dist_ref.terms(dtype, ref.tensor_bits(lay, t, p), ref.tensor_bits(lay, t, q))
                with np.errstate(all="ignore"):
                    got32.append((float(np.cumsum(d.astype(np.float32))[-1]) if len(d) else 0.0,
                                  float(np.cumsum(n.astype(np.float32))[-1]) if len(n) else 0.0))
            failed32 += bool(ref.problems(lay, got32, want))
        assert failed32 > 0, lay.name         # the bound is not vacuous


def test_empty_tensors_and_gaps():
    lay = ref.layout_a()
    p, q = ref.inputs(lay, "normal", fill=0xff)
    want = ref.reference(lay, p, q)
    assert want[4] == (0.0, 0.0)                                   # the empty tensor
    assert all(math.isfinite(d) and math.isfinite(n) for d, n in want)   # NaN gaps show in no tensor
    assert ref.gap_mask(lay).sum() == lay.total_bytes - 4 * sum(ref.A_SIZES)
    whole = dist_ref.terms("f32", p.view(np.uint32), q.view(np.uint32))[0]
    assert np.isnan(whole).any()                                   # while the whole-model sums would be NaN


def test_every_mutant_is_told_from_the_model_by_an_input_the_gpu_tests_run():
    lays = ref.small_layouts() + [ref.layout_b(MAX_ROWS)]
    found = {m: [] for m in ref.MUTANTS}
    for lay in lays:
        sets = gpu_input_sets(lay) if lay.name != "B" else [("normal",) + ref.inputs(lay, "normal"),
                                                            ("last-element",) + ref.inputs(lay, "last-element")]
        for name, p, q in sets:
            want = ref.reference(lay, p, q)
            for m in ref.MUTANTS:
                if m == "rows-not-zeroed":          # the second call of two on one workspace
                    _, rows = ref.model(lay, p, q, MAX_ROWS, mutant=m)
                    got, _ = ref.model(lay, q, p, MAX_ROWS, mutant=m, rows=rows)
                    bad = ref.problems(lay, got, ref.reference(lay, q, p))
                else:
                    got, rows = ref.model(lay, p, q, MAX_ROWS, mutant=m)
                    bad = ref.problems(lay, got, want)
                    assert not rows.any()
                if bad:
                    found[m].append((lay.name, name))
    for m in ref.MUTANTS:
        assert found[m], "no GPU input tells mutant %r from the right kernel" % m
    assert any(lay == "B" for lay, _ in found["payload-span-row"])
    assert any(name == "nan-gaps" for _, name in found["gap-counted"])
