"""One flat, 256-byte-aligned HBM buffer per learner holding every parameter.

The reference snapshots ``named_parameters()`` tensor by tensor into a dict of bytes and
averages them tensor by tensor (dpwa/adapters/pytorch.py:49-53, 66-68).  Here the
parameters are re-homed once into a single contiguous buffer -- each tensor starting on a
256-byte boundary, in ``named_parameters()`` order, gaps zero-filled -- and every
``param.data`` becomes a view into it, so publishing and averaging are one kernel each
over one buffer.  Gaps average to zero (0*a + 0*b).

A model whose parameters share one dtype gets a buffer of that dtype.  A model that mixes
float32, bfloat16 and float16 parameters (fp32 norms in a bf16 body, say) gets a *segmented*
buffer: one segment per dtype present, in the fixed order float32, bfloat16, float16; inside a
segment the tensors in ``named_parameters()`` order, each 256-byte aligned; every segment starting
on a 4096-byte boundary and zero-filled up to a multiple of 4096 bytes, so that no 16-byte word, no
1-KiB wave span of the averaging kernel and no relay stripe holds two dtypes.  That buffer is one
``torch.uint8`` tensor, every ``param.data`` a typed view into it, and ``layout`` says which bytes
hold which dtype (include/dpwa_hip.h ``dpwa_layout``).
"""
import itertools
import struct

import torch

from . import _lib

ALIGN_BYTES = 256
SEGMENT_BYTES = 4096          # DPWA_LAYOUT_ALIGN
_DATA_PTR = torch.Tensor.data_ptr
# the segments' order, and their codes in a dpwa_layout
SEGMENT_DTYPES = ((torch.float32, _lib.F32), (torch.bfloat16, _lib.BF16), (torch.float16, _lib.F16))


def layout_digest(layout):
    """The 32-bit digest peers compare (dpwa_layout_digest in include/dpwa_hip.h, mirrored here):
    FNV-1a over each segment's little-endian (int32 dtype code, int64 offset, int64 length); a
    result of 0 becomes 1.  `layout`: tuples of (torch dtype, byte offset, byte length)."""
    codes = dict(SEGMENT_DTYPES)
    h = 2166136261
    for dtype, off, length in layout:
        for byte in struct.pack("<iqq", codes[dtype], off, length):
            h = ((h ^ byte) * 16777619) & 0xffffffff
    return h or 1


def c_layout(layout):
    """`layout` as the C ABI's dpwa_layout."""
    codes = dict(SEGMENT_DTYPES)
    out = _lib.Layout()
    out.count = len(layout)
    for i, (dtype, off, length) in enumerate(layout):
        out.seg[i] = _lib.Segment(codes[dtype], 0, off, length)
    return out


def c_param_ranges(ranges):
    """`ranges` -- (name, torch dtype, byte offset, byte length) tuples, ``parameter_ranges()`` -- as the
    C ABI's dpwa_param_range array, sorted by byte offset (a segmented buffer keeps
    ``named_parameters()`` order inside a segment only), and the position of each given range in that
    array."""
    codes = dict(SEGMENT_DTYPES)
    order = sorted(range(len(ranges)), key=lambda i: (ranges[i][2], ranges[i][3], i))
    arr = (_lib.ParamRange * max(1, len(ranges)))()
    where = [0] * len(ranges)
    for k, i in enumerate(order):
        _, dtype, off, length = ranges[i]
        if dtype not in codes:
            raise KeyError("dpwa averages float32, bfloat16 or float16 parameters, got %s" % dtype)
        arr[k] = _lib.ParamRange(int(off), int(length), codes[dtype], 0)
        where[i] = k
    return arr, where


class FlatParameters:
    def __init__(self, named_parameters, device=None):
        """device: where the flat buffer lives (a config's per-node `gpu:` key); parameters on
        another device are moved there (create the optimizer afterwards, as the reference's
        trainer does: examples/pytorch-cifar/main.py:109-116)."""
        params = list(named_parameters)
        if not params:
            raise ValueError("the model has no parameters")
        dtypes = {p.dtype for _, p in params}
        devices = {p.device for _, p in params}
        if len(devices) != 1:
            raise TypeError("all parameters must be on one device, got %s" % sorted(map(str, devices)))
        self.device = devices.pop() if device is None else torch.device(device)
        self.layout = None            # segmented buffers only: ((dtype, byte offset, byte length), ...)
        self.layout_digest = 0
        if len(dtypes) != 1:
            self._init_segmented(params, dtypes)
            return
        self.dtype = dtypes.pop()
        esize = torch.empty((), dtype=self.dtype).element_size()
        align = ALIGN_BYTES // esize
        self.names, self.params, self.offsets = [], [], []
        off = 0
        for name, p in params:
            self.names.append(name)
            self.params.append(p)
            self.offsets.append(off)
            off += (p.numel() + align - 1) // align * align
        self.numel = off
        self.buffer = torch.zeros(self.numel, dtype=self.dtype, device=self.device)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                self.buffer[o:o + p.numel()].copy_(p.data.reshape(-1))
        self._rebind()

    def _init_segmented(self, params, dtypes):
        """Parameters of several dtypes: `buffer` is uint8, `offsets` and `numel` count bytes."""
        known = [d for d, _ in SEGMENT_DTYPES]
        for d in sorted(dtypes, key=str):
            if d not in known:
                # the reference's TYPE_CONVERSION lookup raises KeyError (pytorch.py:11-14, 22)
                raise KeyError("dpwa averages float32, bfloat16 or float16 parameters, got %s" % d)
        self.dtype = torch.uint8
        self.names = [name for name, _ in params]
        self.params = [p for _, p in params]
        self._pdtypes = [p.dtype for p in self.params]
        self._pbytes = [p.numel() * p.element_size() for p in self.params]
        self.offsets = [0] * len(params)
        layout, off = [], 0
        for d in known:
            if d not in dtypes:
                continue
            begin = off
            for i, p in enumerate(self.params):
                if p.dtype == d:
                    self.offsets[i] = off
                    off += (self._pbytes[i] + ALIGN_BYTES - 1) // ALIGN_BYTES * ALIGN_BYTES
            off = max(off, begin + 1)         # a segment of empty tensors still takes a block
            off = (off + SEGMENT_BYTES - 1) // SEGMENT_BYTES * SEGMENT_BYTES
            layout.append((d, begin, off - begin))
        self.layout = tuple(layout)
        self.layout_digest = layout_digest(self.layout)
        self.numel = off
        self.buffer = torch.zeros(self.numel, dtype=torch.uint8, device=self.device)
        with torch.no_grad():
            for i, p in enumerate(self.params):
                self._view(self.buffer, i).reshape(-1).copy_(p.data.reshape(-1))
        self._rebind()

    def _view(self, buffer, i):
        """Parameter i's view into `buffer` (a tensor of this layout)."""
        p, o = self.params[i], self.offsets[i]
        if self.layout is None:
            return buffer[o:o + p.numel()].view(p.shape)
        return buffer[o:o + self._pbytes[i]].view(self._pdtypes[i]).view(p.shape)

    def _rebind(self):
        self._ptrs = []
        for i, p in enumerate(self.params):
            p.data = self._view(self.buffer, i)
            self._ptrs.append(p.data_ptr())

    def rehome(self, buffer):
        """Re-points every parameter into `buffer`, a tensor of this layout that already holds
        the values (a resident learner's slot, which alternates between two: their views are
        built once, so a move costs one ``.data`` assignment per parameter)."""
        if buffer is self.buffer:
            return
        if buffer.numel() != self.numel or buffer.dtype != self.dtype or buffer.device != self.device:
            raise ValueError("rehome: a %s buffer of %d elements on %s is needed" % (self.dtype, self.numel,
                                                                                     self.device))
        cache = self.__dict__.setdefault("_homes", {})
        key = buffer.data_ptr()
        views = cache.get(key)
        if views is None:
            if len(cache) >= 2:
                cache.clear()
            views = cache[key] = [self._view(buffer, i) for i in range(len(self.params))]
        self.buffer = buffer
        for p, v in zip(self.params, views):
            p.data = v
        self._ptrs = [v.data_ptr() for v in views]

    def resync(self):
        """Re-homes parameters whose ``.data`` was replaced since the last call (e.g. a
        user assigned ``param.data = ...``); returns the number re-homed."""
        if list(map(_DATA_PTR, self.params)) == self._ptrs:
            return 0          # the common case: one pointer read per parameter
        moved = 0
        with torch.no_grad():
            for i, p in enumerate(self.params):
                dtype = self.dtype if self.layout is None else self._pdtypes[i]
                if p.data_ptr() != self._ptrs[i] or p.device != self.device or p.dtype != dtype:
                    home = self._view(self.buffer, i)
                    home.reshape(-1).copy_(p.data.reshape(-1))
                    p.data = home
                    self._ptrs[i] = p.data_ptr()
                    moved += 1
        return moved

    def adopt(self, named_parameters):
        """The module holds other ``Parameter`` objects than the ones this buffer was built from
        (``load_state_dict(..., assign=True)``, ``module.weight = nn.Parameter(...)``): takes the
        module's objects in their place -- their values copied into the buffer, their ``.data`` a view
        of it -- when the names, shapes and dtypes are unchanged, and returns how many were taken.
        The objects left behind get storage of their own, so whoever still holds one (an optimizer
        created before) no longer writes the buffer through it.  Raises ValueError naming the first
        parameter that does not fit."""
        new = list(named_parameters)
        names = [name for name, _ in new]
        if names != self.names:
            odd = next(a or b for a, b in itertools.zip_longest(names, self.names) if a != b)
            raise ValueError("the module's parameters are no longer the ones the flat buffer was built from "
                             "(at %r): a model whose structure changed needs a new adapter" % odd)
        for i, (name, p) in enumerate(new):
            dtype = self.dtype if self.layout is None else self._pdtypes[i]
            if p is not self.params[i] and (p.shape != self.params[i].shape or p.dtype != dtype):
                raise ValueError("parameter %r was replaced by one of shape %s and dtype %s (the flat buffer holds "
                                 "%s, %s): a model whose structure changed needs a new adapter"
                                 % (name, tuple(p.shape), p.dtype, tuple(self.params[i].shape), dtype))
        taken = 0
        with torch.no_grad():
            for i, (_, p) in enumerate(new):
                old = self.params[i]
                if p is old:
                    continue
                if old.data_ptr() == self._ptrs[i]:
                    old.data = old.data.clone()
                self.params[i] = p
                home = self._view(self.buffer, i)
                home.reshape(-1).copy_(p.data.reshape(-1))
                p.data = home
                self._ptrs[i] = p.data_ptr()
                taken += 1
        return taken

    def parameter_ranges(self):
        """``[(name, torch dtype, byte offset, byte length)]`` in ``named_parameters()`` order: where
        each parameter's elements lie in the buffer, for single-dtype and segmented buffers alike
        (what ``track_distance="per_parameter"`` measures over; ``c_param_ranges`` makes the C ABI's
        dpwa_param_range list of it)."""
        if self.layout is not None:
            return [(name, d, o, b) for name, d, o, b in zip(self.names, self._pdtypes, self.offsets, self._pbytes)]
        esize = self.buffer.element_size()
        return [(name, self.dtype, o * esize, p.numel() * esize)
                for name, p, o in zip(self.names, self.params, self.offsets)]

    def view(self, name):
        return self._view(self.buffer, self.names.index(name))
