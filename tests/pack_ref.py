"""Host model of packed snapshots (include/dpwa_hip.h "packed snapshots"), the rule restated with numpy
float32 operations only.  Payloads are raw bytes (uint8 arrays) of `dtype` in "f32", "bf16", "f16"."""
import numpy as np

from oracle.lerp import bf16_to_f32, f32_to_bf16

GROUP = 256                    # payload bytes of a group
BLOCK = 4096                   # payload bytes of a block: 16 groups
SIZE = {"f32": 4, "bf16": 2, "f16": 2}
QNAN = np.uint32(0x7FC00000)
TINY = np.float32(2.0 ** -100)
F127 = np.float32(127.0)


def widen(payload, dtype):
    """The payload's elements as fp32, exactly."""
    raw = np.ascontiguousarray(payload, dtype=np.uint8)
    if dtype == "f32":
        return raw.view(np.float32).copy()
    if dtype == "bf16":
        return bf16_to_f32(raw.view(np.uint16))
    return raw.view(np.float16).astype(np.float32)


def narrow(x, dtype):
    """fp32 values as payload bytes: a 16-bit type rounds to nearest even."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        out = x if dtype == "f32" else f32_to_bf16(x) if dtype == "bf16" else x.astype(np.float16)
    return np.ascontiguousarray(out).view(np.uint8).copy()


def blocks(nbytes):
    return max(1, -(-nbytes // BLOCK))


def scale_offset(dtype, nbytes):
    return -(-(blocks(nbytes) * (BLOCK // SIZE[dtype])) // 4096) * 4096


def image_bytes(dtype, nbytes):
    return scale_offset(dtype, nbytes) + -(-(blocks(nbytes) * 64) // 4096) * 4096


def pack(payload, dtype):
    """(q, scale): int8 per element and fp32 per group, both padded to whole blocks."""
    nbytes = len(payload)
    per = GROUP // SIZE[dtype]
    x = np.zeros(blocks(nbytes) * (BLOCK // SIZE[dtype]), dtype=np.float32)   # bytes past the end count as zeros
    x[:nbytes // SIZE[dtype]] = widen(payload, dtype)
    g = x.reshape(-1, per)
    bits = g.view(np.uint32) & np.uint32(0x7FFFFFFF)
    nonfinite = (bits >= np.uint32(0x7F800000)).any(axis=1)
    with np.errstate(all="ignore"):
        amax = np.where(nonfinite, np.float32(1.0), np.abs(g).max(axis=1)).astype(np.float32)
        normal = ~nonfinite & (amax >= TINY)
        den = np.where(normal, amax, np.float32(1.0)).astype(np.float32)
        scale = np.where(normal, den / F127, np.float32(0.0)).astype(np.float32)
        inv = (F127 / den).astype(np.float32)
        q = np.clip(np.rint((g * inv[:, None]).astype(np.float32)), -127, 127)
    q = np.where(normal[:, None], np.nan_to_num(q), 0).astype(np.int8)
    scale = scale.view(np.uint32)
    scale[nonfinite] = QNAN
    return q.reshape(-1), scale.view(np.float32)


def image(payload, dtype):
    """The packed image's bytes: the q plane, zeros to the 4096-byte boundary, the scale plane, zeros."""
    q, scale = pack(payload, dtype)
    out = np.zeros(image_bytes(dtype, len(payload)), dtype=np.uint8)
    out[:q.size] = q.view(np.uint8)
    at = scale_offset(dtype, len(payload))
    out[at:at + 4 * scale.size] = scale.view(np.uint8)
    return out


def unpack(q, scale, dtype, nbytes):
    """The dequantised payload's bytes."""
    per = GROUP // SIZE[dtype]
    with np.errstate(all="ignore"):
        x = (q.reshape(-1, per).astype(np.float32) * scale[:, None]).astype(np.float32).reshape(-1)
    return narrow(x[:nbytes // SIZE[dtype]], dtype)


def roundtrip(payload, dtype):
    """What a peer receives of `payload` through a packed pull."""
    q, scale = pack(payload, dtype)
    return unpack(q, scale, dtype, len(payload))
