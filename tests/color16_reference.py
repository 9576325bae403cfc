"""numpy restatement of the 16-bit colour front (include/rssync_color16.h): the maps are the 8-bit sibling's
(tests/color_reference.py, tests/stabilize_reference.py), so what is restated here is the sample alone.

  sample16         sr.sample on uint16 values: its inside test, taps, weights and three float32 operations, rounded to
                   nearest even into uint16
  sample_pairs16   sample16 per channel of interleaved pairs (cr.sample_pairs)
  unpack / pack    a format's stored words <-> its sample values: P010 keeps them in the ten high bits
"""
import numpy as np

import stabilize_reference as sr

GRAY16, P010, P016, I010 = 16, 17, 18, 19
DEPTH = {GRAY16: 16, P010: 10, P016: 16, I010: 10}
SHIFT = {GRAY16: 0, P010: 6, P016: 0, I010: 0}


def sample16(frame, map_xy, fill=0):
    """-> (output (map rows, map cols) uint16, samples filled): float32, one operation at a time, in the device's order"""
    assert frame.dtype == np.uint16
    rows, cols = frame.shape
    m = map_xy.astype(np.float32)
    ok = sr.inside(m, rows, cols)
    x = np.where(ok, m[..., 0], np.float32(0))
    y = np.where(ok, m[..., 1], np.float32(0))
    x0 = np.minimum(np.floor(x).astype(np.int64), cols - 2)
    y0 = np.minimum(np.floor(y).astype(np.int64), rows - 2)
    fx = x - x0.astype(np.float32)
    fy = y - y0.astype(np.float32)
    p00, p01 = frame[y0, x0].astype(np.float32), frame[y0, x0 + 1].astype(np.float32)
    p10, p11 = frame[y0 + 1, x0].astype(np.float32), frame[y0 + 1, x0 + 1].astype(np.float32)
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    val = top + fy * (bot - top)
    assert val.dtype == np.float32
    r = np.rint(val)
    assert r.min() >= 0 and r.max() <= 65535          # (within the taps' range: no clamp)
    out = r.astype(np.uint16)
    out[~ok] = fill
    return out, int((~ok).sum())


def sample_pairs16(uv, map_xy, fill=(32768, 32768)):
    """interleaved pairs (rows, cols, 2) uint16 at one position per pair -> (output (map rows, map cols, 2), samples filled)"""
    u, n = sample16(np.ascontiguousarray(uv[..., 0]), map_xy, fill[0])
    v, _ = sample16(np.ascontiguousarray(uv[..., 1]), map_xy, fill[1])
    return np.stack([u, v], axis=-1), n


def unpack(fmt, planes):
    """stored words -> sample values, plane by plane (P010: word >> 6, the low six bits ignored)"""
    return tuple(np.asarray(p, np.uint16) >> np.uint16(SHIFT[fmt]) for p in planes)


def pack(fmt, values):
    """sample values -> stored words (P010: value << 6)"""
    out = []
    for v in values:
        v = np.asarray(v)
        assert v.min() >= 0 and v.max() < (1 << DEPTH[fmt])
        out.append((v.astype(np.uint32) << SHIFT[fmt]).astype(np.uint16))
    return tuple(out)
