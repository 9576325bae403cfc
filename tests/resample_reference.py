"""numpy restatement of the bicubic sampler (include/rssync_stabilize.h "Sampling", csrc/resample_math.hpp): float32, one
operation at a time, in the device's order -- so that a device result is its bytes, not its neighbourhood.  The maps, the
scenes and the bilinear samplers are the existing reference modules', imported and not changed.

  weights                 Keys' weights (a = -0.5) of t, four float32 arrays
  sample_bicubic          one plane of uint8 or uint16 through a map -> (image, n_filled), like sr.sample; vmax 255, 1023
                          or 65535
  sample_bicubic_pairs    interleaved pairs (U V) at one position per pair
  sample_bicubic_rgba     four channels at one position
  sample_bicubic16        a 16-bit format's plane of STORED words: unpack (P010: >> 6), sample with the format's vmax, pack
  sample_bicubic_pairs16  ... and its interleaved chroma pairs
"""
import numpy as np

import color16_reference as c16
import rectify_reference as rr
import stabilize_reference as sr

F = np.float32
VMAX = {c16.GRAY16: 65535, c16.P010: 1023, c16.P016: 65535, c16.I010: 1023}

# Mean absolute grey difference to the global-shutter truth (sr.truth(), the figure sr.REFERENCE_ERROR is for the bilinear
# sampler: 0.1789 / 0.1757 / 0.1763) of the scene's three frames sampled with sample_bicubic through sr.reference_maps():
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import resample_reference as q; q.print_figures()"
# The sharper kernel is NOT better on this scene: truth and input are renders of a smooth texture, and it passes on more
# of the input's quantisation.  What it keeps is detail: the standard deviation of the tests' 380 x 676 noise frame
# (default_rng(11), 73.9 grey levels) resampled through reference_maps()[0], inside pixels, bilinear and bicubic.
BICUBIC_ERROR = (0.1957, 0.1927, 0.1942)
NOISE_STD = (50.2, 60.9)


def weights(t):
    """t float32 in [0, 1] -> (w0, w1, w2, w3); exactly (-0, 1, 0, 0) at 0 and (0, 0, 1, 0) at 1"""
    t = np.asarray(t, F)
    w0 = ((F(1) - F(0.5) * t) * t - F(0.5)) * t
    w1 = ((F(1.5) * t - F(2.5)) * t) * t + F(1)
    w2 = ((F(2) - F(1.5) * t) * t + F(0.5)) * t
    w3 = ((F(0.5) * t - F(0.5)) * t) * t
    assert all(w.dtype == F for w in (w0, w1, w2, w3))
    return w0, w1, w2, w3


def taps(map_xy, rows, cols):
    """-> (inside mask, tap columns [4], tap rows [4], wx [4], wy [4]) of a map; positions outside are given (0, 0)"""
    m = map_xy.astype(F)
    ok = sr.inside(m, rows, cols)
    x = np.where(ok, m[..., 0], F(0))
    y = np.where(ok, m[..., 1], F(0))
    ix = np.minimum(np.floor(x).astype(np.int64), cols - 2)
    iy = np.minimum(np.floor(y).astype(np.int64), rows - 2)
    tx = x - ix.astype(F)
    ty = y - iy.astype(F)
    xs = [np.clip(ix + d, 0, cols - 1) for d in (-1, 0, 1, 2)]
    ys = [np.clip(iy + d, 0, rows - 1) for d in (-1, 0, 1, 2)]
    return ok, xs, ys, weights(tx), weights(ty)


def _blend(plane, xs, ys, wx, wy, vmax):
    """the float32 value before rounding, clamped, and the value before the clamp"""
    r = []
    for j in range(4):
        p = [plane[ys[j], xs[d]].astype(F) for d in range(4)]
        r.append((wx[0] * p[0] + wx[1] * p[1]) + (wx[2] * p[2] + wx[3] * p[3]))
    raw = (wy[0] * r[0] + wy[1] * r[1]) + (wy[2] * r[2] + wy[3] * r[3])
    assert raw.dtype == F
    return np.minimum(np.maximum(raw, F(0)), F(vmax)), raw


def sample_bicubic(frame, map_xy, fill=0, vmax=255, clamped=None):
    """-> (output (map rows, map cols) of the frame's dtype, samples filled).  clamped: a dict that receives "low" and
    "high", the inside samples whose value the clamp changed at either end"""
    assert frame.dtype in (np.uint8, np.uint16) and frame.ndim == 2
    rows, cols = frame.shape
    ok, xs, ys, wx, wy = taps(map_xy, rows, cols)
    val, raw = _blend(frame, xs, ys, wx, wy, vmax)
    if clamped is not None:
        clamped["low"] = int(((raw < 0) & ok).sum())
        clamped["high"] = int(((raw > F(vmax)) & ok).sum())
    out = np.rint(val).astype(frame.dtype)
    out[~ok] = fill
    return out, int((~ok).sum())


def sample_bicubic_pairs(uv, map_xy, fill=(128, 128), vmax=255):
    """interleaved pairs (rows, cols, 2) at one position per pair -> (output (map rows, map cols, 2), samples filled)"""
    u, n = sample_bicubic(np.ascontiguousarray(uv[..., 0]), map_xy, fill[0], vmax)
    v, _ = sample_bicubic(np.ascontiguousarray(uv[..., 1]), map_xy, fill[1], vmax)
    return np.stack([u, v], axis=-1), n


def sample_bicubic_rgba(img, map_xy, fill=(0, 0, 0, 255)):
    """(rows, cols, 4) uint8 -> (output (map rows, map cols, 4), pixels filled)"""
    ch = [sample_bicubic(np.ascontiguousarray(img[..., k]), map_xy, fill[k]) for k in range(4)]
    return np.stack([c[0] for c in ch], axis=-1), ch[0][1]


def sample_bicubic16(fmt, words, map_xy, fill=0, clamped=None):
    """one plane of a 16-bit format's stored words -> (stored words, samples filled); fill: a sample value"""
    (vals,) = c16.unpack(fmt, (words,))
    out, n = sample_bicubic(vals, map_xy, fill, VMAX[fmt], clamped)
    return c16.pack(fmt, (out,))[0], n


def sample_bicubic_pairs16(fmt, words, map_xy, fill=(32768, 32768)):
    u, n = sample_bicubic16(fmt, np.ascontiguousarray(words[..., 0]), map_xy, fill[0])
    v, _ = sample_bicubic16(fmt, np.ascontiguousarray(words[..., 1]), map_xy, fill[1])
    return np.stack([u, v], axis=-1), n


def noise_frame():
    """the tests' 380 x 676 noise frame"""
    return np.random.default_rng(11).integers(0, 256, (rr.ROWS, rr.COLS), dtype=np.uint8)


def scene_errors():
    """the scene's three errors against the truth, bicubic through the reference maps"""
    s, maps, tr = rr.scene(), sr.reference_maps(), sr.truth()
    return tuple(rr.grey_error(sample_bicubic(s["frames"][k], maps[k])[0], tr[k], rr.inside(maps[k])) for k in range(rr.N_FRAMES))


def noise_stds():
    """-> (bilinear, bicubic, the frame's own) standard deviation of the noise frame through reference_maps()[0], inside
    pixels, and the number of inside pixels the bicubic clamp changed"""
    noise, m = noise_frame(), sr.reference_maps()[0]
    ok = sr.inside(m, rr.ROWS, rr.COLS)
    cl = {}
    lin = sr.sample(noise, m)[0][ok].astype(np.float64).std()
    cub = sample_bicubic(noise, m, clamped=cl)[0][ok].astype(np.float64).std()
    return float(lin), float(cub), float(noise.astype(np.float64).std()), cl["low"] + cl["high"], int(ok.sum())


def print_figures():
    print("bicubic error against the truth: " + " / ".join("%.4f" % e for e in scene_errors()))
    lin, cub, own, n_clamped, n_inside = noise_stds()
    print("noise: frame %.1f bilinear %.1f bicubic %.1f (+%.0f %%), %d of %d inside pixels clamp" %
          (own, lin, cub, 100 * (cub / lin - 1), n_clamped, n_inside))
    t = np.linspace(0, 1, 100001).astype(F)
    w = weights(t)
    print("weight sum: |(w0 + w1) + (w2 + w3) - 1| <= %.3g" % np.abs(((w[0] + w[1]) + (w[2] + w[3])).astype(np.float64) - 1).max())
