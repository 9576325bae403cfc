"""numpy restatement of the dynamic zoom (include/rssync_zoom.h, csrc/zoom_math.hpp), built on the stabiliser's
(tests/stabilize_reference.py), and the two cases its tests share.

  bisect      the procedure of the header for one frame and any predicate clear(z)
  fit64       every frame's smallest clear zoom with stabilize_reference's float64 map on the output's border -- map64's
              arithmetic, with the frame's target and row table computed once instead of once per candidate zoom.  Three
              readings of "clear": plain; liberal (border pixels within a tolerance of a frame edge count as inside);
              conservative (they count as outside).  A device whose map is within that tolerance of the float64 one lies
              between the last two.  With the LENS camera a border pixel beyond the zoomed camera's model range has no
              ray and is outside under every reading; with a `margin` (relative, warp_cases.MARGIN) the pixels within it
              of the range count with the near-edge pixels.  The default, 0, leaves the three readings as they were.
  smooth      the envelope

The scene is rectify_reference.scene(): gyro knots 0 .. 2.4 s, the lens at 380 x 676, frames 32 .. 34.  TIMES are the nine
frame times k / 30, k = 31 .. 39 (the scene's three frames are entries 1 .. 3), the delay is synth.D_TRUE, the path's
sigma 0.2 s.
"""
import functools

import numpy as np

import rectify_reference as rr
import stabilize_reference as sr
from rssync_amd import synth

K = tuple(range(31, 40))
TIMES = np.array([k / 30 for k in K])
SCENE = slice(1, 4)             # TIMES[SCENE] are rr.scene()["times"]
SIGMA = 0.2
STEPS = 10
WINDOW = 0.1                    # s: the envelope of the end-to-end test

# name -> keywords of fit64 / fit_zoom beyond the scene's; FITTED: the float64 bisection's zooms (plain, liberal and
# conservative alike), all multiples of (hi - lo) / 2^10
CASES = {
    "A": dict(camera=sr.LENS, out_size=None, lo=1.0, hi=1.5),
    "B": dict(camera=sr.PINHOLE, out_size=(197, 131), lo=0.5, hi=1.5),
}
FITTED = {
    "A": (1.0419921875, 1.0693359375, 1.08203125, 1.0771484375, 1.05517578125, 1.037109375, 1.05810546875, 1.07861328125, 1.09423828125),
    "B": (0.9111328125, 0.9345703125, 0.9423828125, 0.9326171875, 0.912109375, 0.890625, 0.8828125, 0.8955078125, 0.8955078125),
}

PLAIN, LIBERAL, CONSERVATIVE = 0, 1, 2
CLEAR, NOT_CLEAR = 0, 1


@functools.lru_cache(maxsize=None)
def model_max(k):
    """the largest theta (1 + k1 theta^2 + .. + k4 theta^8) on [0, pi / 2]: what |((u - cx) / fx, (v - cy) / fy)| of a pixel
    the lens camera can image stays below (warp_cases.model_max, restated so that this module needs no case list)"""
    th = np.linspace(0.0, np.pi / 2, 200001)
    t2 = th * th
    return float((th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))).max())


def bisect(clear, lo, hi, steps):
    """-> (zoom, status): include/rssync_zoom.h's procedure; 0.5 * (lo + hi) is one addition and one exact halving"""
    if not clear(hi):
        return hi, NOT_CLEAR
    if clear(lo):
        return lo, CLEAR
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if clear(mid):
            hi = mid
        else:
            lo = mid
    return hi, CLEAR


class frame_border:
    """one frame's border map as a function of the zoom: sr.map64(..., px=sr.border(...)) with what does not depend on the
    zoom -- the target and the row table -- kept"""

    def __init__(self, gyro, lens, rows, cols, frame_time, delay, target=None, sigma=0.0, out_size=None, camera=sr.LENS, cam=None,
                 iterations=3, margin=0.0):
        self.lens, self.rows, self.cols, self.camera, self.cam, self.iterations = lens, rows, cols, camera, cam, iterations
        self.margin = margin
        self.out_cols, self.out_rows = (cols, rows) if out_size is None else out_size
        q_t = sr.path64(gyro, np.array([frame_time]), lens[0], delay, sigma)[0] if target is None else sr.unit(target)
        self.table = sr.row_table(gyro, lens, rows, frame_time, delay, q_t)
        self.px = sr.border(self.out_rows, self.out_cols)

    def map(self, zoom):
        cam = sr.out_camera(self.lens, self.rows, self.cols, self.out_rows, self.out_cols, zoom, self.cam)
        r = sr.rays(self.px, cam, self.lens, self.camera, np.float64)
        return sr.iterate(r, self.table, self.lens, self.rows, self.px[..., 1] * (self.rows / self.out_rows), self.iterations, np.float64)

    def range_band(self, zoom):
        """LENS camera -> (beyond, band) of the border pixels: beyond the zoomed camera's model range by more than the
        relative `margin` (no ray: outside under every reading), and within the margin of it on either side (the device's
        ray may or may not exist there: these count with the near-edge pixels).  PINHOLE: every pixel has a ray."""
        if self.camera != sr.LENS:
            return np.zeros(len(self.px), bool), np.zeros(len(self.px), bool)
        fx, fy, cx, cy = sr.out_camera(self.lens, self.rows, self.cols, self.out_rows, self.out_cols, zoom, self.cam)
        rd = np.hypot((self.px[..., 0] - cx) / fx, (self.px[..., 1] - cy) / fy)
        mx = model_max(tuple(self.lens[5:]))
        return rd > mx * (1 + self.margin), (rd >= mx * (1 - self.margin)) & (rd <= mx * (1 + self.margin))

    def clear(self, zoom, mode=PLAIN, tol=0.0):
        m = self.map(zoom)
        outside = ~sr.inside(m, self.rows, self.cols)        # (a pixel without a ray has a NaN position: outside)
        beyond, band = self.range_band(zoom) if self.margin > 0 else (False, False)
        outside = outside | beyond
        if mode != PLAIN:
            near = sr.near_edge(m, self.rows, self.cols, tol) | band
            outside = (outside & ~near) if mode == LIBERAL else (outside | near)
        return not outside.any()


def borders(case=None, times=TIMES, targets=None, **kw):
    """the frame_border of every time of the scene; case: a name of CASES (its lo and hi are not used here)"""
    s = rr.scene()
    if case is not None:
        kw = dict({k: v for k, v in CASES[case].items() if k not in ("lo", "hi")}, **kw)
    kw.setdefault("sigma", SIGMA)
    return [frame_border(s["gyro"], s["lens"], rr.ROWS, rr.COLS, t, synth.D_TRUE, target=None if targets is None else targets[f], **kw)
            for f, t in enumerate(times)]


def fit64(frames, lo, hi, steps=STEPS, mode=PLAIN, tol=0.0):
    """frames: borders(...) -> (zooms (n,) float64, status (n,) uint32)"""
    res = [bisect(lambda z: fb.clear(z, mode, tol), lo, hi, steps) for fb in frames]
    return np.array([r[0] for r in res], np.float64), np.array([r[1] for r in res], np.uint32)


def weight(d, window):
    x = 3.0 * d / window
    return np.exp(-0.5 * (x * x))


def smooth(times, zooms, window):
    """the envelope, one frame at a time, sums in ascending order; the mean clamped to the largest maximum of its window
    (which it exceeds by rounding alone) and to the frame's own zoom"""
    t, z = np.asarray(times, np.float64), np.asarray(zooms, np.float64)
    if window == 0:
        return z.copy()
    W = [np.flatnonzero(np.abs(t - t[f]) <= window) for f in range(len(t))]
    e = np.array([z[w].max() for w in W])
    out = np.empty_like(z)
    for f, w in enumerate(W):
        num = den = 0.0
        for g in w:
            k = weight(t[g] - t[f], window)
            num = num + k * e[g]
            den = den + k
        out[f] = max(min(num / den, e[w].max()), z[f])
    return out
