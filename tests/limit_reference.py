"""numpy restatement of the path limiter (include/rssync_limit.h, csrc/limit_math.hpp), built on the dynamic zoom's
(tests/zoom_reference.py: its scene, its nine frame times, its two cameras and frame_border), and the two cases its tests
share.

  blend       the candidate target at a strength between a frame's own orientation and its goal, in the header's order
  bisect      the procedure of the header for one frame and any predicate clear(a)
  fit64       every frame's largest clear strength with stabilize_reference's float64 map on the output's border: for every
              candidate the blended target, normalised, then zoom_reference.frame_border at the case's zoom.  Three readings
              of "clear" as zoom_reference.fit64 has them: plain; liberal (border pixels within a tolerance of a frame edge
              count as inside); conservative (they count as outside).  A device whose map is within that tolerance of the
              float64 one lies between the last two -- here the conservative reading gives the SMALLER strength.
  smooth      the lower envelope

CASES: the zoom reference's case A (the lens's camera, 380 x 676) at zoom 1.059 and its case B (a pinhole, 197 x 131) at
zoom 0.90, ten steps.  FITTED holds the float64 strengths, plain, liberal and conservative alike: multiples of 2^-10.
Case A was meant for zoom 1.06 (AT_106: its plain and liberal strengths there); at 1.06 the conservative reading of frame 1
is one step lower, 890 / 1024, because a border pixel comes within the map tolerance of a frame edge at 891 / 1024, so the
case's zoom was moved to the nearest thousandth at which the three readings agree in every frame.
"""
import numpy as np

import rectify_reference as rr
import stabilize_reference as sr
import zoom_reference as zr
from rssync_amd import synth

TIMES = zr.TIMES
SIGMA = zr.SIGMA
STEPS = 10
WINDOW = 0.1                    # s: the envelope of the end-to-end test

CASES = {
    "A": dict(camera=sr.LENS, out_size=None, zoom=1.059),
    "B": dict(camera=sr.PINHOLE, out_size=(197, 131), zoom=0.90),
}
# in 1024ths
FITTED = {
    "A": tuple(k / 1024 for k in (1024, 876, 750, 802, 1024, 1024, 1024, 759, 635)),
    "B": tuple(k / 1024 for k in (665, 412, 400, 482, 728, 1024, 1024, 1024, 1024)),
}
AT_106 = tuple(k / 1024 for k in (1024, 891, 762, 814, 1024, 1024, 1024, 773, 646))
NOT_CLEAR_ZOOM = {"A": 1.0, "B": 0.85}        # every frame shows a border even at strength 0

PLAIN, LIBERAL, CONSERVATIVE = zr.PLAIN, zr.LIBERAL, zr.CONSERVATIVE
CLEAR, NOT_CLEAR = 0, 1


def blend(r, g, a):
    """c(a) of include/rssync_limit.h: r and g copied at 0 and 1; else five operations a component, each rounded on its
    own, the dot product summed ((w + x) + y) + z.  Not normalised."""
    r, g = np.asarray(r, np.float64), np.asarray(g, np.float64)
    if a == 0:
        return r.copy()
    if a == 1:
        return g.copy()
    d = ((r[0] * g[0] + r[1] * g[1]) + r[2] * g[2]) + r[3] * g[3]
    s = -1.0 if d < 0 else 1.0
    return (1.0 - a) * r + (s * a) * g


def unit(q):
    """the library's normalisation of a target: n = sqrt(((w w + x x) + y y) + z z), q / n"""
    q = np.asarray(q, np.float64)
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def bisect(clear, steps):
    """-> (strength, status): include/rssync_limit.h's procedure; 0.5 * (lo + hi) is one addition and one exact halving"""
    if clear(1.0):
        return 1.0, CLEAR
    if not clear(0.0):
        return 0.0, NOT_CLEAR
    lo, hi = 0.0, 1.0
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if clear(mid):
            lo = mid
        else:
            hi = mid
    return lo, CLEAR


class limited_frame:
    """one frame's border as a function of the strength at a fixed zoom"""

    def __init__(self, frame_time, zoom, target=None, sigma=SIGMA, gyro=None, lens=None, size=None, delay=None, **kw):
        """gyro, lens, size (rows, cols), delay: None = the scene's; kw: zr.frame_border's"""
        s = rr.scene()
        self.gyro, self.lens = s["gyro"] if gyro is None else gyro, s["lens"] if lens is None else lens
        self.rows, self.cols = (rr.ROWS, rr.COLS) if size is None else size
        self.delay = synth.D_TRUE if delay is None else delay
        self.time, self.zoom, self.kw = frame_time, zoom, kw
        self.own = sr.path64(self.gyro, np.array([frame_time]), self.lens[0], self.delay, 0.0)[0]
        self.goal = sr.path64(self.gyro, np.array([frame_time]), self.lens[0], self.delay, sigma)[0] if target is None \
            else np.asarray(target, np.float64)

    def clear(self, a, mode=PLAIN, tol=0.0):
        fb = zr.frame_border(self.gyro, self.lens, self.rows, self.cols, self.time, self.delay, target=unit(blend(self.own, self.goal, a)),
                             **self.kw)
        return fb.clear(self.zoom, mode, tol)


def frames(case, zoom=None, times=TIMES, targets=None, **kw):
    """the limited_frame of every time; case: a name of CASES; zoom: another than the case's"""
    c = CASES[case]
    kw = dict(dict(camera=c["camera"], out_size=c["out_size"]), **kw)
    return [limited_frame(t, c["zoom"] if zoom is None else zoom, target=None if targets is None else targets[f], **kw)
            for f, t in enumerate(times)]


def fit64(fr, steps=STEPS, mode=PLAIN, tol=0.0):
    """fr: frames(...) -> (strengths (n,) float64, status (n,) uint32)"""
    res = [bisect(lambda a: f.clear(a, mode, tol), steps) for f in fr]
    return np.array([r[0] for r in res], np.float64), np.array([r[1] for r in res], np.uint32)


def smooth(times, strengths, window):
    """the lower envelope, one frame at a time, sums in ascending order; the mean clamped to the smallest minimum of its
    window (which it undercuts by rounding alone) and to the frame's own strength"""
    t, a = np.asarray(times, np.float64), np.asarray(strengths, np.float64)
    if window == 0:
        return a.copy()
    W = [np.flatnonzero(np.abs(t - t[f]) <= window) for f in range(len(t))]
    e = np.array([a[w].min() for w in W])
    out = np.empty_like(a)
    for f, w in enumerate(W):
        num = den = 0.0
        for g in w:
            k = zr.weight(t[g] - t[f], window)
            num = num + k * e[g]
            den = den + k
        out[f] = min(max(num / den, e[w].min()), a[f])
    return out
