"""Cases of tests/test_warp_cases_cpu.py, tests/test_gpu_warp_lenses.py and tests/measure/gpu_warp_lenses.py: the rectifier
and the stabiliser across lenses, motions, frame sizes and reuses of the ray-map cache.  Helpers only: numpy, the project's
synth and the two restatements (tests/rectify_reference.py, tests/stabilize_reference.py).

  lenses   the seven of pixel_cases.lenses() and pixel_cases.nonmonotonic_lens(), each brought to the test size with
           rr.scaled_lens ('half' is a lens of a 760 x 1352 image: at 95 x 169 its centre lies in the upper left quarter)
  sizes    95 x 169 (1520 // 16 x 2704 // 16: two full 64 x 4 tiles and a part of one across, a part-tile row below) and
           the EDGE_SIZES, with 'synth' and 'aniso'
  motions  gyros with the scene's rate and start (synth.make_gyro(1.0, 1.0 + 12 / FPS, seed=77)):
             x1    the scene's
             x20   its rates times 20, integrated again
             roll  its rates plus ROLL_RATE about the optical axis.  A constant rate alone gives every frame the same map
                   (M_j depends on nothing but the row), and the tests need three frames with three counts of filled
                   pixels, so the scene's own 2 rad/s stay underneath
             rest  identity quaternions
  masks    in_range / out_of_range from the lens alone, `compared` from the float64 map

Every tolerance is rr.device_tolerance's rule per case: four times the largest difference between the float32 and the
float64 restatement over the pixels that case compares; nothing here looks at the device.
"""
import functools

import numpy as np
from scipy.interpolate import CubicSpline

import pixel_cases as pc
import rectify_reference as rr
import stabilize_reference as sr
from rssync_amd import synth

ROWS, COLS = 1520 // 16, 2704 // 16
LENSES = tuple(pc.LENSES) + ("nonmono",)
EDGE_LENSES = ("synth", "aniso")
EDGE_SIZES = ((2, 2), (2, 65), (65, 2), (4, 64), (5, 129), (29, 37), (37, 29))     # rows, cols
MOTIONS = ("x1", "x20", "roll", "rest")
STAB_LENSES = ("synth", "wide", "strong", "negmild")
STAB_SIGMA, STAB_ZOOM = 0.1, 1.1
UNIMAGEABLE = ("negmild", "nonmono")     # lenses that cannot image every pixel of 95 x 169
MARGIN = 1e-3                            # relative band around the model's range that is compared with nothing
ROLL_RATE = 250.0                        # rad/s about the optical axis: +-1.4 rad between the middle and the outer rows
ROLL_BAND = (0.25, 0.5)                  # share of filled pixels of 'synth' under roll at 95 x 169
# measured on the CPU (tests/test_warp_cases_cpu.py asserts them): the share of the in-range pixels whose float64 source
# lies within half an image of the frame, the smallest over lenses and delays
COMPARED_SHARE = {"x1": 1.0, "x20": 1.0, "roll": 1.0, "rest": 1.0}
EXTRA_DELAYS = (0.0, 0.02)
FILL = 77
FULL_ROWS, FULL_COLS = pc.ROWS, pc.COLS
N_POINTS = 512


def base_lens(name):
    return pc.nonmonotonic_lens() if name == "nonmono" else pc.lenses()[name][0]


def lens(name, rows=ROWS, cols=COLS):
    return rr.scaled_lens(rows, cols, base_lens(name))


def _with_rates(g, rates):
    q = synth.integrate_gyro(rates, np.full(len(rates), 1.0 / g.fs))
    return synth.Gyro(fs=g.fs, t0=g.t0, quats=q, times=g.times,
                      spline=CubicSpline(np.arange(len(q), dtype=np.float64), q, axis=0, bc_type="natural"), rates=rates)


@functools.lru_cache(maxsize=None)
def gyro(motion):
    g = rr.scene()["gyro"]
    if motion == "x1":
        return g
    if motion == "x20":
        return _with_rates(g, 20.0 * g.rates)
    if motion == "roll":
        return _with_rates(g, g.rates + np.array([0.0, 0.0, ROLL_RATE]))
    assert motion == "rest"
    q = np.zeros_like(g.quats)
    q[:, 0] = 1.0
    return synth.Gyro(fs=g.fs, t0=g.t0, quats=q, times=g.times,
                      spline=CubicSpline(np.arange(len(q), dtype=np.float64), q, axis=0, bc_type="natural"), rates=0.0 * g.rates)


def frame_time():
    return float(rr.scene()["times"][1])


def frame_times():
    return np.array(rr.scene()["times"], np.float64)


def delays():
    return tuple(synth.D_TRUE + d for d in EXTRA_DELAYS)


def grid(rows, cols):
    ys, xs = np.mgrid[0:rows, 0:cols]
    return np.stack([xs, ys], axis=-1).astype(np.float64)


# ---- masks -------------------------------------------------------------------------------------------------------------
def model_max(L):
    """the largest model(theta) on [0, pi / 2] -- not model(pi / 2): the nonmonotonic model turns over at theta = 1.05"""
    th = np.linspace(0.0, np.pi / 2, 200001)
    return float(pc.model(L, th).max())


def range_masks(L, px):
    """-> (in_range, out_of_range) of positions px (..., 2) for a lens (ro, fx, fy, cx, cy, k1 .. k4); the positions within
    MARGIN of the range on either side are in neither"""
    rd = np.hypot((px[..., 0] - L[3]) / L[1], (px[..., 1] - L[4]) / L[2])
    mx = model_max(L)
    return rd < mx * (1 - MARGIN), rd > mx * (1 + MARGIN)


def near_frame(m64, rows, cols):
    """float64 source positions within half an image of the frame on every side"""
    x, y = m64[..., 0], m64[..., 1]
    return (x >= -cols / 2) & (x <= cols - 1 + cols / 2) & (y >= -rows / 2) & (y <= rows - 1 + rows / 2)


def tolerance(m32, m64, compared):
    """rr.device_tolerance's rule for one case"""
    return 4.0 * float(np.abs(m32.astype(np.float64) - m64)[compared].max())


# ---- rectifier cases ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rect_case(name, motion, extra_delay=0.0, ref_row=None, rows=ROWS, cols=COLS, time_index=1):
    """one map of the rectifier -> dict(lens, gyro, time, delay, m64, in_range, out_of_range, compared, tol); read-only"""
    L, g = lens(name, rows, cols), gyro(motion)
    t, delay = float(rr.scene()["times"][time_index]), synth.D_TRUE + extra_delay
    m64 = rr.map64(g, L, rows, cols, t, delay, ref_row=ref_row)
    m32 = rr.map32(g, L, rows, cols, t, delay, ref_row=ref_row)
    inr, outr = range_masks(L, grid(rows, cols))
    compared = inr & near_frame(m64, rows, cols)
    for a in (m64, inr, outr, compared):
        a.setflags(write=False)
    return dict(lens=L, gyro=g, time=t, delay=delay, ref_row=ref_row, rows=rows, cols=cols, m64=m64, in_range=inr, out_of_range=outr,
                compared=compared, tol=tolerance(m32, m64, compared))


def rect_cases():
    """(lens, motion, extra delay, ref_row) at 95 x 169: every lens x motion at delay D_TRUE and the default ref_row, and
    every lens once more with the other delay and ref_row 0 under x20"""
    out = [(n, m, 0.0, None) for n in LENSES for m in MOTIONS]
    out += [(n, "x20", EXTRA_DELAYS[1], 0) for n in LENSES]
    return out


# ---- stabiliser cases --------------------------------------------------------------------------------------------------
def stab_camera_lens(L, rows, cols, zoom=STAB_ZOOM, out_size=None):
    """the stabiliser's lens camera as a lens tuple: what the range masks of its output pixels are taken from"""
    oc, orows = (cols, rows) if out_size is None else out_size
    return (L[0],) + tuple(sr.out_camera(L, rows, cols, orows, oc, zoom)) + tuple(L[5:])


@functools.lru_cache(maxsize=None)
def stab_case(name, motion, camera=sr.LENS, out_size=None):
    """out_size: (cols, rows) of the output, None = the input's.  A PINHOLE camera gives every pixel a ray: all in range."""
    L, g = lens(name), gyro(motion)
    t, delay = frame_time(), synth.D_TRUE
    kw = dict(sigma=STAB_SIGMA, zoom=STAB_ZOOM, camera=camera, out_size=out_size)
    m64 = sr.map64(g, L, ROWS, COLS, t, delay, **kw)
    m32 = sr.map32(g, L, ROWS, COLS, t, delay, **kw)
    if camera == sr.LENS:
        ocols, orows = (COLS, ROWS) if out_size is None else out_size
        inr, outr = range_masks(stab_camera_lens(L, ROWS, COLS, out_size=out_size), grid(orows, ocols))
    else:
        inr, outr = np.ones(m64.shape[:2], bool), np.zeros(m64.shape[:2], bool)
    compared = inr & near_frame(m64, ROWS, COLS)
    for a in (m64, inr, outr, compared):
        a.setflags(write=False)
    return dict(lens=L, gyro=g, time=t, delay=delay, m64=m64, in_range=inr, out_of_range=outr, compared=compared,
                tol=tolerance(m32, m64, compared))


def stab_cases():
    return [(n, m) for n in STAB_LENSES for m in ("x1", "x20", "roll")]


PINHOLE_LENSES = STAB_LENSES + ("aniso", "half")
PINHOLE_OUT = (131, 73)                  # cols, rows of the other output size: the output camera's cx, cy are scaled


def pinhole_cases():
    """(lens, motion) of the stabiliser's PINHOLE camera, each at the input's size and at PINHOLE_OUT"""
    return [(n, m) for n in PINHOLE_LENSES for m in ("x1", "x20", "roll")]


# ---- points ------------------------------------------------------------------------------------------------------------
def full_size_points(name):
    """-> (lens at 1520 x 2704, points): N_POINTS in-range positions and those of the four corners that are in range"""
    L = lens(name, FULL_ROWS, FULL_COLS)
    rng = np.random.default_rng([pc.SEED, LENSES.index(name)])
    p = rng.uniform((0, 0), (FULL_COLS - 1, FULL_ROWS - 1), size=(64 * N_POINTS, 2))
    p = p[range_masks(L, p)[0]][:N_POINTS]
    assert len(p) == N_POINTS, name
    corners = np.array([[0, 0], [FULL_COLS - 1, 0], [0, FULL_ROWS - 1], [FULL_COLS - 1, FULL_ROWS - 1]], np.float64)
    return L, np.concatenate([p, corners[range_masks(L, corners)[0]]])


def out_of_range_points(name, n=64):
    """positions of a 1520 x 2704 image the lens cannot image"""
    L = lens(name, FULL_ROWS, FULL_COLS)
    rng = np.random.default_rng([pc.SEED, 7])
    p = rng.uniform((0, 0), (FULL_COLS - 1, FULL_ROWS - 1), size=(65536, 2))
    p = p[range_masks(L, p)[1]][:n]
    assert len(p) > 0, name
    return L, p


# ---- sampler cases -----------------------------------------------------------------------------------------------------
def noise(n, rows, cols, seed=11):
    return np.random.default_rng([seed, rows, cols]).integers(0, 256, size=(n, rows, cols), dtype=np.uint8)


def sampler_cases():
    """(lens, motion, rows, cols): the edge sizes under the scene's motion, 95 x 169 under roll"""
    return [(n, "x1", r, c) for n in EDGE_LENSES for r, c in EDGE_SIZES] + [(n, "roll", ROWS, COLS) for n in EDGE_LENSES]


def budget_bytes(rows, cols, frames_per_slot=1.5):
    """the launcher's budget for `frames_per_slot` host frames in each of its two slots (row table, frame in, frame out)"""
    return int(2 * frames_per_slot * ((rows + 1) * 36 + 2 * rows * cols))


def reference_counts(name, motion, rows, cols):
    """the float64 maps' counts of outside pixels of the three frames, and of inside pixels"""
    L, g = lens(name, rows, cols), gyro(motion)
    ok = [rr.inside(rr.map64(g, L, rows, cols, t, synth.D_TRUE)) for t in frame_times()]
    return [int((~o).sum()) for o in ok], [int(o.sum()) for o in ok]


# ---- the cache sequence (section f) ----------------------------------------------------------------------------------------
CACHE_ROWS, CACHE_COLS = 37, 29


def cache_lenses():
    """A = 'aniso' at 37 x 29 (nine distinct fields); B = A with k4 changed by 1e-3; C = A with another readout time"""
    A = lens("aniso", CACHE_ROWS, CACHE_COLS)
    B = tuple(A[:8]) + (A[8] + 1e-3,)
    C = (0.5 * A[0],) + tuple(A[1:])
    return A, B, C
