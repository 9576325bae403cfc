"""Cases of tests/test_render_cases_cpu.py and tests/test_gpu_render_lenses.py: every renderer built on the stabiliser -- the
colour front, the 16-bit formats, the bicubic sampler, the per-frame zoom, the fits and the infill -- across the lenses and
motions of tests/warp_cases.py.  Helpers only: numpy, warp_cases and the restatements; nothing here looks at the device.

  size     94 x 170 luma, 47 x 85 chroma: the chroma plane is one full 64 x 4 tile and a part of one across with a
           part-tile row below, the luma plane two tiles and a part across; OUT is the other (even) output size
  lenses   LENSES from wc.lens(name, 94, 170); 'half' has its principal point at (42.5, 23.5), in the upper left quarter
  motions  x1, x20, roll (wc.gyro), three frames at wc.frame_times(), delay synth.D_TRUE, path sigma wc.STAB_SIGMA
  planes   plane_case: the float64 and float32 restatement maps of plane 0 (sr.map64) or plane 1 (cr.chroma_map64), the range
           masks of the plane's own output camera, `compared` and the tolerance by wc.tolerance's rule
  fits     FIT_CASES / STRENGTH_CASES: zoom and strength fits whose three float64 readings agree in every frame
  infill   INFILL_CASES and the composition of a frame from per-candidate maps (compose_plane)
  checks   check_map, padded and u32, which tests/test_gpu_yuv_lenses.py shares with tests/test_gpu_render_lenses.py
  formats  the colour front's formats with their noise planes, fills and numpy samplers (color_frames, color_fills,
           color_sample_plane, color_plane_fill), which tests/test_gpu_infill_lenses.py shares with it
"""
import functools

import numpy as np

import color16_reference as c16
import color_reference as cr
import infill_reference as ir
import limit_reference as lr
import resample_reference as q
import stabilize_reference as sr
import warp_cases as wc
import zoom_reference as zr
from rssync_amd import synth

ROWS, COLS = 94, 170
C_ROWS, C_COLS = ROWS // 2, COLS // 2
OUT = (62, 110)                          # rows, cols of the other output size: 31 x 55 chroma samples
LENSES = ("aniso", "half", "strong", "negmild", "nonmono", "synth")
MAP_LENSES = ("aniso", "half", "strong", "negmild")
MOTIONS = ("x1", "x20", "roll")
SITES = (cr.CENTER, cr.LEFT)
CAMERAS = (sr.LENS, sr.PINHOLE)
SIGMA, ZOOM = wc.STAB_SIGMA, wc.STAB_ZOOM
N_FRAMES = 3

# measured with the float64 restatement (tests/test_render_cases_cpu.py asserts them): output samples of the LENS camera
# beyond the model's range (by more than wc.MARGIN), (luma, chroma with LEFT siting)
UNIMAGEABLE = {
    1.0: {"half": (7306, 1816), "negmild": (31, 9), "nonmono": (11629, 2897), "aniso": (0, 0), "strong": (0, 0)},
    1.1: {"half": (6174, 1534), "negmild": (0, 0), "nonmono": (10693, 2669), "aniso": (0, 0), "strong": (0, 0)},
}
# samples whose float64 source is not inside the frame at zoom 1.1, per frame: (lens, motion, camera, plane, site) -> counts
OUTSIDE = {
    ("aniso", "x20", sr.LENS, 0, cr.CENTER): (7485, 8193, 7803),
    ("aniso", "x20", sr.LENS, 1, cr.LEFT): (1889, 2067, 1972),
    ("aniso", "roll", sr.LENS, 0, cr.CENTER): (2204, 2199, 2200),
    ("aniso", "roll", sr.PINHOLE, 0, cr.CENTER): (470, 457, 455),
    ("negmild", "roll", sr.LENS, 0, cr.CENTER): (4808, 4805, 4804),
}

# section c: (lens, motion, zoom, camera)
BODY_CASES = (("half", "x1", 1.0, sr.LENS), ("aniso", "x20", 1.1, sr.PINHOLE), ("synth", "roll", 1.1, sr.LENS), ("negmild", "roll", 1.1, sr.LENS))
# Under roll three frames should give three counts of filled luma pixels (a kernel that read frame 0's table for every frame
# would give one).  The centred 'synth' lens does not at 94 x 170: the float64 map has the same 4805 pixels outside in every
# frame, so 'negmild' under roll (4808, 4805, 4804) stands beside it and carries that assertion.
ROLL_COUNTS_DIFFER = (("negmild", "roll"),)
# section d: (lens, motion, the equal zoom); the different zooms are PERCAM_ZOOMS
PERCAM_CASES = (("half", "x1", 1.0), ("nonmono", "x1", 1.0), ("aniso", "x20", 1.1), ("strong", "roll", 1.1))
PERCAM_ZOOMS = (1.0, 1.1, 1.3)
# section f: (lens, motion); radius 1, LENS camera, zoom 1.1
INFILL_CASES = (("aniso", "roll"), ("negmild", "x20"))
INFILL_RADIUS = 1


def lens(name):
    return wc.lens(name, ROWS, COLS)


def out_shape(out_size):
    """out_size (cols, rows) or None -> (rows, cols)"""
    return (ROWS, COLS) if out_size is None else (out_size[1], out_size[0])


def out_sizes():
    """the `out_size` arguments of the map tests: the input's size and OUT"""
    return (None, (OUT[1], OUT[0]))


def plane_camera_lens(L, plane, site, zoom, out_size):
    """the output camera of a plane as a lens tuple (what the range masks of its samples are taken from): plane 0
    wc.stab_camera_lens, plane 1 cr.chroma_camera with the lens's k1 .. k4"""
    orows, ocols = out_shape(out_size)
    if plane == 0:
        return wc.stab_camera_lens(L, ROWS, COLS, zoom, out_size)
    return (L[0],) + tuple(cr.chroma_camera(L, ROWS, COLS, orows, ocols, site, zoom)) + tuple(L[5:])


def plane_maps(fn_luma, fn_chroma, g, L, t, plane, site, zoom, camera, out_size):
    kw = dict(sigma=SIGMA, zoom=zoom, camera=camera, out_size=out_size)
    if plane == 0:
        return fn_luma(g, L, ROWS, COLS, t, synth.D_TRUE, **kw)
    return fn_chroma(g, L, ROWS, COLS, t, synth.D_TRUE, site, **kw)


def plane_masks(L, plane, site, zoom, camera, out_size):
    """-> (in_range, out_of_range) of a plane's output samples: the LENS camera's from its model range (wc.range_masks with
    its MARGIN); a PINHOLE camera gives every sample a ray"""
    orows, ocols = out_shape(out_size)
    shape = (orows, ocols) if plane == 0 else (orows // 2, ocols // 2)
    if camera == sr.PINHOLE:
        return np.ones(shape, bool), np.zeros(shape, bool)
    return wc.range_masks(plane_camera_lens(L, plane, site, zoom, out_size), wc.grid(*shape))


@functools.lru_cache(maxsize=None)
def plane_case(name, motion, plane=0, site=cr.CENTER, camera=sr.LENS, zoom=ZOOM, out_size=None, time_index=1):
    """one map of a plane -> dict(lens, gyro, time, delay, m64, in_range, out_of_range, compared, tol, rows, cols: the
    source plane's size); read-only.  The tolerance is wc.tolerance's: four times the float32-to-float64 spread of the
    restatement over the compared samples of this case."""
    L, g, t = lens(name), wc.gyro(motion), float(wc.frame_times()[time_index])
    m64 = plane_maps(sr.map64, cr.chroma_map64, g, L, t, plane, site, zoom, camera, out_size)
    m32 = plane_maps(sr.map32, cr.chroma_map32, g, L, t, plane, site, zoom, camera, out_size)
    inr, outr = plane_masks(L, plane, site, zoom, camera, out_size)
    rows, cols = (ROWS, COLS) if plane == 0 else (C_ROWS, C_COLS)
    compared = inr & wc.near_frame(m64, rows, cols)
    for a in (m64, inr, outr, compared):
        a.setflags(write=False)
    return dict(lens=L, gyro=g, time=t, delay=synth.D_TRUE, m64=m64, in_range=inr, out_of_range=outr, compared=compared,
                tol=wc.tolerance(m32, m64, compared), rows=rows, cols=cols)


def outside_counts(name, motion, plane=0, site=cr.CENTER, camera=sr.LENS, zoom=ZOOM):
    """the float64 map's count of samples that are not inside the plane, per frame"""
    out = []
    for k in range(N_FRAMES):
        c = plane_case(name, motion, plane, site, camera, zoom, None, k)
        out.append(int((~sr.inside(c["m64"], c["rows"], c["cols"])).sum()))
    return out


# ---- checks shared by the device tests ----------------------------------------------------------------------------------
def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_map(what, got, c, rows, cols):
    """test_gpu_warp_lenses' three assertions for one map of the device against a plane_case: compared samples within the
    case's tolerance, the other in-range samples outside on both sides, out-of-range samples NaN -> the device's distance"""
    assert got.shape == c["m64"].shape and got.dtype == np.float32, what
    cmp_, inr, outr = c["compared"], c["in_range"], c["out_of_range"]
    assert np.isfinite(got[inr]).all(), what
    worst = float(np.abs(got.astype(np.float64) - c["m64"])[cmp_].max())
    print("%s: %.3g px (tolerance %.3g, %d compared of %d in range, %d out of range)" % (what, worst, c["tol"], cmp_.sum(), inr.sum(), outr.sum()))
    assert worst <= c["tol"], what
    far = inr & ~cmp_
    assert not sr.inside(got, rows, cols)[far].any() and not sr.inside(c["m64"], rows, cols)[far].any(), what
    assert np.isnan(got[outr]).all(), what
    return worst


def padded(shape, dtype, value):
    """an array with a frame of padding around (n, rows, cols[, c]) and the view into it"""
    n, rows, cols = shape[:3]
    whole = np.full((n, rows + 3, cols + 9) + tuple(shape[3:]), value, dtype)
    return whole, whole[:, 1:1 + rows, 4:4 + cols]


# ---- planes of noise ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise8(n=N_FRAMES, seed=23):
    """n frames: y (n, 94, 170), u, v (n, 47, 85), uv, rgba; uint8, read-only"""
    rng = np.random.default_rng([seed, ROWS, COLS])
    y = rng.integers(0, 256, (n, ROWS, COLS), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (n, C_ROWS, C_COLS), dtype=np.uint8) for _ in range(2))
    d = dict(y=y, u=u, v=v, uv=np.stack([u, v], -1), rgba=rng.integers(0, 256, (n, ROWS, COLS, 4), dtype=np.uint8))
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def noise16(depth, n=N_FRAMES, seed=29):
    """n frames of sample VALUES over the whole range of `depth` bits: y, u, v, uv; uint16, read-only"""
    rng = np.random.default_rng([seed, depth])
    y = rng.integers(0, 1 << depth, (n, ROWS, COLS), dtype=np.uint16)
    u, v = (rng.integers(0, 1 << depth, (n, C_ROWS, C_COLS), dtype=np.uint16) for _ in range(2))
    d = dict(y=y, u=u, v=v, uv=np.stack([u, v], -1))
    for a in d.values():
        a.setflags(write=False)
    return d


# ---- the colour front's formats: their noise planes, fills and numpy samplers ------------------------------------------------
# (shared by tests/test_gpu_render_lenses.py and tests/test_gpu_infill_lenses.py)
GRAY8, NV12, I420, RGBA32 = 0, 1, 2, 3
GRAY16, P010, P016, I010 = 16, 17, 18, 19
COLOR_SIBLING = {GRAY16: GRAY8, P010: NV12, P016: NV12, I010: I420}
COLOR_DEPTH = {GRAY8: 8, NV12: 8, I420: 8, RGBA32: 8, GRAY16: 16, P010: 10, P016: 16, I010: 10}
FILLS8 = (7, 99, 200, 31)
FILLS16 = {10: (70, 300, 900), 16: (700, 30000, 60000)}               # sample values


def color_frames(fmt, sub=slice(None)):
    """the noise planes of a format as the calls take them (stored words) -> frames argument"""
    if fmt in COLOR_SIBLING:
        d = noise16(COLOR_DEPTH[fmt])
        y, u, v, uv = (c16.pack(fmt, (d[k][sub],))[0] for k in ("y", "u", "v", "uv"))
    else:
        d = noise8()
        y, u, v, uv = (d[k][sub] for k in ("y", "u", "v", "uv"))
    return {GRAY8: y, NV12: (y, uv), I420: (y, u, v), RGBA32: noise8()["rgba"][sub]}[COLOR_SIBLING.get(fmt, fmt)]


def color_fills(fmt):
    f = FILLS16[COLOR_DEPTH[fmt]] if fmt in COLOR_SIBLING else FILLS8
    return f if fmt == RGBA32 else f[:1] if fmt in (GRAY8, GRAY16) else f[:3]


def as_tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def color_sample_plane(fmt, k, words, m, fill, filter):
    """plane k of a format (stored words) through the numpy sampler on a map -> (stored words, samples filled): the 8-bit
    restatements, and for the 16-bit formats the same arithmetic on the sample values"""
    pairs = words.ndim == 3 and words.shape[-1] == 2
    if fmt == RGBA32:
        return (cr.sample_rgba if filter == 0 else q.sample_bicubic_rgba)(words, m, fill)
    if fmt not in COLOR_SIBLING:
        if pairs:
            return (cr.sample_pairs if filter == 0 else q.sample_bicubic_pairs)(words, m, fill)
        return (sr.sample if filter == 0 else q.sample_bicubic)(words, m, fill)
    if filter == 1:
        return q.sample_bicubic_pairs16(fmt, words, m, fill) if pairs else q.sample_bicubic16(fmt, words, m, fill)
    (vals,) = c16.unpack(fmt, (words,))
    out, n = c16.sample_pairs16(vals, m, fill) if pairs else c16.sample16(vals, m, fill)
    return c16.pack(fmt, (out,))[0], n


def color_plane_fill(fmt, k, fills):
    """the fill argument of plane k's sampler"""
    if fmt == RGBA32:
        return fills
    if k == 0:
        return fills[0]
    return (fills[1], fills[2]) if COLOR_SIBLING.get(fmt, fmt) == NV12 else fills[k]


# ---- fits ---------------------------------------------------------------------------------------------------------------
FIT_LO, FIT_HI, FIT_STEPS = 1.0, 3.0, 10
CLEAR, NOT_CLEAR = zr.CLEAR, zr.NOT_CLEAR

# Zoom fits in [1, 3]: name -> (lens, motion, camera, steps, luma k, luma status, chroma k, chroma status): the float64
# bisection's zooms 1 + 2 k / 2^steps of plane 0 and of the chroma plane (CENTER siting) per frame, plain, liberal and
# conservative alike (tests/test_render_cases_cpu.py proves that and the values).  Every lens x motion x camera:
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import render_cases as rc; rc.print_fits()"
# 'nonmono' and 'half' under x1 with the LENS camera are set by imageability alone: the frame itself is clear from 1.06 on,
# the border has a ray from 2.6 (2.17) on.  The band of MARGIN around the model's range is 0.0026 zoom wide there, more than
# a step of the ten-step bisection (0.002), in which the liberal and the conservative reading cannot agree; with six and
# seven steps they do.  Most other x20 cases are not clear at 3 in any frame, and 'half' under roll is not either.
FIT_CASES = {
    "half-x20-lens": ("half", "x20", sr.LENS, 10, (852, 946, 804), (0, 0, 0), (850, 945, 803), (0, 0, 0)),
    "negmild-x20-lens": ("negmild", "x20", sr.LENS, 10, (1024, 1024, 691), (1, 1, 0), (1024, 1024, 709), (1, 1, 0)),
    "synth-roll-lens": ("synth", "roll", sr.LENS, 10, (499, 495, 491), (0, 0, 0), (508, 504, 500), (0, 0, 0)),
    "aniso-roll-lens": ("aniso", "roll", sr.LENS, 10, (341, 337, 335), (0, 0, 0), (350, 347, 344), (0, 0, 0)),
    "nonmono-x1-lens": ("nonmono", "x1", sr.LENS, 6, (52, 52, 52), (0, 0, 0), (51, 51, 51), (0, 0, 0)),
    "half-x1-lens": ("half", "x1", sr.LENS, 7, (75, 75, 75), (0, 0, 0), (75, 75, 75), (0, 0, 0)),
    "half-x20-pinhole": ("half", "x20", sr.PINHOLE, 10, (192, 256, 85), (0, 0, 0), (198, 262, 92), (0, 0, 0)),
    "negmild-x20-pinhole": ("negmild", "x20", sr.PINHOLE, 10, (1024, 1024, 631), (1, 1, 0), (1024, 1024, 652), (1, 1, 0)),
    "aniso-roll-pinhole": ("aniso", "roll", sr.PINHOLE, 10, (164, 160, 157), (0, 0, 0), (178, 174, 170), (0, 0, 0)),
}
IMAGEABILITY_FITS = ("nonmono-x1-lens", "half-x1-lens")
# Strength fits, ten steps: name -> (lens, motion, camera, zoom, strengths in 1024ths, statuses).  With the LENS camera
# 'half' has no ray for a part of its border below zoom 2.17: its case runs at 2.7, and at 1.1 under the scene's own motion --
# where the frame itself is clear, as the pinhole camera's strength 1 at that zoom shows -- every frame is not clear for
# that reason alone.
STRENGTH_CASES = {
    "half-x1-lens-no-ray": ("half", "x1", sr.LENS, 1.1, (0, 0, 0), (1, 1, 1)),
    "half-x1-pinhole": ("half", "x1", sr.PINHOLE, 1.1, (1024, 1024, 1024), (0, 0, 0)),
    "aniso-x20-lens": ("aniso", "x20", sr.LENS, 1.1, (28, 92, 81), (0, 0, 0)),
    "strong-x20-lens": ("strong", "x20", sr.LENS, 1.1, (0, 40, 0), (1, 0, 1)),
    "half-x20-lens": ("half", "x20", sr.LENS, 2.7, (1024, 966, 1024), (0, 0, 0)),
    "half-x20-pinhole": ("half", "x20", sr.PINHOLE, 1.1, (894, 867, 994), (0, 0, 0)),
    "strong-x20-pinhole": ("strong", "x20", sr.PINHOLE, 1.1, (0, 39, 8), (1, 0, 0)),
    "negmild-x20-pinhole": ("negmild", "x20", sr.PINHOLE, 1.1, (230, 293, 402), (0, 0, 0)),
}


def fit_zooms(k, steps):
    return np.array([FIT_LO + (FIT_HI - FIT_LO) * v / (1 << steps) for v in k], np.float64)


def fit_strengths(k):
    return np.array([v / 1024 for v in k], np.float64)


def fit_tolerance(name, motion, camera, zoom, plane=0, site=cr.CENTER):
    """The tolerance of a fit's near-edge band.  A border pixel's ray at a zoom z >= lo is a ray of the whole output at
    zoom lo (the border moves inwards as the zoom grows), so the float32-to-float64 spread of the whole plane's map at the
    smallest zoom the fit visits bounds the border's at every zoom; four times that, as everywhere."""
    return plane_case(name, motion, plane, site, camera, zoom)["tol"]


def luma_borders(name, motion, camera, targets=None):
    L, g = lens(name), wc.gyro(motion)
    return [zr.frame_border(g, L, ROWS, COLS, t, synth.D_TRUE, target=None if targets is None else targets[f], sigma=SIGMA, camera=camera,
                            margin=wc.MARGIN) for f, t in enumerate(wc.frame_times())]


def chroma_borders(name, motion, camera, site=cr.CENTER):
    """include/rssync_colorzoom.h, step 2 and 3: the chroma plane as a camera of its own -- the chroma lens, half the size,
    the chroma frame times, the chroma output camera at zoom 1 -- against the path at the LUMA's frame times"""
    L, g = lens(name), wc.gyro(motion)
    targets = sr.path64(g, wc.frame_times(), L[0], synth.D_TRUE, SIGMA)
    return [zr.frame_border(g, cr.chroma_lens(L, site), C_ROWS, C_COLS, cr.chroma_time(t, L, ROWS, site), synth.D_TRUE, target=targets[f],
                            camera=camera, cam=cr.chroma_camera(L, ROWS, COLS, ROWS, COLS, site), margin=wc.MARGIN)
            for f, t in enumerate(wc.frame_times())]


def zoom_readings(borders, lo, hi, tol, steps=FIT_STEPS):
    """-> [(zooms, status)] of the plain, the liberal and the conservative reading"""
    return [zr.fit64(borders, lo, hi, steps, mode, tol) for mode in (zr.PLAIN, zr.LIBERAL, zr.CONSERVATIVE)]


def strength_frames(name, motion, camera, zoom):
    L, g = lens(name), wc.gyro(motion)
    return [lr.limited_frame(t, zoom, sigma=SIGMA, gyro=g, lens=L, size=(ROWS, COLS), camera=camera, margin=wc.MARGIN) for t in wc.frame_times()]


def strength_readings(frames, tol):
    return [lr.fit64(frames, FIT_STEPS, mode, tol) for mode in (lr.PLAIN, lr.LIBERAL, lr.CONSERVATIVE)]


def agree(readings):
    (z0, s0) = readings[0]
    return all((z == z0).all() and (s == s0).all() for z, s in readings[1:])


def print_fits():
    """every lens x motion x camera at lo = 1, hi = 3: the three readings and whether they agree"""
    for name in LENSES + ("wide",):
        for motion in MOTIONS:
            for camera in CAMERAS:
                tol = fit_tolerance(name, motion, camera, FIT_LO)
                r = zoom_readings(luma_borders(name, motion, camera), FIT_LO, FIT_HI, tol)
                rc_ = zoom_readings(chroma_borders(name, motion, camera), FIT_LO, FIT_HI, fit_tolerance(name, motion, camera, FIT_LO, 1))
                print("%-8s %-5s %d  luma %s %s %s  chroma %s %s %s" % (name, motion, camera, ((r[0][0] - FIT_LO) * 512).tolist(), r[0][1].tolist(),
                                                                         agree(r), ((rc_[0][0] - FIT_LO) * 512).tolist(), rc_[0][1].tolist(), agree(rc_)))
    for name in LENSES:
        for motion in MOTIONS:
            for camera in CAMERAS:
                for zoom in (1.1, 1.3):
                    r = strength_readings(strength_frames(name, motion, camera, zoom), fit_tolerance(name, motion, camera, zoom))
                    print("%-8s %-5s %d zoom %.1f strengths %s %s %s" % (name, motion, camera, zoom, (r[0][0] * 1024).tolist(), r[0][1].tolist(), agree(r)))


# ---- infill -------------------------------------------------------------------------------------------------------------
def compose_plane(frames, maps, rows, cols, fill, sample):
    """The infilled picture of one frame of one plane from the maps of its candidates in infill_reference.candidates' order
    (maps[k]: the map of candidate k's time against this frame's target; frames[k]: that candidate's plane): every sample
    from the first candidate whose position is inside, by `sample(frame, positions) -> values`; `fill` where none is.
    -> (picture, place: the donor's place in the order, -1 where filled).  infill_reference.first_hits' rule on given maps."""
    place = np.full(maps[0].shape[:2], -1, np.int64)
    for k in range(len(maps) - 1, -1, -1):
        place[sr.inside(maps[k], rows, cols)] = k
    out = np.empty(place.shape + frames[0].shape[2:], frames[0].dtype)
    out[...] = np.asarray(fill, frames[0].dtype)
    for k in range(len(maps)):
        sel = place == k
        if sel.any():
            out[sel] = sample(frames[k], maps[k][sel][None])[0]
    return out, place


def infill_hits(name, motion, plane, f, site=cr.CENTER):
    """infill_reference.first_hits of frame f in a plane's camera: float64, LENS, zoom ZOOM, the path's targets"""
    L, g, times = lens(name), wc.gyro(motion), wc.frame_times()
    targets = sr.path64(g, times, L[0], synth.D_TRUE, SIGMA)
    if plane == 0:
        return ir.first_hits(g, L, ROWS, COLS, times, synth.D_TRUE, targets, INFILL_RADIUS, f, zoom=ZOOM)
    times_c = np.array([cr.chroma_time(t, L, ROWS, site) for t in times])
    return ir.first_hits(g, cr.chroma_lens(L, site), C_ROWS, C_COLS, times_c, synth.D_TRUE, targets, INFILL_RADIUS, f,
                         cam=cr.chroma_camera(L, ROWS, COLS, ROWS, COLS, site, ZOOM))


# ---- the cache sequence (section g) ---------------------------------------------------------------------------------------
CACHE_ROWS, CACHE_COLS = 38, 30
CACHE_OUT = (22, 26)                     # cols, rows of the sequence's other output size


def cache_lenses():
    """A = 'aniso' at 38 x 30; B = A with k4 changed by 1e-3"""
    A = wc.lens("aniso", CACHE_ROWS, CACHE_COLS)
    return A, tuple(A[:8]) + (A[8] + 1e-3,)
