"""Cases of tests/test_yuv_cases_cpu.py and tests/test_gpu_yuv_lenses.py: the 4:2:2 and 4:4:4 renderers (include/rssync_yuv.h,
include/rssync_zoomyuv.h) across the lenses and motions of tests/warp_cases.py, as tests/render_cases.py holds the cases of
the 4:2:0, RGBA and gray renderers.  Helpers only: numpy, render_cases, warp_cases and the restatements; nothing here looks
at the device.

  size     94 x 170 luma, 94 x 85 for the 4:2:2 chroma plane: one full 64 x 4 tile and a part of one across, a part-tile row
           below, an output width that is 2 mod 4; rc.OUT is the other output size, OUT444 an odd one for the 4:4:4 maps
  lenses   rc.LENSES, motions rc.MOTIONS, three frames at wc.frame_times(), delay synth.D_TRUE, path sigma rc.SIGMA
  planes   plane_case: plane 0 is rc.plane_case's; plane 1 holds the float64 and float32 restatement maps of the 4:2:2 chroma
           plane (yr.chroma_map64 / 32), the range masks of the chroma output camera taken as a lens, `compared` and the
           tolerance by wc.tolerance's rule
  samples  noise planes of 8, 10 and 16 bits in every format's layout, and sample_plane: one plane of stored words through
           the numpy samplers on a map
  fits     FIT_CASES: fits of the 4:2:2 chroma plane whose three float64 readings agree in every frame
  cache    cache_trap_cameras: a 4:2:0 and a 4:2:2 call whose chroma ray maps differ in their height alone
"""
import functools

import numpy as np

import color16_reference as c16
import color_reference as cr
import render_cases as rc
import resample_reference as q
import stabilize_reference as sr
import warp_cases as wc
import yuv_reference as yr
import zoom_reference as zr
from rssync_amd import synth

ROWS, COLS = rc.ROWS, rc.COLS
C_ROWS, C_COLS = ROWS, COLS // 2         # the 4:2:2 chroma plane: halved in x alone
OUT444 = (109, 61)                       # cols, rows: an odd output width, which 4:4:4 alone takes

I422, NV16, I444 = 32, 33, 34
I210, P210, P216, I410 = 48, 49, 50, 51
FORMATS = (I422, NV16, I444, I210, P210, P216, I410)
NAMES = {I422: "i422", NV16: "nv16", I444: "i444", I210: "i210", P210: "p210", P216: "p216", I410: "i410"}
SIBLING = {I210: I422, P210: NV16, P216: NV16, I410: I444}
DEPTH = {I422: 8, NV16: 8, I444: 8, I210: 10, P210: 10, P216: 16, I410: 10}
SHIFT = {P210: 6}                        # the container's: P210 keeps its ten bits in the high end of the word
F422 = (I422, NV16, I210, P210, P216)
F444 = (I444, I410)
# distinct fills per plane, in sample values of the format's depth
FILLS = {8: (7, 99, 200), 10: (70, 300, 900), 16: (700, 30000, 60000)}

# measured with the float64 restatement (tests/test_yuv_cases_cpu.py asserts them): output samples of the LENS camera beyond
# the model's range (by more than wc.MARGIN) at zoom 1.0: lens -> (luma, 4:2:2 chroma CENTER, 4:2:2 chroma LEFT)
UNIMAGEABLE = {
    "half": (7306, 3649, 3635), "nonmono": (11629, 5808, 5816), "negmild": (31, 15, 17), "aniso": (0, 0, 0), "strong": (0, 0, 0),
    "synth": (0, 0, 0),
}


def is_422(fmt):
    return fmt in F422


def plane_size(fmt, plane):
    """(rows, cols) of a source plane"""
    return (C_ROWS, C_COLS) if plane and is_422(fmt) else (ROWS, COLS)


def chroma_shape(out_size):
    orows, ocols = rc.out_shape(out_size)
    return orows, ocols // 2


def plane_camera_lens(L, plane, site, zoom, out_size):
    """the output camera of a plane as a lens tuple: plane 0 wc.stab_camera_lens, plane 1 yr.chroma_camera422 with the lens's
    readout time and k1 .. k4"""
    if plane == 0:
        return rc.plane_camera_lens(L, 0, site, zoom, out_size)
    orows, ocols = rc.out_shape(out_size)
    return (L[0],) + tuple(yr.chroma_camera422(L, ROWS, COLS, orows, ocols, site, zoom)) + tuple(L[5:])


def plane_masks(L, plane, site, zoom, camera, out_size):
    """-> (in_range, out_of_range) of a plane's output samples (rc.plane_masks with the 4:2:2 chroma extent)"""
    if plane == 0:
        return rc.plane_masks(L, 0, site, zoom, camera, out_size)
    shape = chroma_shape(out_size)
    if camera == sr.PINHOLE:
        return np.ones(shape, bool), np.zeros(shape, bool)
    return wc.range_masks(plane_camera_lens(L, 1, site, zoom, out_size), wc.grid(*shape))


@functools.lru_cache(maxsize=None)
def plane_case(name, motion, plane=0, site=cr.CENTER, camera=sr.LENS, zoom=rc.ZOOM, out_size=None, time_index=1):
    """rc.plane_case with the 4:2:2 chroma plane as plane 1; read-only"""
    if plane == 0:
        return rc.plane_case(name, motion, 0, cr.CENTER, camera, zoom, out_size, time_index)
    L, g, t = rc.lens(name), wc.gyro(motion), float(wc.frame_times()[time_index])
    m64 = rc.plane_maps(sr.map64, yr.chroma_map64, g, L, t, 1, site, zoom, camera, out_size)
    m32 = rc.plane_maps(sr.map32, yr.chroma_map32, g, L, t, 1, site, zoom, camera, out_size)
    inr, outr = plane_masks(L, 1, site, zoom, camera, out_size)
    compared = inr & wc.near_frame(m64, C_ROWS, C_COLS)
    for a in (m64, inr, outr, compared):
        a.setflags(write=False)
    return dict(lens=L, gyro=g, time=t, delay=synth.D_TRUE, m64=m64, in_range=inr, out_of_range=outr, compared=compared,
                tol=wc.tolerance(m32, m64, compared), rows=C_ROWS, cols=C_COLS)


def outside_counts(name, motion, plane=0, site=cr.CENTER, camera=sr.LENS, zoom=rc.ZOOM):
    """the float64 map's count of samples that are not inside the plane, per frame"""
    out = []
    for k in range(rc.N_FRAMES):
        c = plane_case(name, motion, plane, site, camera, zoom, None, k)
        out.append(int((~sr.inside(c["m64"], c["rows"], c["cols"])).sum()))
    return out


# ---- planes of noise and the numpy samplers ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise(depth, n=rc.N_FRAMES, seed=37):
    """n frames of sample VALUES over the whole range of `depth` bits: y (n, 94, 170), the 4:2:2 planes u, v (n, 94, 85), the
    4:4:4 planes u4, v4 (n, 94, 170); uint8 or uint16, read-only"""
    rng = np.random.default_rng([seed, depth])
    dtype = np.uint8 if depth == 8 else np.uint16
    d = dict(y=rng.integers(0, 1 << depth, (n, ROWS, COLS), dtype=dtype))
    for k in ("u", "v"):
        d[k] = rng.integers(0, 1 << depth, (n, C_ROWS, C_COLS), dtype=dtype)
    for k in ("u4", "v4"):
        d[k] = rng.integers(0, 1 << depth, (n, ROWS, COLS), dtype=dtype)
    for a in d.values():
        a.setflags(write=False)
    return d


def frames(fmt, sub=slice(None)):
    """the noise planes of a format as the calls take them: stored words (P210: value << 6) in the format's layout"""
    d = noise(DEPTH[fmt])
    s = SHIFT.get(fmt, 0)
    y, u, v, u4, v4 = (d[k][sub] << s if s else d[k][sub] for k in ("y", "u", "v", "u4", "v4"))
    return {I422: (y, u, v), NV16: (y, np.stack([u, v], axis=-1)), I444: (y, u4, v4)}[SIBLING.get(fmt, fmt)]


def fills(fmt):
    return FILLS[DEPTH[fmt]]


def plane_fill(fmt, k):
    """the fill argument of plane k's sampler: a sample value, or the pair of an interleaved plane"""
    f = fills(fmt)
    return (f[1], f[2]) if k == 1 and SIBLING.get(fmt, fmt) == NV16 else f[k]


def sample_plane(fmt, words, m, fill, filter):
    """one plane of a format (stored words; (rows, cols, 2): interleaved pairs) through the numpy sampler on a map -> (stored
    words, samples filled): the 8-bit restatements, and for the formats in 16-bit containers the same arithmetic on the sample
    values, the bicubic result clamped to the format's largest value"""
    pairs = words.ndim == 3
    if DEPTH[fmt] == 8:
        if pairs:
            return (cr.sample_pairs if filter == 0 else q.sample_bicubic_pairs)(words, m, fill)
        return (sr.sample if filter == 0 else q.sample_bicubic)(words, m, fill)
    s, vmax = SHIFT.get(fmt, 0), (1 << DEPTH[fmt]) - 1
    vals = np.ascontiguousarray(words >> s)
    assert vals.dtype == np.uint16 and vals.max() <= vmax
    if pairs:
        out, n = c16.sample_pairs16(vals, m, fill) if filter == 0 else q.sample_bicubic_pairs(vals, m, fill, vmax)
    else:
        out, n = c16.sample16(vals, m, fill) if filter == 0 else q.sample_bicubic(vals, m, fill, vmax)
    return (out << s).astype(np.uint16), n


# ---- fits -------------------------------------------------------------------------------------------------------------------
def chroma_borders(name, motion, camera, site=cr.CENTER):
    """include/rssync_zoomyuv.h: the 4:2:2 chroma plane as a camera of its own -- the chroma lens, rows x cols / 2, the chroma
    output camera at zoom 1 -- at the LUMA's frame times, against the path at those times"""
    L, g = rc.lens(name), wc.gyro(motion)
    targets = sr.path64(g, wc.frame_times(), L[0], synth.D_TRUE, rc.SIGMA)
    return [zr.frame_border(g, yr.chroma_lens422(L, site), C_ROWS, C_COLS, t, synth.D_TRUE, target=targets[f], camera=camera,
                            cam=yr.chroma_camera422(L, ROWS, COLS, ROWS, COLS, site), margin=wc.MARGIN)
            for f, t in enumerate(wc.frame_times())]


def fit_tolerance(name, motion, camera, zoom, plane=0, site=cr.CENTER):
    """rc.fit_tolerance's rule for either plane"""
    return plane_case(name, motion, plane, site, camera, zoom)["tol"]


@functools.lru_cache(maxsize=None)
def fit_readings(name, motion, camera, steps, plane, site=cr.CENTER):
    """-> [(zooms, status)] of the plain, the liberal and the conservative reading of the float64 bisection in
    [rc.FIT_LO, rc.FIT_HI]"""
    borders = rc.luma_borders(name, motion, camera) if plane == 0 else chroma_borders(name, motion, camera, site)
    return rc.zoom_readings(borders, rc.FIT_LO, rc.FIT_HI, fit_tolerance(name, motion, camera, rc.FIT_LO, plane, site), steps)


# Zoom fits in [1, 3] of rc.FIT_CASES' lenses, motions and cameras with either siting: name -> (lens, motion, camera, site,
# steps, luma k, luma status, chroma k, chroma status): the float64 bisection's zooms 1 + 2 k / 2^steps of plane 0 and of the
# 4:2:2 chroma plane per frame, plain, liberal and conservative alike (tests/test_yuv_cases_cpu.py proves that and the values).
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import yuv_cases as yc; yc.print_fits()"
# Where the readings disagree at rc.FIT_CASES' step count the case runs at another: FIT_STEPS_TRIED, the first that agrees.
FIT_STEPS_TRIED = (10, 9, 8, 7, 6, 5)
FIT_CASES = {
    "half-x20-lens-center": ("half", "x20", 0, 0, 10, (852, 946, 804), (0, 0, 0), (851, 944, 802), (0, 0, 0)),
    "half-x20-lens-left": ("half", "x20", 0, 1, 10, (852, 946, 804), (0, 0, 0), (849, 942, 800), (0, 0, 0)),
    "negmild-x20-lens-center": ("negmild", "x20", 0, 0, 10, (1024, 1024, 691), (1, 1, 0), (1024, 1024, 709), (1, 1, 0)),
    "negmild-x20-lens-left": ("negmild", "x20", 0, 1, 10, (1024, 1024, 691), (1, 1, 0), (1024, 1024, 727), (1, 1, 0)),
    "synth-roll-lens-center": ("synth", "roll", 0, 0, 10, (499, 495, 491), (0, 0, 0), (494, 489, 485), (0, 0, 0)),
    "synth-roll-lens-left": ("synth", "roll", 0, 1, 10, (499, 495, 491), (0, 0, 0), (489, 484, 480), (0, 0, 0)),
    "aniso-roll-lens-center": ("aniso", "roll", 0, 0, 8, (86, 85, 84), (0, 0, 0), (85, 84, 83), (0, 0, 0)),          # (disagree at 10 and 9)
    "aniso-roll-lens-left": ("aniso", "roll", 0, 1, 10, (341, 337, 335), (0, 0, 0), (332, 329, 326), (0, 0, 0)),
    "nonmono-x1-lens-center": ("nonmono", "x1", 0, 0, 6, (52, 52, 52), (0, 0, 0), (51, 51, 51), (0, 0, 0)),
    "nonmono-x1-lens-left": ("nonmono", "x1", 0, 1, 6, (52, 52, 52), (0, 0, 0), (52, 52, 52), (0, 0, 0)),
    "half-x1-lens-center": ("half", "x1", 0, 0, 7, (75, 75, 75), (0, 0, 0), (75, 75, 75), (0, 0, 0)),
    "half-x1-lens-left": ("half", "x1", 0, 1, 5, (19, 19, 19), (0, 0, 0), (19, 19, 19), (0, 0, 0)),                # (disagree at 6 .. 10)
    "half-x20-pinhole-center": ("half", "x20", 1, 0, 10, (192, 256, 85), (0, 0, 0), (192, 256, 85), (0, 0, 0)),
    "half-x20-pinhole-left": ("half", "x20", 1, 1, 10, (192, 256, 85), (0, 0, 0), (192, 256, 85), (0, 0, 0)),
    "negmild-x20-pinhole-center": ("negmild", "x20", 1, 0, 10, (1024, 1024, 631), (1, 1, 0), (1024, 1024, 631), (1, 1, 0)),
    "negmild-x20-pinhole-left": ("negmild", "x20", 1, 1, 10, (1024, 1024, 631), (1, 1, 0), (1024, 1024, 631), (1, 1, 0)),
    "aniso-roll-pinhole-center": ("aniso", "roll", 1, 0, 10, (164, 160, 157), (0, 0, 0), (160, 156, 153), (0, 0, 0)),
    "aniso-roll-pinhole-left": ("aniso", "roll", 1, 1, 10, (164, 160, 157), (0, 0, 0), (156, 152, 149), (0, 0, 0)),
}
# what decides a frame's zoom: the chroma plane (frame 2 of 'negmild' under x20 with the LENS camera), the luma plane ('half'
# under x20 and 'synth' under roll with the LENS camera); 'negmild' under x20 holds clear and not-clear frames in one call
CHROMA_DECIDES = ("negmild-x20-lens-center", "negmild-x20-lens-left")
LUMA_DECIDES = ("half-x20-lens-center", "synth-roll-lens-center", "aniso-roll-lens-left")
MIXED_STATUS = ("negmild-x20-lens-center", "negmild-x20-pinhole-left")


def print_fits():
    """every case of rc.FIT_CASES with both sitings at the first step count of FIT_STEPS_TRIED (rc's own first) at which the
    three readings of both planes agree, as a line of FIT_CASES"""
    for case, (name, motion, camera, steps0, *_r) in rc.FIT_CASES.items():
        for site in rc.SITES:
            for steps in (steps0,) + tuple(s for s in FIT_STEPS_TRIED if s != steps0):
                rl, rc_ = fit_readings(name, motion, camera, steps, 0), fit_readings(name, motion, camera, steps, 1, site)
                if rc.agree(rl) and rc.agree(rc_):
                    k = [tuple(int(round((z - rc.FIT_LO) / (rc.FIT_HI - rc.FIT_LO) * (1 << steps))) for z in r[0][0]) for r in (rl, rc_)]
                    st = [tuple(int(s) for s in r[0][1]) for r in (rl, rc_)]
                    print('    "%s-%s": ("%s", "%s", %d, %d, %d, %s, %s, %s, %s),' % (case, ("center", "left")[site], name, motion, camera, site, steps,
                                                                                   k[0], st[0], k[1], st[1]))
                    break
                print("    # %s site %d: the readings disagree at %d steps" % (case, site, steps))


# ---- the cache sequence (section e) ---------------------------------------------------------------------------------------
def cache_trap_cameras():
    """`out_camera` arguments (an NV12 call's, an NV16 call's) at rc.CACHE_ROWS x rc.CACHE_COLS whose chroma cameras are the
    same four numbers -- fy doubled and cy = 2 cy' + 0.5 for the 4:2:0 call, every operation exact -- so that the two chroma
    ray maps differ in nothing but their height: the 4:2:0 map is the upper half of the 4:2:2 map, and a cache that took the
    one for the other would leave the lower half as the call before left it"""
    A, _ = rc.cache_lenses()
    cy = round(A[4] * 8) / 8
    return (A[1], 2 * A[2], A[3], 2 * cy + 0.5), (A[1], A[2], A[3], cy)


def print_unimageable():
    for name in rc.LENSES:
        L = rc.lens(name)
        print('"%s": (%d, %d, %d),' % (name, plane_masks(L, 0, cr.CENTER, 1.0, sr.LENS, None)[1].sum(),
                                       plane_masks(L, 1, cr.CENTER, 1.0, sr.LENS, None)[1].sum(), plane_masks(L, 1, cr.LEFT, 1.0, sr.LENS, None)[1].sum()))
