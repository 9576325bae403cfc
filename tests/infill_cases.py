"""Cases of tests/test_infill_cases_cpu.py and tests/test_gpu_infill_lenses.py: the three infill kernel families -- gray
(include/rssync_infill.h), the colour front (include/rssync_colorinfill.h) and 4:2:2 / 4:4:4 (include/rssync_infillyuv.h) --
across the lenses and motions of tests/warp_cases.py, as tests/render_cases.py and tests/yuv_cases.py hold the renderers'
cases.  Helpers only: numpy, render_cases, yuv_cases, warp_cases and the restatements; nothing here looks at the device.

  size     94 x 170 luma (rc.ROWS, rc.COLS): one full 64 x 4 tile and a part of one across in every chroma plane
  frames   the three of wc.frame_times(), delay synth.D_TRUE, targets the path at rc.SIGMA, passed explicitly
  radius   2: the candidate orders are [0, 1, 2], [1, 0, 2], [2, 1, 0]; frame 0 skips the steps 1 and 3 (f - 1, f - 2),
           frame 2 the steps 2 and 4 (f + 1, f + 2)
  cases    CASES: lens, motion, zoom, camera, output size, and the siting of the 4:2:2 and of the 4:2:0 chroma plane
  planes   a plane is a camera: LUMA (and every plane of a 4:4:4, RGBA or gray frame), C422 (halved in x alone, the frames'
           times) and C420 (halved in both, the chroma frame times); geometry() is what infill_reference.first_hits takes
  counts   COUNTS: per case and plane the samples beyond the lens model's range and per frame [own, 2nd place, 3rd place,
           filled] over the samples in range, from the float64 restatement (tests/test_infill_cases_cpu.py asserts them).  The
           restatement extrapolates where the device has NaN, so samples that are not in range are left out of every count
  maps     map_case: one donor map -- candidate g's time against frame f's target -- as rc.check_map takes it
  formats  FORMATS: every format of the three families with its noise planes, fills and numpy samplers
"""
import collections
import functools

import numpy as np

import color_reference as cr
import infill_reference as ir
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
import yuv_cases as yc
import yuv_reference as yr
from rssync_amd import synth

RADIUS = 2
N_FRAMES = rc.N_FRAMES
ORDERS = ([0, 1, 2], [1, 0, 2], [2, 1, 0])
OUT = (rc.OUT[1], rc.OUT[0])             # cols, rows: 110 x 62
OUT_ODD = yc.OUT444                      # cols, rows: 109 x 61, which 4:4:4, RGBA and gray alone take
LUMA, C422, C420 = "luma", "422", "420"
KINDS = (LUMA, C422, C420)
MIN_COMPARED_SHARE = 0.25                # of a map's samples, as section e of tests/test_gpu_yuv_lenses.py asks
MIN_NAN = 9                              # samples without a ray that a 'half' plane must have

Case = collections.namedtuple("Case", "name lens motion zoom camera out_size site422 site420")
CASES = {c.name: c for c in (
    Case("half-x20", "half", "x20", 1.0, sr.LENS, None, cr.CENTER, cr.LEFT),
    Case("negmild-roll", "negmild", "roll", 1.1, sr.LENS, None, cr.LEFT, cr.LEFT),
    Case("strong-x20-pinhole", "strong", "x20", 1.1, sr.PINHOLE, None, cr.CENTER, cr.CENTER),
    Case("negmild-roll-out", "negmild", "roll", 1.1, sr.LENS, OUT, cr.CENTER, cr.LEFT),
    Case("half-x20-out", "half", "x20", 1.0, sr.LENS, OUT, cr.LEFT, cr.CENTER),
    Case("negmild-roll-odd", "negmild", "roll", 1.1, sr.LENS, OUT_ODD, cr.CENTER, cr.CENTER),
    Case("half-x20-odd", "half", "x20", 1.0, sr.LENS, OUT_ODD, cr.CENTER, cr.CENTER),
)}
INPUT_SIZE_CASES = ("half-x20", "negmild-roll", "strong-x20-pinhole")
RESIZED_CASES = ("negmild-roll-out", "half-x20-out")
ODD_CASES = ("negmild-roll-odd", "half-x20-odd")
CHUNK_CASES = ("half-x20", "strong-x20-pinhole")
HALF_CASES = tuple(n for n, c in CASES.items() if c.lens == "half")


def kinds(name):
    """the planes a case has: an odd output width has no chroma plane of its own"""
    return (LUMA,) if name in ODD_CASES else KINDS


# (case, plane) -> (samples that are not in range, per frame (own, 2nd place, 3rd place, filled) in range): float64
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import infill_cases as ic; ic.print_counts()"
COUNTS = {
    ("half-x20", LUMA): (7332, ((7039, 1, 84, 1524), (6633, 883, 87, 1045), (6727, 36, 475, 1410))),
    ("half-x20", C422): (3657, ((3516, 2, 47, 768), (3313, 448, 42, 530), (3361, 16, 238, 718))),
    ("half-x20", C420): (1822, ((1759, 0, 23, 391), (1656, 228, 22, 267), (1686, 8, 114, 365))),
    ("negmild-roll", LUMA): (0, ((11172, 1915, 1554, 1339), (11175, 1839, 1456, 1510), (11176, 1840, 1581, 1383))),
    ("negmild-roll", C422): (0, ((5588, 955, 783, 664), (5591, 921, 722, 756), (5594, 920, 794, 682))),
    ("negmild-roll", C420): (0, ((2776, 490, 390, 339), (2775, 471, 362, 387), (2776, 473, 399, 347))),
    ("strong-x20-pinhole", LUMA): (0, ((7349, 0, 0, 8631), (6867, 1678, 0, 7435), (7226, 0, 657, 8097))),
    ("strong-x20-pinhole", C422): (0, ((3669, 0, 0, 4321), (3429, 839, 0, 3722), (3605, 0, 330, 4055))),
    ("negmild-roll-out", LUMA): (0, ((4768, 818, 669, 565), (4770, 783, 627, 640), (4771, 782, 676, 591))),
    ("negmild-roll-out", C422): (0, ((2386, 410, 331, 283), (2387, 389, 312, 322), (2387, 387, 340, 296))),
    ("half-x20-out", LUMA): (3109, ((3022, 0, 38, 651), (2848, 379, 36, 448), (2888, 15, 204, 604))),
    ("strong-x20-pinhole", C420): (0, ((1823, 0, 0, 2172), (1704, 422, 0, 1869), (1792, 0, 170, 2033))),
    ("negmild-roll-out", C420): (0, ((1183, 205, 174, 143), (1185, 206, 154, 160), (1185, 205, 171, 144))),
    ("half-x20-out", C422): (1539, ((1524, 0, 18, 329), (1434, 195, 18, 224), (1451, 9, 104, 307))),
    ("half-x20-out", C420): (777, ((752, 0, 9, 167), (710, 94, 9, 115), (716, 3, 51, 158))),
    ("negmild-roll-odd", LUMA): (0, ((4650, 802, 650, 547), (4652, 761, 608, 628), (4653, 766, 657, 573))),
    ("half-x20-odd", LUMA): (3034, ((2947, 0, 35, 633), (2781, 368, 37, 429), (2817, 16, 198, 584))),
}


def case(name):
    return CASES[name]


def lens(c):
    return rc.lens(c.lens)


def site_of(c, kind):
    return {LUMA: cr.CENTER, C422: c.site422, C420: c.site420}[kind]


def source_size(kind):
    """(rows, cols) of a source plane"""
    return {LUMA: (rc.ROWS, rc.COLS), C422: (yc.C_ROWS, yc.C_COLS), C420: (rc.C_ROWS, rc.C_COLS)}[kind]


def out_shape(c, kind):
    """(rows, cols) of an output plane"""
    orows, ocols = rc.out_shape(c.out_size)
    return {LUMA: (orows, ocols), C422: (orows, ocols // 2), C420: (orows // 2, ocols // 2)}[kind]


def masks(c, kind):
    """-> (in_range, out_of_range) of a plane's output samples, from the plane's own output camera"""
    L = lens(c)
    if kind == C422:
        return yc.plane_masks(L, 1, c.site422, c.zoom, c.camera, c.out_size)
    return rc.plane_masks(L, 0 if kind == LUMA else 1, site_of(c, kind), c.zoom, c.camera, c.out_size)


def targets64(c):
    return sr.path64(wc.gyro(c.motion), wc.frame_times(), lens(c)[0], synth.D_TRUE, rc.SIGMA)


def geometry(c, kind):
    """-> (lens, rows, cols, frame times, kw) of a plane as a camera: infill_reference.first_hits' arguments"""
    L, times = lens(c), wc.frame_times()
    orows, ocols = rc.out_shape(c.out_size)
    if kind == LUMA:
        return L, rc.ROWS, rc.COLS, times, dict(zoom=c.zoom, camera=c.camera, out_size=c.out_size)
    if kind == C422:
        return (yr.chroma_lens422(L, c.site422), yc.C_ROWS, yc.C_COLS, times,
                dict(camera=c.camera, out_size=(ocols // 2, orows), cam=yr.chroma_camera422(L, rc.ROWS, rc.COLS, orows, ocols, c.site422, c.zoom)))
    times_c = np.array([cr.chroma_time(t, L, rc.ROWS, c.site420) for t in times])
    return (cr.chroma_lens(L, c.site420), rc.C_ROWS, rc.C_COLS, times_c,
            dict(camera=c.camera, out_size=(ocols // 2, orows // 2), cam=cr.chroma_camera(L, rc.ROWS, rc.COLS, orows, ocols, c.site420, c.zoom)))


@functools.lru_cache(maxsize=None)
def hits(name, kind, f):
    """infill_reference.first_hits' places of frame f in a plane's camera: float64, the path's targets; read-only"""
    c = case(name)
    L, rows, cols, times, kw = geometry(c, kind)
    place, _, _ = ir.first_hits(wc.gyro(c.motion), L, rows, cols, times, synth.D_TRUE, targets64(c), RADIUS, f, **kw)
    place.setflags(write=False)
    return place


def counts(name, kind):
    """-> (samples not in range, per frame [own, 2nd place, 3rd place, filled] over the samples in range)"""
    inr = masks(case(name), kind)[0]
    rows = []
    for f in range(N_FRAMES):
        place = hits(name, kind, f)[inr]
        rows.append(tuple(int((place == k).sum()) for k in (0, 1, 2)) + (int((place < 0).sum()),))
    return int((~inr).sum()), tuple(rows)


def print_counts():
    for name in CASES:
        for kind in kinds(name):
            print('    ("%s", %s): %s,' % (name, {LUMA: "LUMA", C422: "C422", C420: "C420"}[kind], counts(name, kind)))


# ---- donor maps ---------------------------------------------------------------------------------------------------------
def reference_map(c, kind, f, g, targets, fn=64):
    """the restatement's map of candidate g's time against frame f's target: float64, or float32 with the device's roundings"""
    L, t = lens(c), float(wc.frame_times()[g])
    kw = dict(target=targets[f], zoom=c.zoom, camera=c.camera, out_size=c.out_size)
    if kind == LUMA:
        return (sr.map64 if fn == 64 else sr.map32)(wc.gyro(c.motion), L, rc.ROWS, rc.COLS, t, synth.D_TRUE, **kw)
    mod = yr if kind == C422 else cr
    return (mod.chroma_map64 if fn == 64 else mod.chroma_map32)(wc.gyro(c.motion), L, rc.ROWS, rc.COLS, t, synth.D_TRUE, site_of(c, kind), **kw)


def map_case(c, kind, f, g, targets):
    """one donor map as rc.check_map takes it: the float64 map, the range masks of the plane's output camera, `compared` and
    the tolerance by wc.tolerance's rule -- four times the float32 restatement's distance from the float64 one over the
    compared samples of this very map"""
    m64, m32 = reference_map(c, kind, f, g, targets), reference_map(c, kind, f, g, targets, 32)
    inr, outr = masks(c, kind)
    compared = inr & wc.near_frame(m64, *source_size(kind))
    return dict(m64=m64, in_range=inr, out_of_range=outr, compared=compared, tol=wc.tolerance(m32, m64, compared))


def pairs():
    """every (f, g) of the three orders"""
    return [(f, g) for f in range(N_FRAMES) for g in ir.candidates(f, N_FRAMES, RADIUS)]


# ---- formats ------------------------------------------------------------------------------------------------------------
GRAY, COLOR, YUV = "gray", "color", "yuv"
# name -> (family: the call that takes it, the family's format number)
FORMATS = {
    "gray8": (GRAY, rc.GRAY8),
    "nv12": (COLOR, rc.NV12), "i420": (COLOR, rc.I420), "rgba32": (COLOR, rc.RGBA32), "p010": (COLOR, rc.P010), "p016": (COLOR, rc.P016),
    "i010": (COLOR, rc.I010), "gray16": (COLOR, rc.GRAY16),
    "i422": (YUV, yc.I422), "nv16": (YUV, yc.NV16), "i444": (YUV, yc.I444), "i210": (YUV, yc.I210), "p210": (YUV, yc.P210),
    "p216": (YUV, yc.P216), "i410": (YUV, yc.I410),
}
YUV_FORMATS = ("i422", "nv16", "i444", "i210", "p210", "p216", "i410")
COLOR_FORMATS = ("gray8", "nv12", "i420", "rgba32", "p010", "p016", "i010", "gray16")


def frames(name):
    """the noise planes of a format over its whole range, as the calls take them -> tuple of planes"""
    family, fmt = FORMATS[name]
    return tuple(yc.frames(fmt)) if family == YUV else rc.as_tuple(rc.color_frames(fmt))


def fills(name):
    """distinct fills per plane, in sample values"""
    family, fmt = FORMATS[name]
    return yc.fills(fmt) if family == YUV else rc.color_fills(fmt)


def plane_fill(name, k):
    """the fill argument of plane k's sampler"""
    family, fmt = FORMATS[name]
    return yc.plane_fill(fmt, k) if family == YUV else rc.color_plane_fill(fmt, k, fills(name))


def shift(name):
    """the container's: P010 and P210 keep their ten bits in the high end of the word"""
    return 6 if name in ("p010", "p210") else 0


def stored_fill(name, k):
    return np.asarray(plane_fill(name, k)) << shift(name)


def kind_of(name, k):
    """the camera of plane k of a format"""
    family, fmt = FORMATS[name]
    if k == 0:
        return LUMA
    if family == YUV:
        return C422 if fmt in yc.F422 else LUMA
    return C420 if rc.COLOR_SIBLING.get(fmt, fmt) in (rc.NV12, rc.I420) else LUMA


def sample(name, k, words, m, filter):
    """plane k of a format (stored words) through the numpy sampler on a map -> stored words"""
    family, fmt = FORMATS[name]
    if family == YUV:
        return yc.sample_plane(fmt, words, m, plane_fill(name, k), filter)[0]
    return rc.color_sample_plane(fmt, k, words, m, plane_fill(name, k), filter)[0]


def compose(name, k, src, maps, f, filter):
    """plane k of frame f composed from the maps of its candidates (maps[(f, g)]) -> (picture, place)"""
    cand = ir.candidates(f, N_FRAMES, RADIUS)
    rows, cols = source_size(kind_of(name, k))
    return rc.compose_plane([src[k][g] for g in cand], [maps[(f, g)] for g in cand], rows, cols, stored_fill(name, k),
                            lambda fr, m: sample(name, k, fr, m, filter))
