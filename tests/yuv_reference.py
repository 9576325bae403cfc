"""numpy restatement of the 4:2:2 and 4:4:4 formats (include/rssync_yuv.h, csrc/color_math.hpp), built on the stabiliser's
(tests/stabilize_reference.py) and the colour front's (tests/color_reference.py): a 4:2:2 chroma plane is the image of a
camera of its own, halved in x alone, so its map IS sr.map64 / sr.map32 with the chroma lens, the frame's own time, the chroma
output camera and the luma's target.  A 4:4:4 frame's planes all have the luma's map.

  chroma_lens422, chroma_camera422       the header's formulas, float64, in its operations
  chroma_map64 / chroma_map32            the map of every output chroma sample, in chroma-plane coordinates
  scene                                  the 4:2:2 scene: Y = rr.scene()'s frames; U and V rendered at 380 x 338 through the
                                         chroma lens with cr's texture seeds on the same camera path, as cr.scene renders its
  truth                                  U and V as a global-shutter chroma camera at the path's orientations sees them
"""
import functools

import numpy as np

import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr
from rssync_amd import synth, synth_video as sv

CENTER, LEFT = cr.CENTER, cr.LEFT
OFFSET = {CENTER: 0.5, LEFT: 0.0}            # ox: there is no vertical offset
C_ROWS, C_COLS = rr.ROWS, rr.COLS // 2       # 380 x 338

# Mean absolute grey difference of the 4:2:2 chroma planes to the global-shutter truth at the path's orientation (sigma
# 0.1 s, LENS, same size, delay D_TRUE, 3 iterations) over the inside samples at least 8 from the border, of the float64
# reference and of the raw planes, per siting, per plane (U, V), frames 32, 33, 34:
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import yuv_reference as yr; yr.print_figures()"
# -> the two lines per siting below, the float32 spread of the chroma map per camera and siting, and how far a chroma
#    sample's ray lies from the ray of its luma position (fp64)
#    (7.5e-5 / 8.7e-5 chroma px centre / left with the lens's camera, 8.4e-5 / 7.3e-5 with a pinhole; 6.3e-5 .. 8.4e-5 into
#    131 x 198), and 0 for the rays: halving fx and cx - ox is exact, so the two divisions see the same quotient
REFERENCE_ERROR = {
    CENTER: ((0.2723, 0.2794, 0.2783), (0.2819, 0.2892, 0.2869)),
    LEFT: ((0.2723, 0.2798, 0.2771), (0.2854, 0.2917, 0.2876)),
}
RAW_ERROR = {
    CENTER: ((29.9, 35.3, 34.2), (36.1, 42.4, 40.4)),
    LEFT: ((29.9, 35.3, 34.2), (36.1, 42.4, 40.4)),
}
MAP_SPREAD = 9e-5     # chroma px: the float32 restatement against the float64 one, the largest over cameras, sitings and sizes as first measured (8.71e-5)
RAY_AGREEMENT = 1e-15 # the largest component difference of the two unit rays over a grid of cameras, both sitings (fp64): measured 0


def _half_x(fx, fy, cx, cy, site):
    return fx * 0.5, fy, (cx - OFFSET[site]) * 0.5, cy


def chroma_lens422(lens, site=CENTER):
    """ro, fx * 0.5, fy, (cx - ox) * 0.5, cy, k1 .. k4"""
    return (lens[0],) + _half_x(lens[1], lens[2], lens[3], lens[4], site) + tuple(lens[5:])


def chroma_camera422(lens, rows, cols, out_rows, out_cols, site=CENTER, zoom=1.0, cam=None):
    """the luma output camera after defaults, scaling and zoom, as the camera of the 4:2:2 chroma grid"""
    return _half_x(*sr.out_camera(lens, rows, cols, out_rows, out_cols, zoom, cam), site)


def _chroma_map(fn, gyro, lens, rows, cols, frame_time, delay, site, target, sigma, out_size, zoom, camera, cam, iterations):
    oc, orows = (cols, rows) if out_size is None else out_size
    # one target per frame for all planes: the path at the frame's centre time, or the caller's; the time is the frame's
    q_t = sr.path64(gyro, np.array([frame_time]), lens[0], delay, sigma)[0] if target is None else sr.unit(target)
    return fn(gyro, chroma_lens422(lens, site), rows, cols // 2, frame_time, delay, target=q_t, out_size=(oc // 2, orows), camera=camera,
              cam=chroma_camera422(lens, rows, cols, orows, oc, site, zoom, cam), iterations=iterations)


def chroma_map64(gyro, lens, rows, cols, frame_time, delay, site=CENTER, target=None, sigma=0.0, out_size=None, zoom=1.0, camera=sr.LENS,
                 cam=None, iterations=3):
    """(out_rows, out_cols / 2, 2) float64 source positions in the rows x cols / 2 chroma plane; rows, cols, out_size
    (cols, rows), zoom and cam are the LUMA's"""
    return _chroma_map(sr.map64, gyro, lens, rows, cols, frame_time, delay, site, target, sigma, out_size, zoom, camera, cam, iterations)


def chroma_map32(gyro, lens, rows, cols, frame_time, delay, site=CENTER, target=None, sigma=0.0, out_size=None, zoom=1.0, camera=sr.LENS,
                 cam=None, iterations=3):
    """the device's roundings (sr.map32)"""
    return _chroma_map(sr.map32, gyro, lens, rows, cols, frame_time, delay, site, target, sigma, out_size, zoom, camera, cam, iterations)


@functools.lru_cache(maxsize=None)
def scene(site=CENTER):
    """The 4:2:2 scene (read-only): rr.scene() with Y = its frames, and U, V (3, 380, 338) rendered through the chroma lens
    with the textures of cr.U_SEED and cr.V_SEED: chroma row j at T + ro * j / 380 + D_TRUE, the luma row's time."""
    s = dict(rr.scene())
    lens_c = chroma_lens422(s["lens"], site)
    for name, seed in (("u", cr.U_SEED), ("v", cr.V_SEED)):
        s[name], _ = sv.render(s["gyro"], rr.F0, rr.F0 + rr.N_FRAMES, lens=lens_c, rows=C_ROWS, cols=C_COLS, seed=rr.SEED,
                               d_true=synth.D_TRUE, texture_seed=seed)
        s[name].setflags(write=False)
    s["y"] = s["frames"]
    s["uv"] = np.stack([s["u"], s["v"]], axis=-1)
    s["uv"].setflags(write=False)
    s["lens_c"] = lens_c
    return s


@functools.lru_cache(maxsize=None)
def truth(site=CENTER, sigma=sr.SIGMA):
    """(U, V) (3, 380, 338) as a global-shutter chroma camera at the path's orientations sees them (read-only)"""
    s = scene(site)
    lens = (0.0,) + tuple(s["lens_c"][1:])
    out = []
    for seed in (cr.U_SEED, cr.V_SEED):
        t = np.stack([sv.render(sr.fixed(q), rr.F0 + k, rr.F0 + k + 1, lens=lens, rows=C_ROWS, cols=C_COLS, seed=rr.SEED, d_true=0.0,
                                texture_seed=seed)[0][0] for k, q in enumerate(sr.path(sigma))])
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_maps(site=CENTER, sigma=sr.SIGMA):
    """the float64 chroma maps of the scene's three frames along the path: LENS, same size, zoom 1 (read-only)"""
    s = rr.scene()
    maps = [chroma_map64(s["gyro"], s["lens"], rr.ROWS, rr.COLS, t, synth.D_TRUE, site, sigma=sigma) for t in s["times"]]
    for m in maps:
        m.setflags(write=False)
    return maps


def map_spread(camera=sr.LENS, site=CENTER, out_size=None):
    """px of the chroma plane: the largest difference between the float32 and the float64 restatement of the chroma map
    (frame 32, delay D_TRUE, the path at sigma 0.1, zoom 1)"""
    s = rr.scene()
    args = (s["gyro"], s["lens"], rr.ROWS, rr.COLS, s["times"][0], synth.D_TRUE, site)
    kw = dict(sigma=sr.SIGMA, camera=camera, out_size=out_size)
    return float(np.abs(chroma_map32(*args, **kw).astype(np.float64) - chroma_map64(*args, **kw)).max())


@functools.lru_cache(maxsize=None)
def device_tolerance(camera=sr.LENS):
    """px of the chroma plane: four times the float32 restatement's distance from the float64 one for that camera at
    380 x 338, the larger of the two sitings: cr.device_tolerance's rule, the number from the reference alone."""
    return 4.0 * max(map_spread(camera, CENTER), map_spread(camera, LEFT))


def ray_agreement(lens, site, n=9):
    """the largest component difference between the unit ray of chroma sample (cu, cv) through the chroma lens and the ray
    of luma position (2 cu + ox, cv) through the lens, over an n x n grid of samples: one camera, up to fp64 rounding"""
    cols, rows = int(round(2 * lens[3])), int(round(2 * lens[4]))
    cu, cv = np.meshgrid(np.linspace(0, cols // 2 - 1, n), np.linspace(0, rows - 1, n))
    pc = np.stack([cu, cv], axis=-1)
    pl = np.stack([2.0 * cu + OFFSET[site], cv], axis=-1)
    return float(np.abs(synth.unproject(pc, chroma_lens422(lens, site)) - synth.unproject(pl, tuple(lens))).max())


def chroma_errors(site, images=None):
    """per plane (U, V) and frame: (error of `images` -- None: the float64 reference's --, error of the raw plane) against
    the truth, over the reference map's inside samples"""
    s, maps, tr = scene(site), reference_maps(site), truth(site)
    out = []
    for p, name in enumerate(("u", "v")):
        row = []
        for k in range(rr.N_FRAMES):
            ok = sr.inside(maps[k], C_ROWS, C_COLS)
            img = sr.sample(s[name][k], maps[k])[0] if images is None else images[p][k]
            row.append((rr.grey_error(img, tr[p][k], ok), rr.grey_error(s[name][k], tr[p][k], ok)))
        out.append(row)
    return out


def lens_grid():
    """cameras of several sizes and aspect ratios: the scene's lens scaled"""
    return [rr.scaled_lens(rows, cols) for rows, cols in ((3, 4), (5, 130), (31, 38), (199, 330), (rr.ROWS, rr.COLS), (1080, 1920))]


def print_figures():
    """the figures the constants above were taken from"""
    for site in (CENTER, LEFT):
        e = chroma_errors(site)
        print("site %d reference" % site, tuple(tuple(round(x[0], 4) for x in row) for row in e))
        print("site %d raw      " % site, tuple(tuple(round(x[1], 1) for x in row) for row in e))
    for camera in (sr.LENS, sr.PINHOLE):
        for out_size in (None, (198, 131)):
            print("camera %d out %s float32 - float64: centre %.3g, left %.3g chroma px" %
                  (camera, out_size, map_spread(camera, CENTER, out_size), map_spread(camera, LEFT, out_size)))
    print("ray agreement: %.3g" % max(ray_agreement(lens, site) for lens in lens_grid() for site in (CENTER, LEFT)))
