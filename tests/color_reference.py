"""numpy restatement of the colour front (include/rssync_color.h, csrc/color_math.hpp), built on the stabiliser's
(tests/stabilize_reference.py): a 4:2:0 chroma plane is the image of a camera of its own, so its map IS sr.map64 / sr.map32
with the chroma lens, the chroma frame time, the chroma output camera and the luma's target.

  chroma_lens, chroma_time, chroma_camera   the header's formulas, float64, in its operations
  chroma_map64 / chroma_map32               the map of every output chroma sample, in chroma-plane coordinates
  sample_pairs, sample_rgba                 sr.sample per channel: interleaved UV pairs, RGBA pixels
  scene                                     the colour scene: Y = rr.scene()'s frames; U and V rendered at 190 x 338 through
                                            the chroma lens with other texture seeds on the same camera path
"""
import functools

import numpy as np

import rectify_reference as rr
import stabilize_reference as sr
from rssync_amd import synth, synth_video as sv

CENTER, LEFT = 0, 1
OFFSET = {CENTER: (0.5, 0.5), LEFT: (0.0, 0.5)}
U_SEED, V_SEED = 1077, 2077                  # the textures of U and V (Y has rr.SEED's)
C_ROWS, C_COLS = rr.ROWS // 2, rr.COLS // 2  # 190 x 338

# Mean absolute grey difference of the chroma planes to the global-shutter truth at the path's orientation (sigma 0.1 s,
# LENS, same size, delay D_TRUE, 3 iterations) over the inside samples at least 8 from the border, of the float64
# reference and of the raw planes, per siting, per plane (U, V), frames 32, 33, 34:
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import color_reference as cr; cr.print_figures()"
# -> the two lines per siting below; float32 against float64 6.1e-5 (centre) and 6.8e-5 (left) chroma px with the lens's
#    camera, 5.6e-5 and 5.5e-5 with a pinhole
REFERENCE_ERROR = {
    CENTER: ((0.3027, 0.3211, 0.3173), (0.3563, 0.3707, 0.3688)),
    LEFT: ((0.3031, 0.3221, 0.3209), (0.3539, 0.3742, 0.3725)),
}
RAW_ERROR = {
    CENTER: ((29.9, 35.3, 34.2), (36.2, 42.6, 40.6)),
    LEFT: ((29.9, 35.2, 34.2), (36.2, 42.5, 40.6)),
}


def _half(fx, fy, cx, cy, site):
    ox, oy = OFFSET[site]
    return fx * 0.5, fy * 0.5, (cx - ox) * 0.5, (cy - oy) * 0.5


def chroma_lens(lens, site=CENTER):
    """ro, fx * 0.5, fy * 0.5, (cx - ox) * 0.5, (cy - oy) * 0.5, k1 .. k4"""
    return (lens[0],) + _half(lens[1], lens[2], lens[3], lens[4], site) + tuple(lens[5:])


def chroma_time(frame_time, lens, rows, site=CENTER):
    """T_c = T + ro * (oy / height): rows is the LUMA's height"""
    return frame_time + lens[0] * (OFFSET[site][1] / rows)


def chroma_camera(lens, rows, cols, out_rows, out_cols, site=CENTER, zoom=1.0, cam=None):
    """the luma output camera after defaults, scaling and zoom, as the camera of the chroma grid"""
    return _half(*sr.out_camera(lens, rows, cols, out_rows, out_cols, zoom, cam), site)


def _chroma_map(fn, gyro, lens, rows, cols, frame_time, delay, site, target, sigma, out_size, zoom, camera, cam, iterations):
    oc, orows = (cols, rows) if out_size is None else out_size
    # one target per frame for all planes: the path at the LUMA's centre time, or the caller's
    q_t = sr.path64(gyro, np.array([frame_time]), lens[0], delay, sigma)[0] if target is None else sr.unit(target)
    return fn(gyro, chroma_lens(lens, site), rows // 2, cols // 2, chroma_time(frame_time, lens, rows, site), delay, target=q_t,
              out_size=(oc // 2, orows // 2), camera=camera, cam=chroma_camera(lens, rows, cols, orows, oc, site, zoom, cam),
              iterations=iterations)


def chroma_map64(gyro, lens, rows, cols, frame_time, delay, site=CENTER, target=None, sigma=0.0, out_size=None, zoom=1.0, camera=sr.LENS,
                 cam=None, iterations=3):
    """(out_rows / 2, out_cols / 2, 2) float64 source positions in the rows / 2 x cols / 2 chroma plane; rows, cols,
    out_size (cols, rows), zoom and cam are the LUMA's"""
    return _chroma_map(sr.map64, gyro, lens, rows, cols, frame_time, delay, site, target, sigma, out_size, zoom, camera, cam, iterations)


def chroma_map32(gyro, lens, rows, cols, frame_time, delay, site=CENTER, target=None, sigma=0.0, out_size=None, zoom=1.0, camera=sr.LENS,
                 cam=None, iterations=3):
    """the device's roundings (sr.map32)"""
    return _chroma_map(sr.map32, gyro, lens, rows, cols, frame_time, delay, site, target, sigma, out_size, zoom, camera, cam, iterations)


def sample_pairs(uv, map_xy, fill=(128, 128)):
    """interleaved pairs (rows, cols, 2) at one position per pair -> (output (map rows, map cols, 2), samples filled)"""
    u, n = sr.sample(uv[..., 0], map_xy, fill[0])
    v, _ = sr.sample(uv[..., 1], map_xy, fill[1])
    return np.stack([u, v], axis=-1), n


def sample_rgba(img, map_xy, fill=(0, 0, 0, 255)):
    """(rows, cols, 4) at one position per pixel, sr.sample's arithmetic per channel -> (output, pixels filled)"""
    ch = [sr.sample(img[..., k], map_xy, fill[k]) for k in range(4)]
    return np.stack([c[0] for c in ch], axis=-1), ch[0][1]


@functools.lru_cache(maxsize=None)
def scene(site=CENTER):
    """The colour scene (read-only): rr.scene() with Y = its frames, and U, V (3, 190, 338) rendered through the chroma lens
    with the textures of U_SEED and V_SEED: each chroma row j at T + ro * j / 190 + D_TRUE + ro * oy / 380."""
    s = dict(rr.scene())
    lens_c = chroma_lens(s["lens"], site)
    d = synth.D_TRUE + s["lens"][0] * OFFSET[site][1] / rr.ROWS
    for name, seed in (("u", U_SEED), ("v", V_SEED)):
        s[name], _ = sv.render(s["gyro"], rr.F0, rr.F0 + rr.N_FRAMES, lens=lens_c, rows=C_ROWS, cols=C_COLS, seed=rr.SEED, d_true=d,
                               texture_seed=seed)
        s[name].setflags(write=False)
    s["y"] = s["frames"]
    s["uv"] = np.stack([s["u"], s["v"]], axis=-1)
    s["uv"].setflags(write=False)
    s["lens_c"] = lens_c
    return s


@functools.lru_cache(maxsize=None)
def truth(site=CENTER, sigma=sr.SIGMA):
    """(U, V) (3, 190, 338) as a global-shutter chroma camera at the path's orientations sees them (read-only)"""
    s = scene(site)
    lens = (0.0,) + tuple(s["lens_c"][1:])
    out = []
    for seed in (U_SEED, V_SEED):
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
    190 x 338, the larger of the two sitings.  The rectifier's rule (rr.device_tolerance), for its reason; the number comes
    from the reference alone, never from the device."""
    return 4.0 * max(map_spread(camera, CENTER), map_spread(camera, LEFT))


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


def print_figures():
    """the figures the constants above were taken from"""
    for site in (CENTER, LEFT):
        e = chroma_errors(site)
        print("site %d reference" % site, tuple(tuple(round(x[0], 4) for x in row) for row in e))
        print("site %d raw      " % site, tuple(tuple(round(x[1], 1) for x in row) for row in e))
    for camera in (sr.LENS, sr.PINHOLE):
        print("camera %d float32 - float64: centre %.3g, left %.3g chroma px" % (camera, map_spread(camera, CENTER), map_spread(camera, LEFT)))
