"""numpy restatement of the rectifier (include/rssync_rectify.h, csrc/rectify_math.hpp), and the scene its tests share.

  map64     the map of every output pixel in float64: the algorithm as the header states it (ray, table of rows + 1
            matrices, `iterations` rounds of lerp + project), nothing rounded
  map32     the same with every stage rounded where the device rounds it: rays and table stored as float32, the
            iteration in float32
  sample    the bilinear sampler in float32 in the device's order of operations: from the DEVICE's map it gives the
            device's bytes
  forward_points   rolling-shutter position -> rectified position, closed form, float64

The rays come from synth.unproject (plain Newton with the true derivative, 40 steps): the inverse of the forward model.
The device starts from the driver's nine-step schedule, whose slope has 8 k4 for 9 k4; that schedule alone agrees with the
true inverse far below a float32 ulp for synth.LENS, but not for every lens (tests/pixel_cases.py's `wide`: 1.3e-2 px at
the border of 1520 x 2704), so rect_pixel_ray polishes it with the true derivative -- tests/warp_cases.py holds the
device to this reference for eight lenses.  Positions a lens cannot image get a clipped, meaningless ray here and a NaN
ray on the device: compare in range only (warp_cases.range_masks).
"""
import functools

import numpy as np

from rssync_amd import synth, synth_video as sv

ROWS, COLS = 380, 676          # the quarter-size frame of the ground-truth scene
F0, N_FRAMES, SEED = 32, 3, 77


# Mean absolute grey difference to the global-shutter truth over the inside pixels at least 8 px from the border, frames
# 32, 33, 34, of the float64 reference (3 iterations, delay D_TRUE, default ref_row) and of the unrectified frames:
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import rectify_reference as rr; from rssync_amd import synth
#   s, maps = rr.scene(), rr.reference_maps()
#   for k in range(3):
#       ok = rr.inside(maps[k]); img, n = rr.sample(s['frames'][k], maps[k])
#       print(rr.grey_error(img, s['truth'][k], ok), rr.grey_error(s['frames'][k], s['truth'][k], ok), n / ok.size)"
# -> 0.1692 1.5172 0.0069 / 0.1520 0.2416 0.0067 / 0.1787 1.2467 0.0022
REFERENCE_ERROR = (0.1692, 0.1520, 0.1787)
UNRECTIFIED_ERROR = (1.5172, 0.2416, 1.2467)
RATIO = 0.25       # rectified <= RATIO x unrectified on frames 32 and 34 (33 is near-static at that instant)


def scaled_lens(rows, cols, lens=synth.LENS):
    """synth.LENS (a 1520 x 2704 image) for a rows x cols image of the same field of view"""
    ro, fx, fy, cx, cy = lens[:5]
    return (ro, fx * cols / synth.IMAGE_COLS, fy * rows / synth.IMAGE_ROWS, cx * cols / synth.IMAGE_COLS,
            cy * rows / synth.IMAGE_ROWS) + tuple(lens[5:])


def rot_matrix(q):
    """R(q) (..., 3, 3) of unit quaternions (..., 4): R(q) v = synth.rotate(q, v)"""
    eye = np.eye(3)
    return np.stack([synth.rotate(q, np.broadcast_to(eye[i], q.shape[:-1] + (3,))) for i in range(3)], axis=-1)


def row_table(gyro, lens, rows, frame_time, delay, ref_row=None):
    """(rows + 1, 3, 3) float64: M_j = R(q(T + ro j / rows + delay)) R(q_ref)^T"""
    ro = lens[0]
    ref_row = rows / 2 if ref_row is None else ref_row
    q = gyro.orientation(frame_time + ro * (np.arange(rows + 1) / rows) + delay)
    q_ref = gyro.orientation(frame_time + ro * (ref_row / rows) + delay)
    return rot_matrix(q) @ rot_matrix(q_ref).T


def pixel_rays(lens, rows, cols):
    ys, xs = np.mgrid[0:rows, 0:cols]
    return synth.unproject(np.stack([xs, ys], axis=-1).astype(np.float64), lens)


def _project(c, lens, dtype):
    fx, fy, cx, cy, k1, k2, k3, k4 = (dtype(v) for v in lens[1:])
    h = np.sqrt(c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1])
    th = np.arctan2(h, c[..., 2])
    t2 = th * th
    thd = th * (dtype(1) + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    s = np.where(h > 0, thd / np.where(h > 0, h, dtype(1)), dtype(0))
    return fx * (s * c[..., 0]) + cx, fy * (s * c[..., 1]) + cy


def _iterate(rays, table, lens, rows, iterations, dtype):
    v = np.arange(rows, dtype=dtype)[:, None]
    x = np.zeros(rays.shape[:2], dtype)
    y = np.broadcast_to(v, rays.shape[:2]).astype(dtype)
    for _ in range(iterations):
        yc = np.clip(y, dtype(0), dtype(rows - 1))
        fl = np.floor(yc)
        i = fl.astype(np.int64)
        f = (yc - fl)[..., None, None]
        M = table[i] + f * (table[i + 1] - table[i])
        c = np.stack([(M[..., r, 0] * rays[..., 0] + M[..., r, 1] * rays[..., 1]) + M[..., r, 2] * rays[..., 2] for r in range(3)],
                     axis=-1)
        x, y = _project(c, lens, dtype)
    return np.stack([x, y], axis=-1)


def map64(gyro, lens, rows, cols, frame_time, delay, ref_row=None, iterations=3):
    """(rows, cols, 2) float64 source positions"""
    return _iterate(pixel_rays(lens, rows, cols), row_table(gyro, lens, rows, frame_time, delay, ref_row), lens, rows, iterations,
                    np.float64)


def map32(gyro, lens, rows, cols, frame_time, delay, ref_row=None, iterations=3):
    """(rows, cols, 2) float32: the device's roundings -- rays and table computed in float64 and stored as float32, the
    iteration in float32"""
    rays = pixel_rays(lens, rows, cols).astype(np.float32)
    table = row_table(gyro, lens, rows, frame_time, delay, ref_row).astype(np.float32)
    return _iterate(rays, table, lens, rows, iterations, np.float32)


def inside(map_xy):
    rows, cols = map_xy.shape[:2]
    x, y = map_xy[..., 0], map_xy[..., 1]
    return (x >= 0) & (x <= cols - 1) & (y >= 0) & (y <= rows - 1)


def sample(frame, map_xy, fill=0):
    """-> (rectified (rows, cols) uint8, pixels filled): float32, one operation at a time, in the device's order"""
    rows, cols = frame.shape
    m = map_xy.astype(np.float32)
    ok = inside(m)
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
    out = np.rint(val).astype(np.uint8)
    out[~ok] = fill
    return out, int((~ok).sum())


def forward_points(gyro, lens, rows, frame_time, delay, points, ref_row=None):
    """rolling-shutter positions (..., 2) -> project(R(q_ref) R(q(row time + delay))^T ray), float64"""
    ro = lens[0]
    ref_row = rows / 2 if ref_row is None else ref_row
    points = np.asarray(points, np.float64)
    q = gyro.orientation(frame_time + ro * (points[..., 1] / rows) + delay)
    q_ref = gyro.orientation(frame_time + ro * (ref_row / rows) + delay)
    world = synth.rotate_inv(q, synth.unproject(points, lens))
    return synth.project(synth.rotate(np.broadcast_to(q_ref, q.shape), world), lens)


def border_mask(rows, cols, margin):
    m = np.zeros((rows, cols), bool)
    m[margin:rows - margin, margin:cols - margin] = True
    return m


def grey_error(img, truth, ok, margin=8):
    """mean absolute grey difference over the inside pixels at least `margin` px from the border"""
    sel = ok & border_mask(img.shape[0], img.shape[1], margin)
    return float(np.abs(img.astype(np.float64) - truth.astype(np.float64))[sel].mean())


@functools.lru_cache(maxsize=None)
def scene():
    """The ground-truth scene: three rolling-shutter frames of the synthetic video at a quarter of the lens's size, and the
    same frames from a global-shutter camera at the orientation of the middle row's time -- render() gives every row the
    orientation at time + ro * row / rows + d_true and one camera position per frame, so with ro = 0 and
    d_true = D_TRUE + ro / 2 it renders exactly what rotation-only rectification to ref_row = rows / 2 aims at.
    -> dict(gyro, lens, frames, times, truth); computed once per process, the arrays are read-only."""
    gyro = synth.make_gyro(1.0, 1.0 + 12 / synth.FPS, seed=SEED)         # t0 = 0
    lens = scaled_lens(ROWS, COLS)
    frames, times = sv.render(gyro, F0, F0 + N_FRAMES, lens=lens, rows=ROWS, cols=COLS, seed=SEED)
    truth, _ = sv.render(gyro, F0, F0 + N_FRAMES, lens=(0.0,) + tuple(lens[1:]), rows=ROWS, cols=COLS, seed=SEED,
                         d_true=synth.D_TRUE + lens[0] / 2)
    for a in (frames, times, truth):
        a.setflags(write=False)
    return dict(gyro=gyro, lens=lens, frames=frames, times=times, truth=truth)


@functools.lru_cache(maxsize=None)
def reference_maps():
    """the float64 maps of the scene's three frames at delay D_TRUE, default ref_row, 3 iterations (read-only)"""
    s = scene()
    maps = [map64(s["gyro"], s["lens"], ROWS, COLS, t, synth.D_TRUE) for t in s["times"]]
    for m in maps:
        m.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def device_tolerance():
    """px: four times the largest difference between the float32 and the float64 restatement of the map at 380 x 676
    (frame 32, delay D_TRUE).  The factor covers another atan2f, an approximate division and another order of
    operations; the number comes from the reference alone, never from the device."""
    s = scene()
    m32 = map32(s["gyro"], s["lens"], ROWS, COLS, s["times"][0], synth.D_TRUE)
    return 4.0 * float(np.abs(m32.astype(np.float64) - reference_maps()[0]).max())
