"""Rolling-shutter grayscale video of the synthetic scene (numpy only), with the ground truth of the tracker.

The camera of ``synth`` -- the gyro's orientation at row time + D_TRUE, the fisheye ``LENS``, 0.05 m of
translation per frame along ``make_pixel_frames``' direction -- looks at the inside of a box whose walls carry a
band-limited procedural texture: a sum of random 3-D sinusoids evaluated on the wall, with wavelengths chosen so
that a period covers at least ~8 pixels of the image (no aliasing) and enough of them in every direction that no
region is flat.  Every pixel's ray comes from ``unproject`` once per lens; each ROW has its own orientation
(row time = frame time + ro * y / rows, core_testcode.cpp:144-145), the camera position changes per frame.

``true_points`` is what an exact tracker would return for the driver's grid points: a's ray meets the box, the hit
point is re-projected into the next frame with the row-time iteration of ``make_pixel_frames``.
"""
import numpy as np

from . import synth

BOX = 6.0               # half side of the box (m); the camera starts at its centre
N_WAVES = 24
WAVELENGTH = (0.35, 2.5)  # m: >= ~8 px at the far corners under grazing view, half-resolution lens
FLAT_GRAY = 128           # render(flat=...): the flat region's value
FLAT_EDGE = 0.5           # m: the width of the band outside the flat region over which the texture fades in


def half_lens(lens=synth.LENS):
    """the same lens for a frame of half the size"""
    ro, fx, fy, cx, cy = lens[:5]
    return (ro, fx / 2, fy / 2, cx / 2, cy / 2) + tuple(lens[5:])


def _texture(seed):
    rng = np.random.default_rng([seed, 991])
    lam = np.exp(rng.uniform(np.log(WAVELENGTH[0]), np.log(WAVELENGTH[1]), N_WAVES))
    d = rng.normal(size=(N_WAVES, 3))
    k = (2 * np.pi / lam)[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)
    amp = lam / lam.max()                     # (a little more weight on the long waves: contrast at every scale)
    return k.astype(np.float32), rng.uniform(0, 2 * np.pi, N_WAVES).astype(np.float32), amp.astype(np.float32)


def _direction(frame, seed):
    ang = 0.002 * frame + 0.7 * seed          # make_pixel_frames' translation direction
    return np.array([np.cos(ang), np.sin(ang) * np.cos(0.3 * ang), np.sin(ang) * np.sin(0.3 * ang)])


def camera_position(frame, seed=0):
    """centre of frame `frame`: 0.05 m per frame from the box centre at frame 0"""
    return sum((0.05 * _direction(g, seed) for g in range(int(frame))), np.zeros(3))


def _hit(c, d):
    """first wall of the box [-BOX, BOX]^3 on the ray c + t d (c inside)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.sign(d) * BOX - c) / d
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf).min(axis=-1, keepdims=True)
    return c + t * d


def _shade(P, tex, weight=None):
    """weight (render's flat=): the texture's share, 0 = FLAT_GRAY"""
    k, ph, amp = tex
    s = np.sin(P.astype(np.float32) @ k.T + ph) @ amp
    v = 128.0 + 100.0 * s / np.sqrt(0.5 * (amp ** 2).sum()) / 2.0
    if weight is not None:
        v = np.where(weight < 1, FLAT_GRAY + weight * (v - FLAT_GRAY), v)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def render(gyro, frame_begin, frame_end, lens=synth.LENS, rows=synth.IMAGE_ROWS, cols=synth.IMAGE_COLS, seed=0,
           d_true=synth.D_TRUE, flat=None, texture_seed=None):
    """-> frames (n, rows, cols) uint8, frame_times (n,) s, for frames [frame_begin, frame_end).

    texture_seed: None = `seed`; else the walls carry that seed's texture while the camera still moves along `seed`'s
    path: another plane (the U or V of a colour frame) of the same shot.

    flat: None, or a world-space box ((x0, y0, z0), (x1, y1, z1)) whose part of the walls is rendered as constant gray
    FLAT_GRAY (sky, a blank wall), the texture fading in over FLAT_EDGE m around it.  Then a third result,
    mask (n, rows, cols) bool: the pixels that see the region."""
    ys, xs = np.mgrid[0:rows, 0:cols]
    rays = synth.unproject(np.stack([xs, ys], axis=-1).astype(np.float64), lens)   # (rows, cols, 3), once per lens
    tex = _texture(seed if texture_seed is None else texture_seed)
    ro = lens[0]
    n = frame_end - frame_begin
    out = np.empty((n, rows, cols), np.uint8)
    mask = np.zeros((n, rows, cols), bool) if flat is not None else None
    times = np.arange(frame_begin, frame_end) / synth.FPS
    for i, fr in enumerate(range(frame_begin, frame_end)):
        q = gyro.orientation(times[i] + ro * np.arange(rows) / rows + d_true)            # one orientation per row
        world = synth.rotate_inv(q[:, None, :], rays)
        P = _hit(camera_position(fr, seed), world)
        if flat is None:
            out[i] = _shade(P, tex)
        else:
            # distance of the wall point to the region: 0 inside (flat), the texture fades in over FLAT_EDGE outside it
            # -- a band-limited border like the texture's own, not an aliased step
            lo, hi = np.asarray(flat[0], np.float64), np.asarray(flat[1], np.float64)
            d = np.linalg.norm(np.maximum(np.maximum(lo - P, P - hi), 0.0), axis=-1)
            mask[i] = d == 0.0
            out[i] = _shade(P, tex, np.minimum(d / FLAT_EDGE, 1.0).astype(np.float32))
    if flat is not None:
        return out, times, mask
    return out, times


def true_points(gyro, frame_begin, frame_end, points, lens=synth.LENS, rows=synth.IMAGE_ROWS, seed=0, d_true=synth.D_TRUE):
    """-> (n-1, P, 2): where the grid points (P, 2) of frame f are in frame f+1, for f in [frame_begin, frame_end - 1)"""
    ro = lens[0]
    a_cam = synth.unproject(points, lens)
    out = np.zeros((frame_end - frame_begin - 1, points.shape[0], 2))
    for i, fr in enumerate(range(frame_begin, frame_end - 1)):
        t_a, t_b = fr / synth.FPS, (fr + 1) / synth.FPS
        qa = gyro.orientation(t_a + ro * points[:, 1] / rows + d_true)
        X = _hit(camera_position(fr, seed), synth.rotate_inv(qa, a_cam))
        v = X - camera_position(fr + 1, seed)
        v /= np.linalg.norm(v, axis=-1, keepdims=True)
        pb = points.copy()
        for _ in range(4):  # the row of the point in the next frame sets the time it is seen at (make_pixel_frames)
            pb = synth.project(synth.rotate(gyro.orientation(t_b + ro * pb[:, 1] / rows + d_true), v), lens)
        out[i] = pb
    return out
