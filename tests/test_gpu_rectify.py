"""The rectifier on the device (include/rssync_rectify.h, csrc/kernels/rectify.hpp) against its numpy restatement
(tests/rectify_reference.py) and the synthetic video's global-shutter ground truth."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import rectify_reference as rr
from rectify_reference import RATIO, REFERENCE_ERROR

pytestmark = pytest.mark.gpu


def _problem(gyro=None):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    if gyro is not None:
        p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def scene(built):
    s = dict(rr.scene())
    s["problem"] = _problem(s["gyro"])
    return s


@pytest.fixture(scope="module")
def rectified(scene):
    """the scene's three frames through the device, with the device's own maps (read-only)"""
    from rssync_amd import synth
    p = scene["problem"]
    out, n_out = p.rectify_frames(scene["frames"], scene["times"], scene["lens"], synth.D_TRUE)
    maps = [p.rectify_map(rr.COLS, rr.ROWS, scene["lens"], t, synth.D_TRUE) for t in scene["times"]]
    for a in [out, n_out] + maps:
        a.setflags(write=False)
    return out, n_out, maps


def _grid(rows, cols):
    ys, xs = np.mgrid[0:rows, 0:cols]
    return np.stack([xs, ys], axis=-1).astype(np.float64)


@pytest.mark.parametrize("rows,cols,extra_delay,iterations,ref_row", [
    (rr.ROWS, rr.COLS, 0.0, 3, None), (rr.ROWS, rr.COLS, 0.02, 3, None), (rr.ROWS, rr.COLS, 0.0, 1, None),
    (rr.ROWS, rr.COLS, 0.0, 3, 0), (rr.ROWS, rr.COLS, 0.02, 1, rr.ROWS),
    (331, 197, 0.0, 3, None), (331, 197, 0.02, 1, 331), (37, 29, 0.0, 3, None), (37, 29, 0.02, 1, 0), (37, 29, 0.0, 3, 37)])
def test_map_against_the_float64_reference(scene, rows, cols, extra_delay, iterations, ref_row):
    """380 x 676, and two sizes that are no multiple of the 64 x 4 tile, one of them smaller than a tile"""
    from rssync_amd import synth
    lens = rr.scaled_lens(rows, cols)
    delay, t = synth.D_TRUE + extra_delay, scene["times"][1]
    got = scene["problem"].rectify_map(cols, rows, lens, t, delay, ref_row=ref_row, iterations=iterations)
    want = rr.map64(scene["gyro"], lens, rows, cols, t, delay, ref_row=ref_row, iterations=iterations)
    assert got.shape == want.shape and got.dtype == np.float32
    diff = np.abs(got.astype(np.float64) - want).max()
    print("%d x %d delay %.3f iterations %d ref_row %s: %.3g px (tolerance %.3g)" % (rows, cols, delay, iterations, ref_row, diff,
                                                                                     rr.device_tolerance()))
    assert diff <= rr.device_tolerance()


def test_sampler_is_the_float32_restatement_bit_for_bit(scene, rectified):
    """from the device's own map the restated sampler gives the device's bytes; pitched input and output, the padding of
    the output untouched"""
    from rssync_amd import synth
    p, frames = scene["problem"], scene["frames"]
    out, n_out, maps = rectified
    wide = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS + 45), np.uint8)
    wide[:, :, 7:7 + rr.COLS] = frames
    dst = np.full((rr.N_FRAMES, rr.ROWS + 3, rr.COLS + 21), 201, np.uint8)
    view = dst[:, 1:1 + rr.ROWS, 5:5 + rr.COLS]
    got, got_n = p.rectify_frames(wide[:, :, 7:7 + rr.COLS], scene["times"], scene["lens"], synth.D_TRUE, fill=77, out=view)
    assert got is view
    for k in range(rr.N_FRAMES):
        want, want_n = rr.sample(frames[k], maps[k], fill=77)
        np.testing.assert_array_equal(view[k], want, err_msg="frame %d" % k)
        assert int(got_n[k]) == want_n == int(n_out[k]) and want_n > 0
        filled = ~rr.inside(maps[k])
        np.testing.assert_array_equal(out[k][~filled], want[~filled])
        assert (out[k][filled] == 0).all()
    pad = np.ones(dst.shape, bool)
    pad[:, 1:1 + rr.ROWS, 5:5 + rr.COLS] = False
    assert (dst[pad] == 201).all()


def test_error_against_the_global_shutter_truth(scene, rectified):
    out, n_out, maps = rectified
    frames, truth, ref_maps = scene["frames"], scene["truth"], rr.reference_maps()
    for k in range(rr.N_FRAMES):
        ok = rr.inside(maps[k])
        err = rr.grey_error(out[k], truth[k], ok)
        raw = rr.grey_error(frames[k], truth[k], ok)
        ref_img, _ = rr.sample(frames[k], ref_maps[k])
        ref_ok = rr.inside(ref_maps[k])
        both = ok & ref_ok
        worst = np.abs(out[k].astype(int) - ref_img.astype(int))[both].max()
        flips = (ok != ref_ok).mean()
        print("frame %d: device %.4f reference %.4f unrectified %.4f; device against reference image: %d grey levels, "
              "%.2g of the inside flags differ" % (rr.F0 + k, err, REFERENCE_ERROR[k], raw, worst, flips))
        assert err <= 1.05 * REFERENCE_ERROR[k], (k, err)
        if k != 1:
            assert err <= RATIO * raw, (k, err, raw)
        assert worst <= 1 and flips <= 1e-3, (k, worst, flips)


def _noise(n=2, seed=11):
    return np.random.default_rng(seed).integers(0, 256, size=(n, rr.ROWS, rr.COLS), dtype=np.uint8)


def _assert_identity(out, frames):
    np.testing.assert_array_equal(out[:, 1:-1, 1:-1], frames[:, 1:-1, 1:-1])


def test_no_readout_time_is_the_identity(scene):
    """random noise: the worst case for interpolation"""
    from rssync_amd import synth
    frames = _noise()
    lens = (0.0,) + tuple(scene["lens"][1:])
    out, _ = scene["problem"].rectify_frames(frames, scene["times"][:2], lens, synth.D_TRUE)
    _assert_identity(out, frames)


def test_a_camera_at_rest_is_the_identity(scene, built):
    from rssync_amd import synth
    g = scene["gyro"]
    quats = np.zeros_like(g.quats)
    quats[:, 0] = 1.0
    p = _problem()
    p.SetGyroQuaternions(quats, g.fs, g.t0)
    frames = _noise()
    assert scene["lens"][0] == synth.READOUT
    out, _ = p.rectify_frames(frames, scene["times"][:2], scene["lens"], synth.D_TRUE)
    _assert_identity(out, frames)


def test_host_device_and_pitched_buffers_agree(scene, rectified):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    want, want_n, _ = rectified
    wide = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS + 61), np.uint8)
    wide[:, :, 13:13 + rr.COLS] = frames
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")
    dwide = torch.from_numpy(wide).to("cuda:0")
    for src in (wide[:, :, 13:13 + rr.COLS], dev, dwide[:, :, 13:13 + rr.COLS]):
        got, n = p.rectify_frames(src, times, lens, synth.D_TRUE)
        assert isinstance(got, torch.Tensor) == isinstance(src, torch.Tensor)
        np.testing.assert_array_equal(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
        np.testing.assert_array_equal(n, want_n)
    # device frames into a host array, host frames into a pitched device tensor
    host_out = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS), np.uint8)
    p.rectify_frames(dev, times, lens, synth.D_TRUE, out=host_out)
    np.testing.assert_array_equal(host_out, want)
    dout = torch.full((rr.N_FRAMES, rr.ROWS, rr.COLS + 19), 9, dtype=torch.uint8, device="cuda:0")
    p.rectify_frames(frames, times, lens, synth.D_TRUE, out=dout[:, :, 3:3 + rr.COLS])
    back = dout.cpu().numpy()
    np.testing.assert_array_equal(back[:, :, 3:3 + rr.COLS], want)
    assert (back[:, :, :3] == 9).all() and (back[:, :, 3 + rr.COLS:] == 9).all()


def test_frames_in_one_call_equal_frames_one_at_a_time(scene, rectified):
    from rssync_amd import synth
    want, want_n, _ = rectified
    for k in range(rr.N_FRAMES):
        got, n = scene["problem"].rectify_frames(scene["frames"][k:k + 1], scene["times"][k:k + 1], scene["lens"], synth.D_TRUE)
        np.testing.assert_array_equal(got[0], want[k])
        assert n[0] == want_n[k]


def test_chunk_boundaries_do_not_change_the_result(scene):
    """seven 37 x 29 frames with a budget of two and a half frames per slot: four chunks through both slots"""
    from rssync_amd import rectify, synth
    rows, cols, n = 37, 29, 7
    p, lens = scene["problem"], rr.scaled_lens(37, 29)
    frames = np.random.default_rng(3).integers(0, 256, size=(n, rows, cols), dtype=np.uint8)
    times = scene["times"][0] + np.arange(n) / synth.FPS
    want = [p.rectify_frames(frames[k:k + 1], times[k:k + 1], lens, synth.D_TRUE, fill=5) for k in range(n)]
    per_frame = (rows + 1) * 36 + 2 * rows * cols
    got, got_n = rectify.rectify_frames_budget(p, frames, times, lens, synth.D_TRUE, 2 * 2.5 * per_frame, fill=5)
    for k in range(n):
        np.testing.assert_array_equal(got[k], want[k][0][0], err_msg="frame %d" % k)
        assert got_n[k] == want[k][1][0]
    one, one_n = p.rectify_frames(frames, times, lens, synth.D_TRUE, fill=5)
    np.testing.assert_array_equal(one, got)
    np.testing.assert_array_equal(one_n, got_n)


def test_bad_arguments_return_an_error_and_the_next_call_works(scene, rectified):
    import rssync_amd
    from rssync_amd import rectify, synth
    p, frames, times, lens = scene["problem"], np.ascontiguousarray(scene["frames"]), scene["times"], scene["lens"]
    want = rectified[0]
    lib = rectify.library()
    lib.rssync_set_panic_mode(1)
    L = np.ascontiguousarray(lens, np.float64)
    T = np.ascontiguousarray(times, np.float64)
    out = np.zeros_like(frames)
    W, H, N = rr.COLS, rr.ROWS, rr.N_FRAMES
    PD = C.POINTER(C.c_double)

    def call(h=p._h, f=frames.ctypes.data, n=N, w=W, hh=H, pitch=W, stride=W * H, t=T, lens_=L, delay=synth.D_TRUE, prm=None, o=None,
             opitch=W, ostride=W * H):
        o = out.ctypes.data if o is None else o
        return lib.rssync_rectify_frames(h, f, n, w, hh, pitch, stride, t.ctypes.data_as(PD) if t is not None else None,
                                         lens_.ctypes.data if lens_ is not None else None, delay,
                                         C.byref(prm) if prm is not None else None, o if o else None, opitch, ostride, None)

    def bad(match, **kw):
        assert call(**kw) != 0, match
        msg = lib.rssync_last_error().decode()
        assert match in msg, (match, msg)

    def lens_with(i, v):
        m = L.copy()
        m[i] = v
        return m

    empty = _problem()
    bad("no gyro data", h=empty._h)
    bad("leaves the gyro data", delay=synth.D_TRUE + 5.0)
    bad("leaves the gyro data", delay=-2.0)
    bad("leaves the gyro data", t=np.array([times[0], 1e9, times[2]]))
    bad("no frames", f=None)
    bad("null output", o=0)
    bad("no frame times", t=None)
    bad("no lens", lens_=None)
    bad("pitch", pitch=W - 1)
    bad("out_pitch", opitch=W - 1)
    bad("too small", w=1, pitch=1)
    bad("too small", hh=1)
    bad("non-finite frame time", t=np.array([times[0], np.nan, times[2]]))
    bad("non-finite delay", delay=float("inf"))
    bad("negative readout", lens_=lens_with(0, -1e-3))
    bad("non-finite lens", lens_=lens_with(0, np.nan))
    bad("iterations", prm=rectify.RectifyParams(-1.0, 9, 0))
    bad("iterations", prm=rectify.RectifyParams(-1.0, -1, 0))
    bad("fill", prm=rectify.RectifyParams(-1.0, 3, 256))
    bad("ref_row", prm=rectify.RectifyParams(H + 0.5, 3, 0))
    bad("overlaps", o=frames.ctypes.data + W * H)
    # ... and the calls that follow work: NULL parameters, a zeroed struct and the spelled-out defaults are the same thing
    for prm in (None, rectify.RectifyParams(0.0, 0, 0), rectify.RectifyParams(H / 2, 3, 0)):
        out[:] = 0
        assert call(prm=prm) == 0, lib.rssync_last_error().decode()
        np.testing.assert_array_equal(out, want)
    m = np.zeros((H, W, 2), np.float32)
    assert lib.rssync_rectify_map(p._h, W, H, L.ctypes.data, float(times[0]), synth.D_TRUE, None, None) != 0
    assert lib.rssync_rectify_map(p._h, W, H, L.ctypes.data, float(times[0]), 9.0, None, m.ctypes.data) != 0
    assert "leaves the gyro data" in lib.rssync_last_error().decode()
    assert lib.rssync_rectify_points(p._h, None, 4, W, H, L.ctypes.data, float(times[0]), synth.D_TRUE, None, None) != 0
    with pytest.raises(rssync_amd.RsSyncError, match="ref_row"):
        p.rectify_map(W, H, lens, times[0], synth.D_TRUE, ref_row=H + 1)
    np.testing.assert_array_equal(p.rectify_map(W, H, lens, times[0], synth.D_TRUE), rectified[2][0])


def test_points_against_the_reference_and_as_the_inverse_of_the_map(scene, rectified):
    from rssync_amd import synth
    p, g, lens = scene["problem"], scene["gyro"], scene["lens"]
    t = scene["times"][0]
    rng = np.random.default_rng(8)
    pts = np.concatenate([rng.uniform((0, 0), (rr.COLS - 1, rr.ROWS - 1), size=(500, 2)),
                          [[0, 0], [rr.COLS - 1, rr.ROWS - 1], [lens[3], lens[4]], [0, rr.ROWS - 1]]])
    for ref_row in (None, 0, rr.ROWS):
        got = p.rectify_points(pts, rr.COLS, rr.ROWS, lens, t, synth.D_TRUE, ref_row=ref_row)
        want = rr.forward_points(g, lens, rr.ROWS, t, synth.D_TRUE, pts, ref_row=ref_row)
        worst = np.abs(got - want).max()
        print("ref_row %s: points against the reference %.3g px" % (ref_row, worst))
        assert worst <= 1e-9
    dev = p.rectify_points(torch.from_numpy(pts).to("cuda:0"), rr.COLS, rr.ROWS, lens, t, synth.D_TRUE)
    np.testing.assert_array_equal(dev.cpu().numpy(), p.rectify_points(pts, rr.COLS, rr.ROWS, lens, t, synth.D_TRUE))
    m = rectified[2][0]
    ok = rr.inside(m)
    back = p.rectify_points(m.astype(np.float64), rr.COLS, rr.ROWS, lens, t, synth.D_TRUE)
    worst = np.abs(back - _grid(rr.ROWS, rr.COLS))[ok].max()
    print("points o map: %.3g px (tolerance %.3g)" % (worst, rr.device_tolerance()))
    assert worst <= rr.device_tolerance()
