"""The stabiliser on the device (include/rssync_stabilize.h, csrc/kernels/stabilize.hpp) against the rectifier it is
anchored to, its numpy restatement (tests/stabilize_reference.py) and global-shutter renders of the synthetic video at the
smoothed path's orientations."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import rectify_reference as rr
import stabilize_reference as sr

pytestmark = pytest.mark.gpu

SMALL = (37, 29)       # rows, cols: smaller than one 64 x 4 tile
ODD = (331, 197)       # no multiple of the tile


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
def stabilised(scene):
    """the scene's three frames along the path at sigma 0.1 through the device, with the device's own maps (read-only)"""
    from rssync_amd import synth
    p = scene["problem"]
    out, n_out = p.stabilize_frames(scene["frames"], scene["times"], scene["lens"], synth.D_TRUE, sigma=sr.SIGMA)
    maps = [p.stabilize_map(rr.COLS, rr.ROWS, scene["lens"], t, synth.D_TRUE, sigma=sr.SIGMA) for t in scene["times"]]
    for a in [out, n_out] + maps:
        a.setflags(write=False)
    return out, n_out, maps


def _noise(n=2, seed=11, rows=rr.ROWS, cols=rr.COLS):
    return np.random.default_rng(seed).integers(0, 256, size=(n, rows, cols), dtype=np.uint8)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(rr.ROWS, rr.COLS), SMALL])
def test_anchor_without_smoothing_it_is_the_rectifier_bit_for_bit(scene, rows, cols):
    from rssync_amd import stabilize, synth
    p, times = scene["problem"], scene["times"]
    lens = scene["lens"] if rows == rr.ROWS else rr.scaled_lens(rows, cols)
    frames = scene["frames"] if rows == rr.ROWS else _noise(rr.N_FRAMES, 5, rows, cols)
    for t in times:
        want = p.rectify_map(cols, rows, lens, t, synth.D_TRUE)
        np.testing.assert_array_equal(p.stabilize_map(cols, rows, lens, t, synth.D_TRUE).view(np.uint32), want.view(np.uint32))
    want, want_n = p.rectify_frames(frames, times, lens, synth.D_TRUE)
    got, got_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_n, want_n)
    assert want_n.sum() > 0
    # NULL parameters and a zeroed struct are the defaults too
    lib = stabilize.library()
    L, T = np.ascontiguousarray(lens, np.float64), np.ascontiguousarray(times, np.float64)
    f = np.ascontiguousarray(frames)
    for prm in (None, C.byref(stabilize.StabilizeParams())):
        out = np.zeros_like(f)
        assert lib.rssync_stabilize_frames(p._h, f.ctypes.data, len(f), cols, rows, cols, rows * cols, T.ctypes.data_as(C.POINTER(C.c_double)),
                                           L.ctypes.data, synth.D_TRUE, None, prm, out.ctypes.data, cols, rows, cols, rows * cols, None) == 0
        np.testing.assert_array_equal(out, want)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.05, 0.2, 1.0])
def test_path_against_the_float64_reference(scene, sigma):
    """385 fp64 terms of magnitude at most 1 round by about 4e-14 at most: 1e-12 per component.  At sigma 1.0 the taps
    clamp at both ends of the 2.4 s of gyro data."""
    from rssync_amd import synth
    p, g, times, ro = scene["problem"], scene["gyro"], scene["times"], scene["lens"][0]
    if sigma == 1.0:
        lo, hi = sr.knot_span(g)
        assert times[0] + synth.D_TRUE - 3 * sigma < lo and times[-1] + synth.D_TRUE + 3 * sigma > hi
    got = p.stabilize_path(times, ro, synth.D_TRUE, sigma)
    want = sr.path64(g, times, ro, synth.D_TRUE, sigma)
    worst = np.abs(got - want).max()
    print("sigma %.2f: path against the reference %.3g" % (sigma, worst))
    assert got.shape == (3, 4) and worst <= 1e-12
    for k in range(3):
        one = p.stabilize_path(times[k:k + 1], ro, synth.D_TRUE, sigma)
        np.testing.assert_array_equal(one[0].view(np.uint64), got[k].view(np.uint64))
    dev = torch.zeros((3, 4), dtype=torch.float64, device="cuda:0")
    assert p.stabilize_path(times, ro, synth.D_TRUE, sigma, out=dev) is dev
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint64), got.view(np.uint64))


def test_path_without_smoothing_is_the_centre_orientation(scene):
    from rssync_amd import synth
    p, g, times, ro = scene["problem"], scene["gyro"], scene["times"], scene["lens"][0]
    got = p.stabilize_path(times, ro, synth.D_TRUE, 0.0)
    assert np.abs(got - sr.path64(g, times, ro, synth.D_TRUE, 0.0)).max() <= 1e-12


# 3 ---------------------------------------------------------------------------------------------------------------------
# (input rows, cols), output (rows, cols), camera, explicit target, zoom, iterations: every output size, both zooms, both
# iteration counts and both kinds of target with each camera
MAP_CASES = [
    ((rr.ROWS, rr.COLS), (rr.ROWS, rr.COLS), sr.LENS, False, 1.0, 3), ((rr.ROWS, rr.COLS), (rr.ROWS, rr.COLS), sr.LENS, True, 1.3, 1),
    ((rr.ROWS, rr.COLS), (200, 320), sr.LENS, True, 1.0, 3), ((rr.ROWS, rr.COLS), (200, 320), sr.LENS, False, 1.3, 3),
    ((rr.ROWS, rr.COLS), SMALL, sr.LENS, False, 1.3, 1), ((rr.ROWS, rr.COLS), SMALL, sr.LENS, True, 1.0, 3),
    (ODD, (64, 48), sr.LENS, False, 1.0, 3), (ODD, (64, 48), sr.LENS, True, 1.3, 1),
    ((rr.ROWS, rr.COLS), (rr.ROWS, rr.COLS), sr.PINHOLE, False, 1.0, 3), ((rr.ROWS, rr.COLS), (rr.ROWS, rr.COLS), sr.PINHOLE, True, 1.3, 1),
    ((rr.ROWS, rr.COLS), (200, 320), sr.PINHOLE, True, 1.0, 3), ((rr.ROWS, rr.COLS), (200, 320), sr.PINHOLE, False, 1.3, 1),
    ((rr.ROWS, rr.COLS), SMALL, sr.PINHOLE, False, 1.0, 3), ((rr.ROWS, rr.COLS), SMALL, sr.PINHOLE, True, 1.3, 3),
    (ODD, (64, 48), sr.PINHOLE, True, 1.0, 3), (ODD, (64, 48), sr.PINHOLE, False, 1.3, 1),
]


@pytest.mark.parametrize("size,out,camera,explicit,zoom,iterations", MAP_CASES)
def test_map_against_the_float64_reference(scene, size, out, camera, explicit, zoom, iterations):
    """the tolerance is four times the float32 restatement's distance from the float64 one for that camera at 380 x 676:
    the rectifier's rule (rr.device_tolerance), from the reference alone"""
    from rssync_amd import synth
    (rows, cols), (orows, ocols) = size, out
    p, g, t = scene["problem"], scene["gyro"], scene["times"][1]
    lens = rr.scaled_lens(rows, cols)
    # an explicit target: another smoothing's orientation, not of unit length (the library normalises it)
    target = 2.5 * sr.path64(g, np.array([t]), lens[0], synth.D_TRUE, 0.3)[0] if explicit else None
    kw = dict(target=target, sigma=sr.SIGMA, out_size=(ocols, orows), zoom=zoom, camera=camera, iterations=iterations)
    got = p.stabilize_map(cols, rows, lens, t, synth.D_TRUE, **kw)
    want = sr.map64(g, lens, rows, cols, t, synth.D_TRUE, **kw)
    assert got.shape == want.shape == (orows, ocols, 2) and got.dtype == np.float32
    diff, tol = np.abs(got.astype(np.float64) - want).max(), sr.device_tolerance(camera)
    print("%s -> %s camera %d explicit %s zoom %.1f iterations %d: %.3g px (tolerance %.3g)" % (size, out, camera, explicit, zoom,
                                                                                              iterations, diff, tol))
    assert diff <= tol


def test_an_output_camera_given_in_full_is_used(scene):
    from rssync_amd import synth
    p, g, lens, t = scene["problem"], scene["gyro"], scene["lens"], scene["times"][0]
    cam = (300.0, 310.0, 150.5, 99.0)
    kw = dict(sigma=sr.SIGMA, out_size=(320, 200), zoom=1.1, camera=sr.PINHOLE)
    got = p.stabilize_map(rr.COLS, rr.ROWS, lens, t, synth.D_TRUE, out_camera=cam, **kw)
    want = sr.map64(g, lens, rr.ROWS, rr.COLS, t, synth.D_TRUE, cam=cam, **kw)
    assert np.abs(got.astype(np.float64) - want).max() <= sr.device_tolerance(sr.PINHOLE)


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_sampler_is_the_float32_restatement_bit_for_bit(scene, stabilised):
    """from the device's own map rr.sample gives the device's bytes and counts; pitched input and output, the padding of
    the output untouched"""
    from rssync_amd import synth
    p, frames = scene["problem"], scene["frames"]
    out, n_out, maps = stabilised
    wide = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS + 45), np.uint8)
    wide[:, :, 7:7 + rr.COLS] = frames
    dst = np.full((rr.N_FRAMES, rr.ROWS + 3, rr.COLS + 21), 201, np.uint8)
    view = dst[:, 1:1 + rr.ROWS, 5:5 + rr.COLS]
    got, got_n = p.stabilize_frames(wide[:, :, 7:7 + rr.COLS], scene["times"], scene["lens"], synth.D_TRUE, sigma=sr.SIGMA, fill=77, out=view)
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


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_error_against_the_global_shutter_truth_at_the_path(scene, stabilised):
    out, n_out, maps = stabilised
    frames, truth, ref_maps = scene["frames"], sr.truth(), sr.reference_maps()
    for k in range(rr.N_FRAMES):
        ok = rr.inside(maps[k])
        err = rr.grey_error(out[k], truth[k], ok)
        raw = rr.grey_error(frames[k], truth[k], ok)
        ref_img, _ = rr.sample(frames[k], ref_maps[k])
        ref_ok = rr.inside(ref_maps[k])
        both = ok & ref_ok
        worst = np.abs(out[k].astype(int) - ref_img.astype(int))[both].max()
        flips = (ok != ref_ok).mean()
        print("frame %d: device %.4f reference %.4f raw %.1f; device against reference image: %d grey levels, %.2g of the inside "
              "flags differ" % (rr.F0 + k, err, sr.REFERENCE_ERROR[k], raw, worst, flips))
        assert err <= 1.05 * sr.REFERENCE_ERROR[k], (k, err)
        assert err <= rr.RATIO * raw, (k, err, raw)
        assert worst <= 1 and flips <= 1e-3, (k, worst, flips)


# 6 ---------------------------------------------------------------------------------------------------------------------
def _assert_identity(out, frames):
    np.testing.assert_array_equal(out[:, 1:-1, 1:-1], frames[:, 1:-1, 1:-1])


def test_a_camera_at_rest_is_the_identity(scene, built):
    """random noise: the worst case for interpolation"""
    from rssync_amd import synth
    g = scene["gyro"]
    quats = np.zeros_like(g.quats)
    quats[:, 0] = 1.0
    p = _problem()
    p.SetGyroQuaternions(quats, g.fs, g.t0)
    frames = _noise()
    assert scene["lens"][0] == synth.READOUT
    out, _ = p.stabilize_frames(frames, scene["times"][:2], scene["lens"], synth.D_TRUE, sigma=0.2)
    _assert_identity(out, frames)


def test_no_readout_time_at_the_frames_own_orientation_is_the_identity(scene):
    from rssync_amd import synth
    frames = _noise()
    lens = (0.0,) + tuple(scene["lens"][1:])
    targets = scene["gyro"].orientation(scene["times"][:2] + synth.D_TRUE)
    out, _ = scene["problem"].stabilize_frames(frames, scene["times"][:2], lens, synth.D_TRUE, targets=targets)
    _assert_identity(out, frames)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_host_device_and_pitched_buffers_agree(scene, stabilised):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    want, want_n, _ = stabilised
    wide = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS + 61), np.uint8)
    wide[:, :, 13:13 + rr.COLS] = frames
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")
    dwide = torch.from_numpy(wide).to("cuda:0")
    for src in (wide[:, :, 13:13 + rr.COLS], dev, dwide[:, :, 13:13 + rr.COLS]):
        got, n = p.stabilize_frames(src, times, lens, synth.D_TRUE, sigma=sr.SIGMA)
        assert isinstance(got, torch.Tensor) == isinstance(src, torch.Tensor)
        np.testing.assert_array_equal(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
        np.testing.assert_array_equal(n, want_n)
    # device frames into a host array, host frames into a pitched device tensor
    host_out = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS), np.uint8)
    p.stabilize_frames(dev, times, lens, synth.D_TRUE, sigma=sr.SIGMA, out=host_out)
    np.testing.assert_array_equal(host_out, want)
    dout = torch.full((rr.N_FRAMES, rr.ROWS, rr.COLS + 19), 9, dtype=torch.uint8, device="cuda:0")
    p.stabilize_frames(frames, times, lens, synth.D_TRUE, sigma=sr.SIGMA, out=dout[:, :, 3:3 + rr.COLS])
    back = dout.cpu().numpy()
    np.testing.assert_array_equal(back[:, :, 3:3 + rr.COLS], want)
    assert (back[:, :, :3] == 9).all() and (back[:, :, 3 + rr.COLS:] == 9).all()


def test_frames_in_one_call_equal_frames_one_at_a_time(scene, stabilised):
    from rssync_amd import synth
    want, want_n, _ = stabilised
    for k in range(rr.N_FRAMES):
        got, n = scene["problem"].stabilize_frames(scene["frames"][k:k + 1], scene["times"][k:k + 1], scene["lens"], synth.D_TRUE,
                                                   sigma=sr.SIGMA)
        np.testing.assert_array_equal(got[0], want[k])
        assert n[0] == want_n[k]


def test_chunk_boundaries_and_another_output_size_do_not_change_the_result(scene):
    """a budget of one and a half frames per slot: the three frames go as three chunks through both slots, into a
    200 x 320 output; the result is the one call's, and the restated sampler's from the device's map"""
    from rssync_amd import stabilize, synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    orows, ocols = 200, 320
    one, one_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, sigma=sr.SIGMA, out_size=(ocols, orows), fill=5)
    assert one.shape == (rr.N_FRAMES, orows, ocols)
    per_frame = (rr.ROWS + 1) * 36 + rr.ROWS * rr.COLS + orows * ocols
    got, got_n = stabilize.stabilize_frames_budget(p, frames, times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, out_size=(ocols, orows),
                                                   sigma=sr.SIGMA, fill=5)
    np.testing.assert_array_equal(got, one)
    np.testing.assert_array_equal(got_n, one_n)
    dev, dev_n = p.stabilize_frames(torch.from_numpy(np.array(frames)).to("cuda:0"), times, lens, synth.D_TRUE, sigma=sr.SIGMA,
                                    out_size=(ocols, orows), fill=5)
    np.testing.assert_array_equal(dev.cpu().numpy(), one)
    np.testing.assert_array_equal(dev_n, one_n)
    for k in range(rr.N_FRAMES):
        m = p.stabilize_map(rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, sigma=sr.SIGMA, out_size=(ocols, orows))
        want, want_n = sr.sample(frames[k], m, fill=5)
        np.testing.assert_array_equal(one[k], want, err_msg="frame %d" % k)
        assert int(one_n[k]) == want_n


def test_mixed_memory_kinds_across_chunks(scene, monkeypatch):
    """device frames into a host array and host frames into a device tensor, each with a budget of one and a half of the
    frames that then pass through a slot: three chunks through both slots.  Where the output lies in a slot depends on
    whether the input passes through it too; the result is the unchunked all-host call's."""
    from rssync_amd import stabilize, synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    orows, ocols = 200, 320
    kw = dict(out_size=(ocols, orows), sigma=sr.SIGMA, fill=5)
    one, one_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, **kw)
    tab, px_in, px_out = (rr.ROWS + 1) * 36, rr.ROWS * rr.COLS, orows * ocols
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")
    got, got_n = stabilize.stabilize_frames_budget(p, dev, times, lens, synth.D_TRUE, 2 * 1.5 * (tab + px_out), **kw)
    np.testing.assert_array_equal(got, one)
    np.testing.assert_array_equal(got_n, one_n)
    # the budget wrapper writes a host array: hand the launcher a device tensor in its place
    lib = stabilize.library()
    launcher = lib.rship_stabilize_frames
    dout = torch.zeros((rr.N_FRAMES, orows, ocols), dtype=torch.uint8, device="cuda:0")
    monkeypatch.setattr(lib, "rship_stabilize_frames", lambda *a: launcher(*a[:8], dout.data_ptr(), *a[9:]))
    _, got_n = stabilize.stabilize_frames_budget(p, frames, times, lens, synth.D_TRUE, 2 * 1.5 * (tab + px_in), **kw)
    np.testing.assert_array_equal(dout.cpu().numpy(), one)
    np.testing.assert_array_equal(got_n, one_n)


# 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 0.2])
def test_coverage_and_the_chosen_zoom(scene, sigma):
    """a device count may differ from the reference's by the border pixels whose source the reference puts within the
    map tolerance of a frame edge, and by no more"""
    from rssync_amd import synth
    p, g, lens, times = scene["problem"], scene["gyro"], scene["lens"], scene["times"]
    tol = sr.device_tolerance(sr.LENS)
    want, near = sr.coverage64(g, lens, rr.ROWS, rr.COLS, times, synth.D_TRUE, sr.ZOOMS, sigma=sigma, tol=tol)
    got = p.stabilize_coverage(rr.COLS, rr.ROWS, lens, times, synth.D_TRUE, sr.ZOOMS, sigma=sigma)
    print("sigma %.1f device" % sigma, got.tolist(), "reference", want.tolist(), "near an edge", near.tolist())
    assert got.shape == want.shape and got.dtype == np.uint32
    assert (np.abs(got.astype(np.int64) - want) <= near).all()
    zoom = p.stabilize_zoom(rr.COLS, rr.ROWS, lens, times, synth.D_TRUE, sr.ZOOMS, sigma=sigma)
    assert zoom == sr.first_clear(sr.ZOOMS, want) == pytest.approx(max(sr.FIRST_CLEAR_ZOOM[sigma]))
    _, n_clear = p.stabilize_frames(scene["frames"], times, lens, synth.D_TRUE, sigma=sigma, zoom=zoom)
    assert (n_clear == 0).all()
    _, n_below = p.stabilize_frames(scene["frames"], times, lens, synth.D_TRUE, sigma=sigma, zoom=sr.ZOOMS[sr.ZOOMS.index(zoom) - 1])
    assert (n_below > 0).any()
    assert p.stabilize_zoom(rr.COLS, rr.ROWS, lens, times, synth.D_TRUE, sr.ZOOMS[:2], sigma=sigma) is None


def test_coverage_with_a_pinhole_of_another_size_and_given_targets(scene):
    from rssync_amd import synth
    p, g, lens, times = scene["problem"], scene["gyro"], scene["lens"], scene["times"]
    targets = 0.5 * sr.path64(g, times, lens[0], synth.D_TRUE, 0.3)
    zooms = (0.6, 0.8, 1.0)     # (a pinhole of the lens's focal length sees less than the fisheye: wider ones reach past the frame)
    kw = dict(targets=targets, out_size=(197, 131), camera=sr.PINHOLE)
    want, near = sr.coverage64(g, lens, rr.ROWS, rr.COLS, times, synth.D_TRUE, zooms, tol=sr.device_tolerance(sr.PINHOLE), **kw)
    got = p.stabilize_coverage(rr.COLS, rr.ROWS, lens, times, synth.D_TRUE, zooms, **kw)
    print("device", got.tolist(), "reference", want.tolist(), "near an edge", near.tolist())
    assert want.max() > 0 and (np.abs(got.astype(np.int64) - want) <= near).all()


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene, stabilised):
    import rssync_amd
    from rssync_amd import stabilize, synth
    p, frames, times, lens = scene["problem"], np.ascontiguousarray(scene["frames"]), scene["times"], scene["lens"]
    want = stabilised[0]
    lib = stabilize.library()
    lib.rssync_set_panic_mode(1)
    L = np.ascontiguousarray(lens, np.float64)
    T = np.ascontiguousarray(times, np.float64)
    out = np.zeros_like(frames)
    W, H, N = rr.COLS, rr.ROWS, rr.N_FRAMES
    PD = C.POINTER(C.c_double)
    SP = stabilize.StabilizeParams
    good = dict(sigma=sr.SIGMA, zoom=0.0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, camera=0, iterations=0, fill=0)

    def prm_with(**kw):
        return SP(**dict(good, **kw))

    def call(h=p._h, f=frames.ctypes.data, n=N, w=W, hh=H, pitch=W, stride=W * H, t=T, lens_=L, delay=synth.D_TRUE, targets=None,
             prm=None, o=None, ow=W, oh=H, opitch=W, ostride=W * H):
        o = out.ctypes.data if o is None else o
        prm = prm_with() if prm is None else prm
        return lib.rssync_stabilize_frames(h, f, n, w, hh, pitch, stride, t.ctypes.data_as(PD) if t is not None else None,
                                           lens_.ctypes.data if lens_ is not None else None, delay,
                                           targets.ctypes.data_as(PD) if targets is not None else None, C.byref(prm), o if o else None,
                                           ow, oh, opitch, ostride, None)

    def bad(match, **kw):
        assert call(**kw) != 0, match
        msg = lib.rssync_last_error().decode()
        assert match in msg, (match, msg)

    def lens_with(i, v):
        m = L.copy()
        m[i] = v
        return m

    def targets_with(v):
        q = np.tile([1.0, 0.0, 0.0, 0.0], (N, 1))
        q[1] = v
        return q

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
    bad("too small", ow=1)
    bad("too small", oh=1)
    bad("non-finite frame time", t=np.array([times[0], np.nan, times[2]]))
    bad("non-finite delay", delay=float("inf"))
    bad("negative readout", lens_=lens_with(0, -1e-3))
    bad("non-finite lens", lens_=lens_with(2, np.nan))
    bad("sigma", prm=prm_with(sigma=-0.1))
    bad("sigma", prm=prm_with(sigma=float("nan")))
    bad("sigma", prm=prm_with(sigma=float("inf")))
    bad("zoom", prm=prm_with(zoom=-1.0))
    bad("zoom", prm=prm_with(zoom=float("inf")))
    bad("zoom", prm=prm_with(zoom=float("nan")))
    bad("target 1", targets=targets_with(0.0))
    bad("target 1", targets=targets_with([1.0, np.nan, 0.0, 0.0]))
    bad("target 1", targets=targets_with([np.inf, 0.0, 0.0, 0.0]))
    bad("given together", prm=prm_with(fx=300.0))
    bad("given together", prm=prm_with(fx=300.0, fy=300.0, cx=10.0))
    bad("camera", prm=prm_with(camera=2))
    bad("camera", prm=prm_with(camera=-1))
    bad("iterations", prm=prm_with(iterations=9))
    bad("iterations", prm=prm_with(iterations=-1))
    bad("fill", prm=prm_with(fill=256))
    bad("fill", prm=prm_with(fill=-1))
    bad("overlaps", o=frames.ctypes.data + W * H)
    if torch.cuda.device_count() > 1:
        other = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        bad("memory of device", o=other.data_ptr())
        bad("memory of device", f=other.data_ptr())
    # ... and the calls that follow work: the defaults spelled out are the same thing
    for prm in (prm_with(), prm_with(zoom=1.0, iterations=3)):
        out[:] = 0
        assert call(prm=prm) == 0, lib.rssync_last_error().decode()
        np.testing.assert_array_equal(out, want)
    # the other three entry points
    m = np.zeros((H, W, 2), np.float32)
    q = np.zeros((N, 4))
    cov = np.zeros((N, 2), np.uint32)
    PU = C.POINTER(C.c_uint32)

    def zs(*v):
        return np.array(v, np.float64).ctypes.data_as(PD)

    def coverage(h=p._h, t=T.ctypes.data_as(PD), delay=synth.D_TRUE, prm=None, z=zs(1.0, 1.1), o=cov.ctypes.data_as(PU)):
        return lib.rssync_stabilize_coverage(h, W, H, L.ctypes.data, W, H, t, N, delay, None, C.byref(prm_with() if prm is None else prm),
                                             z, 2, o)

    assert lib.rssync_stabilize_map(p._h, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, None, None, None) != 0
    assert lib.rssync_stabilize_map(p._h, W, H, L.ctypes.data, W, H, float(times[0]), 9.0, None, None, m.ctypes.data) != 0
    assert "leaves the gyro data" in lib.rssync_last_error().decode()
    assert lib.rssync_stabilize_map(p._h, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, zs(0, 0, 0, 0), None, m.ctypes.data) != 0
    assert lib.rssync_stabilize_map(empty._h, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, None, None, m.ctypes.data) != 0
    assert lib.rssync_stabilize_path(p._h, T.ctypes.data_as(PD), N, lens[0], synth.D_TRUE, -1.0, q.ctypes.data) != 0
    assert "sigma" in lib.rssync_last_error().decode()
    assert lib.rssync_stabilize_path(p._h, T.ctypes.data_as(PD), N, lens[0], synth.D_TRUE, float("nan"), q.ctypes.data) != 0
    assert lib.rssync_stabilize_path(p._h, None, N, lens[0], synth.D_TRUE, 0.1, q.ctypes.data) != 0
    assert lib.rssync_stabilize_path(p._h, T.ctypes.data_as(PD), N, lens[0], synth.D_TRUE, 0.1, None) != 0
    assert lib.rssync_stabilize_path(p._h, T.ctypes.data_as(PD), N, lens[0], 9.0, 0.1, q.ctypes.data) != 0
    assert "leaves the gyro data" in lib.rssync_last_error().decode()
    assert lib.rssync_stabilize_path(empty._h, T.ctypes.data_as(PD), N, lens[0], synth.D_TRUE, 0.1, q.ctypes.data) != 0
    assert "no gyro data" in lib.rssync_last_error().decode()
    for kw in (dict(z=zs(1.0, 0.0)), dict(z=zs(-1.0, 1.0)), dict(z=zs(1.0, np.nan)), dict(z=zs(np.inf, 1.0)), dict(z=None), dict(o=None),
               dict(t=None), dict(delay=9.0), dict(h=empty._h), dict(prm=prm_with(sigma=-1.0)), dict(prm=prm_with(camera=5))):
        assert coverage(**kw) != 0, kw
    assert coverage() == 0, lib.rssync_last_error().decode()
    assert coverage(prm=prm_with(zoom=-7.0)) == 0        # (the sweep replaces params->zoom: it is not read)
    with pytest.raises(rssync_amd.RsSyncError, match="sigma"):
        p.stabilize_map(W, H, lens, times[0], synth.D_TRUE, sigma=-1.0)
    np.testing.assert_array_equal(p.stabilize_map(W, H, lens, times[0], synth.D_TRUE, sigma=sr.SIGMA), stabilised[2][0])
    np.testing.assert_array_equal(p.stabilize_path(times, lens[0], synth.D_TRUE, 0.1), p.stabilize_path(times, lens[0], synth.D_TRUE, 0.1))
