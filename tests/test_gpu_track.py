"""The tracker on the device (include/rssync_track.h, csrc/kernels/track.hpp) against the numpy reference
(tests/track_reference.py) and the synthetic video's ground truth (rs-sync_amd/synth_video.py)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import track_reference as tr

pytestmark = pytest.mark.gpu

F0, N_FRAMES, STEP, SEED = 30, 41, 100, 77
ROWS, COLS = 760, 1352
# The same pipeline on the CPU -- this video, the numpy reference tracker, then the oracle's PreSync + Sync fed the driver's
# way (pixels_to_tracks + SetTrackResult, gyro integrated as core_testcode.cpp:36-52) -- lands 8.2e-4 s from D_TRUE
# (3636 of 3640 points status 0; their error against the ground truth: median 0.133 px, 99th percentile 1.16 px).
CPU_DELAY_ERROR = 8.2e-4
TRACK_MEDIAN_PX, TRACK_P99_PX = 0.133, 1.16


@pytest.fixture(scope="module")
def video():
    from rssync_amd import synth, synth_video as sv
    gyro = synth.make_gyro(1.0, 1.0 + (N_FRAMES + 2) / synth.FPS, seed=SEED)   # t0 = 0: rate timestamps must be >= 0
    lens = sv.half_lens()
    frames, times = sv.render(gyro, F0, F0 + N_FRAMES, lens=lens, rows=ROWS, cols=COLS, seed=SEED)
    return gyro, lens, frames, times


def _problem():
    import rssync_amd
    return rssync_amd.SyncProblem(seed=321)


def test_pyramid_is_the_numpy_restatement_bit_for_bit(built):
    from rssync_amd import track
    rng = np.random.default_rng(3)
    p = _problem()
    for h, w in ((197, 331), (29, 37), (120, 64)):
        wide = rng.integers(0, 256, size=(3, h, w + 45), dtype=np.uint8)
        frames = wide[:, :, 7:7 + w]                                   # pitch > width
        for levels in (4, 3):
            got = track.pyramid(p, frames, levels)
            for k in range(frames.shape[0]):
                want = tr.pyramid(frames[k], levels)[1:]
                for lv, (g, wv) in enumerate(zip(got, want)):
                    assert g[k].shape == wv.shape
                    np.testing.assert_array_equal(g[k], wv, err_msg="%dx%d level %d" % (w, h, lv + 1))


def test_points_equal_the_reference(built, video):
    _, _, frames, _ = video
    p = _problem()
    pa, pb, st, res = p.track_points(frames[:9], grid_step=STEP)
    ra, rb, rst, rres = tr.track(frames[:9], step=STEP)
    np.testing.assert_array_equal(pa, ra)
    np.testing.assert_array_equal(st, rst)
    ok = st == 0
    assert ok.mean() > 0.95
    assert np.abs(pb - rb)[ok].max() <= 1e-3, np.abs(pb - rb)[ok].max()
    assert np.abs(res - rres)[ok].max() <= 1e-2


def test_error_against_the_ground_truth(built, video):
    from rssync_amd import synth_video as sv
    gyro, lens, frames, _ = video
    pa, pb, st, _ = _problem().track_points(frames, grid_step=STEP)
    truth = sv.true_points(gyro, F0, F0 + N_FRAMES, pa, lens=lens, rows=ROWS, seed=SEED)
    err = np.linalg.norm(pb - truth, axis=-1)[st == 0]
    assert (st == 0).mean() >= 0.99
    assert np.median(err) <= TRACK_MEDIAN_PX * 1.05 and np.percentile(err, 99) <= TRACK_P99_PX * 1.05, \
        (np.median(err), np.percentile(err, 99))


def test_track_frames_is_points_then_set_track_pixels(built, video):
    gyro, lens, frames, times = video
    a, b = _problem(), _problem()
    for p in (a, b):
        p.set_gyro_rates(gyro.times, gyro.rates)
    a.track_frames(frames[:8], times[:8], lens, first_frame=F0, grid_step=STEP)
    pa, pb, _, _ = b.track_points(frames[:8], grid_step=STEP)
    for k in range(7):
        b.set_track_pixels(F0 + k, times[k], times[k + 1], pa, pb[k], lens, ROWS)
    for k in range(7):
        ra, rb = a.frame_rays(F0 + k)
        sa, sb = b.frame_rays(F0 + k)
        assert ra.shape[0] == pa.shape[0]
        np.testing.assert_array_equal(ra, sa)
        np.testing.assert_array_equal(rb, sb)


def test_host_device_and_pitched_inputs_agree(built, video):
    _, _, frames, _ = video
    f = np.ascontiguousarray(frames[:5])
    p = _problem()
    want = p.track_points(f, grid_step=STEP)
    wide = np.zeros((5, ROWS, COLS + 61), np.uint8)
    wide[:, :, 13:13 + COLS] = f
    dev = torch.from_numpy(f).to("cuda:0")
    dwide = torch.from_numpy(wide).to("cuda:0")
    for src in (wide[:, :, 13:13 + COLS], dev, dwide[:, :, 13:13 + COLS]):
        got = p.track_points(src, grid_step=STEP)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_overlapping_batches_equal_one_call(built, video):
    _, _, frames, _ = video
    p = _problem()
    one = p.track_points(frames[:9], grid_step=STEP)
    first = p.track_points(frames[:5], grid_step=STEP)
    second = p.track_points(frames[4:9], grid_step=STEP)
    for k in (1, 2, 3):
        np.testing.assert_array_equal(one[k], np.concatenate([first[k], second[k]]))


def test_chunk_boundaries_do_not_change_the_result(built, video):
    """20 frames of 2704 x 1520 (9.5 MB each with their pyramid) exceed one chunk slot of the tracker's budget: the call is
    cut into chunks that share a frame.  The same pairs tracked in two calls that each fit one chunk agree bit for bit."""
    _, _, frames, _ = video
    big = np.repeat(np.repeat(frames[:20], 2, axis=1), 2, axis=2)
    assert big.shape == (20, 1520, 2704)
    p = _problem()
    one = p.track_points(big)
    a = p.track_points(big[:11])
    b = p.track_points(big[10:])
    assert one[1].shape == (19, 91, 2)
    for k in (1, 2, 3):
        np.testing.assert_array_equal(one[k], np.concatenate([a[k], b[k]]))
    assert (one[2] == 0).mean() > 0.9


def test_constant_frames_are_ill_conditioned(built):
    p = _problem()
    pa, pb, st, res = p.track_points(np.full((3, 300, 400), 77, np.uint8), grid_step=50)
    assert (st == 1).all() and np.isfinite(pb).all() and np.isfinite(res).all()
    np.testing.assert_array_equal(pb, np.broadcast_to(pa, pb.shape))


def test_points_carried_off_the_frame_leave_the_image(built, video):
    _, _, frames, _ = video
    f0 = frames[0, 200:540, 300:720]                       # 420 x 340 of the render
    f1 = np.empty_like(f0)
    f1[:, 60:] = f0[:, :-60]                                # content moves 60 px to the right
    f1[:, :60] = frames[1, 200:540, 100:160]
    pair = np.stack([f0, f1])
    pa, pb, st, _ = _problem().track_points(pair, grid_step=100)
    _, rb, rst, _ = tr.track(pair, step=100)
    gone = pa[:, 0] + 60 > 419                              # the true b is outside
    np.testing.assert_array_equal(st, rst)
    # LK is local: a point whose content left the frame can still lock onto something inside (clamped border), so
    # status 2 is asked of most of them.  A point may leave at a coarse level (that level's extent, scaled back: within
    # 2^3 px of level 0's border), so a status-2 point ends outside the image shrunk by 8 px
    assert gone.any() and (st[0][gone] == 2).mean() >= 0.5, st
    out = pb[0][st[0] == 2]
    assert ((out[:, 0] < 8) | (out[:, 0] > 411) | (out[:, 1] < 8) | (out[:, 1] > 331)).all(), out
    inside = ~gone & (st[0] == 0)
    assert inside.any() and np.abs(pb[0][inside] - pa[inside] - (60, 0)).max() < 0.05


def test_bad_arguments_raise(built, video):
    import rssync_amd
    from rssync_amd import track
    gyro, lens, frames, times = video
    p = _problem()
    f = frames[:3]
    with pytest.raises(rssync_amd.RsSyncError, match="at least 2 frames"):
        p.track_points(f[:1])
    with pytest.raises(rssync_amd.RsSyncError, match="grid step"):
        p.track_points(f, grid_step=-1)
    with pytest.raises(rssync_amd.RsSyncError, match="too small"):
        p.track_points(np.zeros((2, 12, 12), np.uint8), grid_step=5)     # levels 12, 6, 3, 2
    with pytest.raises(rssync_amd.RsSyncError, match="window"):
        p.track_points(f, window=22)
    with pytest.raises(rssync_amd.RsSyncError, match="non-finite frame time"):
        p.track_frames(f, [0.0, np.nan, 0.1], lens)
    lib = track.library()
    P = 18                                                      # 1352 x 760 at the default step 200: 6 x 3
    out = [np.zeros(2 * P), np.zeros(2 * 2 * P), np.zeros(2 * P, np.uint8), np.zeros(2 * P, np.float32)]
    args = [o.ctypes.data_as(t) for o, t in zip(out, (C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p,
                                                      C.POINTER(C.c_float)))]
    n = C.c_size_t()
    ptr = f.ctypes.data
    assert lib.rssync_track_points(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, None, *args, P, C.byref(n)) == 0
    assert n.value == P
    assert lib.rssync_track_points(p._h, ptr, 3, COLS, ROWS, COLS - 1, COLS * ROWS, None, *args, P, C.byref(n)) != 0
    assert "pitch" in lib.rssync_last_error().decode()
    assert lib.rssync_track_points(p._h, None, 3, COLS, ROWS, COLS, COLS * ROWS, None, *args, P, C.byref(n)) != 0
    assert lib.rssync_track_points(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, None, *args, P - 1, C.byref(n)) != 0
    assert n.value == P
    t = np.ascontiguousarray(times[:3])
    assert lib.rssync_track_frames(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, t.ctypes.data_as(C.POINTER(C.c_double)),
                                   0, None, None) != 0
    assert "lens" in lib.rssync_last_error().decode()


def test_frames_and_gyro_in_delay_out(built, video):
    """rates -> orientations, frames -> tracked pixels -> rays, PreSync + Sync: every step in the library, on the GPU"""
    from rssync_amd import synth
    gyro, lens, frames, times = video
    p = _problem()
    p.set_gyro_rates(gyro.times, gyro.rates)
    p.track_frames(frames, times, lens, first_frame=F0, grid_step=STEP)
    _, d = p.PreSync(0.0, F0, F0 + N_FRAMES - 1, 0.002, 0.1)
    _, d = p.Sync(d, F0, F0 + N_FRAMES - 2, 0.0, 0.2)
    assert abs(d - synth.D_TRUE) <= 2 * CPU_DELAY_ERROR, (d, synth.D_TRUE)
