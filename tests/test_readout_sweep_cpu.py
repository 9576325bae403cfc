"""The readout sweep (rssync_ext_readout_sweep, rssync_ext_set_readout) on the host solver linked against the CPU test
double of the device ABI.  The double has no re-timing launcher, so every readout goes the plain way there -- the frames
repacked with the new readout, then PreSync -- and these tests pin the host's part: the frame records it computes for a
readout (the same as set_track_pixels with that lens.ro), the arg-min rule, the restore afterwards and the errors.  The
device's pipelined route is compared with the same loop in tests/test_gpu_readout_sweep.py."""
import numpy as np
import pytest

SEED = 321
READOUTS = [0.004, 0.007, 0.0095, 0.0105, 0.01111, 0.012, 0.015, 0.02]   # straddle the installed synth.READOUT


def _scene():
    """pixel frames of two size classes (64 and 600 tracks) and one frame set as rays, outside the swept range"""
    from rssync_amd import synth
    gyro = synth.make_gyro(0.0, 14 / synth.FPS, seed=5)
    frames = [next(iter(synth.make_pixel_frames(gyro, fr, fr + 1, 64 if fr < 6 else 600, seed=5))) for fr in range(8)]
    rays = next(iter(synth.make_frames(gyro, 9, 10, 50, seed=5)))
    return gyro, frames, rays


def _lens(ro):
    from rssync_amd import synth
    return (ro,) + tuple(synth.LENS[1:])


def _feed(p, gyro, frames, rays, ro):
    from rssync_amd import synth
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr, ta, tb, pa, pb in frames:
        p.set_track_pixels(fr, ta, tb, pa, pb, _lens(ro), synth.IMAGE_ROWS)
    p.SetTrackResult(*rays)
    return p


def _rays(p, ids):
    return [p.frame_rays(fr, cap=4096) for fr in ids]


def _same_rays(x, y):
    for (a1, b1), (a2, b2) in zip(x, y):
        np.testing.assert_array_equal(a1.view(np.uint32), a2.view(np.uint32))
        np.testing.assert_array_equal(b1.view(np.uint32), b2.view(np.uint32))


def _problem(lib):
    import rssync_amd
    return rssync_amd.SyncProblem(seed=SEED, _lib=lib)


ARGS = (0.0, 0, 8, 0.004, 0.06)


def test_sweep_equals_the_reset_loop(hosttest_lib):
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    loop = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    want = []
    for ro in READOUTS:
        for fr, ta, tb, pa, pb in frames:
            loop.set_track_pixels(fr, ta, tb, pa, pb, _lens(ro), synth.IMAGE_ROWS)
        want.append(loop.PreSync(*ARGS))
    swp = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    costs, delays = swp.readout_sweep(READOUTS, *ARGS)
    for i in range(len(READOUTS)):
        assert (costs[i], delays[i]) == want[i], i
    assert len(set(costs.tolist())) == len(READOUTS)        # the readout changes the problem
    # (the installed readout: as PreSync on the frames as they were set)
    assert (costs[4], delays[4]) == _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT).PreSync(*ARGS)


def test_set_readout_is_setting_the_frames_again(hosttest_lib):
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    ids = [f[0] for f in frames] + [rays[0]]
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    p.PreSync(*ARGS)                                     # packed with the installed readout first
    for ro in (0.0, 0.017, 0.03):
        p.set_readout(ro)
        q = _feed(_problem(hosttest_lib), gyro, frames, rays, ro)
        _same_rays(_rays(p, ids), _rays(q, ids))
        assert p.PreSync(*ARGS) == q.PreSync(*ARGS)
    # the rays frame was not touched, the times of the pixel frames were
    ref = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    _same_rays(_rays(p, ids[-1:]), _rays(ref, ids[-1:]))
    assert not np.array_equal(_rays(p, ids[:1])[0][1], _rays(ref, ids[:1])[0][1])


def test_frames_keep_their_own_readout_after_a_sweep(hosttest_lib):
    """each frame its own readout, frames with different readouts included"""
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    ids = [f[0] for f in frames] + [rays[0]]
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    fr, ta, tb, pa, pb = frames[2]
    p.set_track_pixels(fr, ta, tb, pa, pb, _lens(0.006), synth.IMAGE_ROWS)
    before_rays, before = _rays(p, ids), p.PreSync(*ARGS)
    p.readout_sweep(READOUTS, *ARGS)
    _same_rays(_rays(p, ids), before_rays)
    assert p.PreSync(*ARGS) == before


def test_errors(hosttest_lib):
    import rssync_amd
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    with pytest.raises(rssync_amd.RsSyncError, match="set as rays"):
        p.readout_sweep(READOUTS, 0.0, 0, 10, 0.004, 0.06)          # frame 9 was set by SetTrackResult
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(rssync_amd.RsSyncError, match="readout"):
            p.readout_sweep([0.01, bad], *ARGS)
        with pytest.raises(rssync_amd.RsSyncError, match="readout"):
            p.set_readout(bad)
    with pytest.raises(rssync_amd.RsSyncError, match="no readouts"):
        p.readout_sweep([], *ARGS)
    # nothing of that changed the frames
    q = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    assert p.PreSync(*ARGS) == q.PreSync(*ARGS)


def test_estimate_readout_helper(hosttest_lib):
    from rssync_amd import synth
    from rssync_amd.readout import estimate_readout
    gyro, frames, rays = _scene()
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.READOUT)
    grid = np.arange(0.004, 0.0201, 0.002)
    est = estimate_readout(p, grid, *ARGS)
    costs, delays = p.readout_sweep(grid, *ARGS)
    k = min(range(grid.size), key=lambda i: (costs[i], delays[i]))
    assert est.readout == grid[k] and est.delay == delays[k] and est.cost == costs[k]
    np.testing.assert_array_equal(est.costs, costs)
    if 0 < k < grid.size - 1:
        assert est.vertex_is_interior and grid[k - 1] <= est.vertex <= grid[k + 1]
    else:
        assert not est.vertex_is_interior and est.vertex == grid[k]
