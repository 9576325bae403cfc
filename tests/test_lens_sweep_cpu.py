"""The lens sweep (rssync_ext_lens_sweep, rssync_ext_set_lens, rssync_amd.lens.estimate_lens) on the host solver linked
against the CPU test double of the device ABI.  The double has no re-lens launcher, so every lens goes the plain way there
-- the frames repacked with the new lens, then PreSync -- and these tests pin the host's part: the frame records it
computes for a lens (the same as set_track_pixels with it), the arg-min rule, the restore afterwards, the errors, and the
coordinate search built on the sweep.  The device's pipelined route is compared with the same loop in
tests/test_gpu_lens_sweep.py."""
import numpy as np
import pytest

SEED = 321
ARGS = (0.0, 0, 8, 0.004, 0.06)


def _scene():
    """the readout sweep tests' scene: pixel frames of two size classes (64 and 600 tracks) and one frame set as rays,
    outside the swept range"""
    from rssync_amd import synth
    gyro = synth.make_gyro(0.0, 14 / synth.FPS, seed=5)
    frames = [next(iter(synth.make_pixel_frames(gyro, fr, fr + 1, 64 if fr < 6 else 600, seed=5))) for fr in range(8)]
    rays = next(iter(synth.make_frames(gyro, 9, 10, 50, seed=5)))
    return gyro, frames, rays


def _lenses():
    """eight lenses around synth.LENS: fx and fy, k1, cx and ro moved, alone and together; the installed one is number 3"""
    from rssync_amd import synth
    ro, fx, fy, cx, cy, k1, k2, k3, k4 = synth.LENS
    return np.array([
        (ro, 0.85 * fx, 0.85 * fy, cx, cy, k1, k2, k3, k4),
        (ro, 1.1 * fx, 1.1 * fy, cx, cy, k1, k2, k3, k4),
        (ro, fx, fy, cx, cy, k1 - 0.08, k2, k3, k4),
        synth.LENS,
        (ro, fx, fy, cx, cy, k1 + 0.06, k2, k3, k4),
        (ro, fx, fy, cx + 70.0, cy, k1, k2, k3, k4),
        (0.007, fx, fy, cx, cy, k1, k2, k3, k4),
        (0.015, 0.95 * fx, 1.02 * fy, cx - 40.0, cy, 0.0, 0.0, 0.0, 0.0),
    ])


def _feed(p, gyro, frames, rays, lens):
    from rssync_amd import synth
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr, ta, tb, pa, pb in frames:
        p.set_track_pixels(fr, ta, tb, pa, pb, lens, synth.IMAGE_ROWS)
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


def test_sweep_equals_the_reset_loop(hosttest_lib):
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    lenses = _lenses()
    loop = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    want = []
    for lens in lenses:
        for fr, ta, tb, pa, pb in frames:
            loop.set_track_pixels(fr, ta, tb, pa, pb, lens, synth.IMAGE_ROWS)
        want.append(loop.PreSync(*ARGS))
    swp = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    costs, delays = swp.lens_sweep(lenses, *ARGS)
    for i in range(len(lenses)):
        assert (costs[i], delays[i]) == want[i], i
    assert len(set(costs.tolist())) == len(lenses)         # every lens changes the problem
    # (the installed lens: as PreSync on the frames as they were set)
    assert (costs[3], delays[3]) == _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS).PreSync(*ARGS)


def test_set_lens_is_setting_the_frames_again(hosttest_lib):
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    ids = [f[0] for f in frames] + [rays[0]]
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    p.PreSync(*ARGS)                                     # packed with the installed lens first
    for lens in _lenses()[[0, 4, 7]]:
        p.set_lens(lens)
        q = _feed(_problem(hosttest_lib), gyro, frames, rays, lens)
        _same_rays(_rays(p, ids), _rays(q, ids))
        assert p.PreSync(*ARGS) == q.PreSync(*ARGS)
    # the rays frame was not touched, the directions of the pixel frames were
    ref = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    _same_rays(_rays(p, ids[-1:]), _rays(ref, ids[-1:]))
    assert not np.array_equal(_rays(p, ids[:1])[0][0], _rays(ref, ids[:1])[0][0])


def test_frames_keep_their_own_lens_after_a_sweep(hosttest_lib):
    """each frame its own lens, frames with different lenses included"""
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    ids = [f[0] for f in frames] + [rays[0]]
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    for i, lens in ((2, _lenses()[7]), (6, _lenses()[1])):
        fr, ta, tb, pa, pb = frames[i]
        p.set_track_pixels(fr, ta, tb, pa, pb, lens, synth.IMAGE_ROWS)
    before_rays, before = _rays(p, ids), p.PreSync(*ARGS)
    p.lens_sweep(_lenses(), *ARGS)
    _same_rays(_rays(p, ids), before_rays)
    assert p.PreSync(*ARGS) == before


def test_lenses_that_differ_in_ro_give_the_readout_sweep(hosttest_lib):
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    readouts = [0.004, 0.007, 0.0095, 0.0105, 0.01111, 0.012, 0.015, 0.02]
    a = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    b = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    want_c, want_d = a.readout_sweep(readouts, *ARGS)
    costs, delays = b.lens_sweep([(ro,) + tuple(synth.LENS[1:]) for ro in readouts], *ARGS)
    np.testing.assert_array_equal(costs.view(np.uint64), want_c.view(np.uint64))
    np.testing.assert_array_equal(delays.view(np.uint64), want_d.view(np.uint64))


def test_errors(hosttest_lib):
    import rssync_amd
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    ids = [f[0] for f in frames] + [rays[0]]
    good = np.array(synth.LENS)
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    before_rays = _rays(p, ids)
    with pytest.raises(rssync_amd.RsSyncError, match="frame 9 was set as rays"):
        p.lens_sweep(_lenses(), 0.0, 0, 10, 0.004, 0.06)           # frame 9 was set by SetTrackResult
    for pos, value, what in ((0, -1e-3, "readout"), (1, 0.0, "focal"), (2, -1180.0, "focal"), (5, float("nan"), "non-finite"),
                             (3, float("inf"), "non-finite")):
        bad = good.copy()
        bad[pos] = value
        with pytest.raises(rssync_amd.RsSyncError, match="lens sweep: lens 1 .*" + what):
            p.lens_sweep([good, bad], *ARGS)
        with pytest.raises(rssync_amd.RsSyncError, match="set-lens: .*" + what):
            p.set_lens(bad)
    with pytest.raises(rssync_amd.RsSyncError, match="no lenses"):
        p.lens_sweep(np.zeros((0, 9)), *ARGS)
    with pytest.raises(ValueError):
        p.lens_sweep([good[:8]], *ARGS)
    # nothing of that changed the frames
    _same_rays(_rays(p, ids), before_rays)
    q = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    assert p.PreSync(*ARGS) == q.PreSync(*ARGS)


def test_a_lens_that_breaks_the_rays_fails_as_the_loop_does(hosttest_lib):
    """finite, positive, and still no lens: focal lengths so small that the normalised coordinates overflow"""
    import rssync_amd
    from rssync_amd import synth
    gyro, frames, rays = _scene()
    ids = [f[0] for f in frames] + [rays[0]]
    broken = np.array(synth.LENS)
    broken[1:3] = 1e-300
    loop = _feed(_problem(hosttest_lib), gyro, frames, rays, broken)
    with pytest.raises(rssync_amd.RsSyncError, match="non-finite numbers in rays"):
        loop.PreSync(*ARGS)
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, synth.LENS)
    before_rays, before = _rays(p, ids), p.PreSync(*ARGS)
    with pytest.raises(rssync_amd.RsSyncError, match="non-finite numbers in rays"):
        p.lens_sweep([synth.LENS, broken], *ARGS)
    _same_rays(_rays(p, ids), before_rays)                 # every frame restored
    assert p.PreSync(*ARGS) == before


# ---- the coordinate search -------------------------------------------------------------------------------------------

EST_ARGS = (0.0, 0, 40, 0.002, 0.06)


def _written_out(p, frames, lens):
    """estimate_lens(params=("f", "k1")) with its defaults, spelled with the calls that existed before the sweep: nine
    candidates per parameter and pass through set_track_pixels + PreSync, the move to the vertex of the parabola through
    the arg-min and its neighbours (clamped to them; none on the grid's edge or where the points do not open upwards),
    spans 0.25 and 0.15 shrinking by 0.4, three passes"""
    from rssync_amd import synth

    def presync(lens):
        for fr, ta, tb, pa, pb in frames:
            p.set_track_pixels(fr, ta, tb, pa, pb, lens, synth.IMAGE_ROWS)
        return p.PreSync(*EST_ARGS)

    def moved(lens, nm, off):
        out = np.array(lens, np.float64)
        if nm == "f":
            out[1:3] *= 1.0 + off
        else:
            out[5] += off
        return out

    lens, edges = np.array(lens, np.float64), {}
    for rnd in range(3):
        for nm, span in (("f", 0.25), ("k1", 0.15)):
            grid = np.linspace(-span * 0.4 ** rnd, span * 0.4 ** rnd, 9)
            res = [presync(moved(lens, nm, g)) for g in grid]
            k = min(range(9), key=lambda i: res[i])
            step = grid[k]
            if 0 < k < 8:
                (x0, x1, x2), (y0, y1, y2) = grid[k - 1:k + 2], [r[0] for r in res[k - 1:k + 2]]
                d01, d12 = (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1)
                curv = (d12 - d01) / (x2 - x0)
                if curv > 0:
                    step = min(max(0.5 * (x0 + x1) - d01 / (2.0 * curv), x0), x2)
            edges[nm] = k in (0, 8)
            lens = moved(lens, nm, step)
    return lens, presync(lens), edges


def test_estimate_lens_recovers_the_focal_length(hosttest_lib):
    """40 frames x 200 tracks, seed 1, 0.3 px noise, 10 % outliers; from fx, fy 15 % low and k1 .. k4 = 0.  Measured
    through the written-out loop on this CPU route: fx ends at 1184.1 against 1180 (0.35 % off; the final grid step is
    1 %), k1 at 0.0533 against 0.05 (it absorbs the zeroed higher terms), the cost at 274.47 (the true lens: 274.54)."""
    from rssync_amd import synth
    from rssync_amd.lens import estimate_lens
    gyro = synth.make_gyro(0.0, 46 / synth.FPS, seed=1)
    frames = list(synth.make_pixel_frames(gyro, 0, 40, 200, seed=1))
    start = np.array(synth.LENS)
    start[1:3] *= 0.85
    start[5:] = 0.0

    def fed():
        p = _problem(hosttest_lib)
        p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
        for fr, ta, tb, pa, pb in frames:
            p.set_track_pixels(fr, ta, tb, pa, pb, start, synth.IMAGE_ROWS)
        return p

    p = fed()
    est = estimate_lens(p, start, *EST_ARGS)
    want_lens, want_presync, want_edges = _written_out(fed(), frames, start)
    np.testing.assert_array_equal(est.lens.view(np.uint64), want_lens.view(np.uint64))
    assert (est.cost, est.delay) == want_presync
    print("fx %.2f (truth %.0f), k1 %.4f, cost %.3f, delay %.4f" % (est.lens[1], synth.LENS[1], est.lens[5], est.cost, est.delay))
    assert abs(est.lens[1] / synth.LENS[1] - 1.0) < 0.01
    assert est.lens[1] / est.lens[2] == start[1] / start[2]   # "f" scales fx and fy together
    assert est.unresolved == () and not any(want_edges.values())
    assert [(q.param, q.round) for q in est.passes] == [(nm, r) for r in range(3) for nm in ("f", "k1")]
    assert all(q.grid.size == 9 and q.costs.size == 9 for q in est.passes)
    # nothing was installed: the frames still hold the start lens
    assert p.PreSync(*EST_ARGS) == fed().PreSync(*EST_ARGS)
    p.set_lens(est.lens)
    assert p.PreSync(*EST_ARGS) == (est.cost, est.delay)


def test_estimate_lens_reports_what_the_grid_did_not_bracket(hosttest_lib):
    """a span too narrow to reach the minimum: the arg-min sits on the grid's edge in the last pass"""
    from rssync_amd import synth
    from rssync_amd.lens import estimate_lens
    gyro, frames, rays = _scene()
    start = np.array(synth.LENS)
    start[1:3] *= 0.8
    p = _feed(_problem(hosttest_lib), gyro, frames, rays, start)
    est = estimate_lens(p, start, *ARGS, params=("f",), spans={"f": 0.1}, points=3, rounds=1)
    print(est.passes[0].costs)
    assert est.unresolved == ("f",) and not est.passes[0].vertex_is_interior and est.passes[0].argmin == 2
    assert est.lens[1] == start[1] * (1.0 + 0.1)            # moved to the edge, no further
    with pytest.raises(ValueError):
        estimate_lens(p, start, *ARGS, params=("zoom",))
