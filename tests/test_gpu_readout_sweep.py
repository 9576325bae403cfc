"""The readout sweep on the device (rssync_ext_readout_sweep, rssync_ext_set_readout; csrc/kernels/support.hpp:
retime_pixels_kernel): the same bits on every route, the re-timing kernel against a full repack, the oracle per candidate,
recovery of the readout a scene was made with, end to end from rendered video, and across ranks and devices."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

pytestmark = pytest.mark.gpu

SEED = 321
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lens(ro, lens=None):
    from rssync_amd import synth
    return (ro,) + tuple((lens or synth.LENS)[1:])


def _pixel_scene(sizes, fs=400.0, seed=3, **kw):
    from rssync_amd import synth
    F = len(sizes)
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, fs=fs, seed=seed)
    frames = [next(iter(synth.make_pixel_frames(gyro, fr, fr + 1, n, seed=seed, **kw))) for fr, n in enumerate(sizes)]
    return gyro, frames


def _feed(p, gyro, frames, ro):
    from rssync_amd import synth
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr, ta, tb, pa, pb in frames:
        p.set_track_pixels(fr, ta, tb, pa, pb, _lens(ro), synth.IMAGE_ROWS)
    return p


def _problem(**kw):
    import rssync_amd
    return rssync_amd.SyncProblem(seed=SEED, **kw)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _rays(p, ids):
    return [p.frame_rays(fr, cap=4096) for fr in ids]


def _same_rays(x, y):
    for (a1, b1), (a2, b2) in zip(x, y):
        np.testing.assert_array_equal(a1.view(np.uint32), a2.view(np.uint32))
        np.testing.assert_array_equal(b1.view(np.uint32), b2.view(np.uint32))


# three size classes (the one-wave kernels, four waves of 4 and of 16 rows), a 2 kHz gyro: a pair spans ~67 knots at
# readout 0 and ~127 at 30 ms, so the sweeps' spline windows move from the compiled-in 80 knots to dynamic LDS
SIZES = [64] * 6 + [600] * 3 + [3000] * 2
READOUTS = np.arange(0.0, 0.03001, 0.0025)
ARGS = (0.0, 0, len(SIZES), 0.004, 0.06)


@pytest.fixture(scope="module")
def classes_scene():
    return _pixel_scene(SIZES, fs=2000.0)


def test_every_route_gives_the_same_bits(built, classes_scene):
    gyro, frames = classes_scene
    want_c, want_d, dyn = [], [], []
    loop = _feed(_problem(), gyro, frames, 0.0)       # the plain loop: every frame set again, then PreSync
    for ro in READOUTS:
        _feed(loop, gyro, frames, ro)
        c, d = loop.PreSync(*ARGS)
        want_c.append(c)
        want_d.append(d)
        dyn.append(loop.window_info()["presync_window_dynamic"])
    assert not dyn[0] and dyn[-1], dyn                 # the plan moves to dynamic LDS windows inside the sweep
    calls = _feed(_problem(), gyro, frames, 0.0)      # per-candidate calls: set_readout (the re-timing kernel), PreSync
    got = [calls.PreSync(*ARGS)]
    for ro in READOUTS:
        calls.set_readout(ro)
        got.append(calls.PreSync(*ARGS))
    assert got[1] == got[0]
    np.testing.assert_array_equal(_bits([g[0] for g in got[1:]]), _bits(want_c))
    np.testing.assert_array_equal(_bits([g[1] for g in got[1:]]), _bits(want_d))
    swp = _feed(_problem(), gyro, frames, 0.0)
    c1, d1 = swp.readout_sweep(READOUTS, *ARGS)       # the pipeline
    os.environ["RSSYNC_SWEEP_PIPELINE"] = "0"
    try:
        c0, d0 = swp.readout_sweep(READOUTS, *ARGS)   # one readout after the other
    finally:
        del os.environ["RSSYNC_SWEEP_PIPELINE"]
    for c, d in ((c1, d1), (c0, d0)):
        np.testing.assert_array_equal(_bits(c), _bits(want_c))
        np.testing.assert_array_equal(_bits(d), _bits(want_d))


def test_retimed_streams_equal_a_repack(built, classes_scene):
    from rssync_amd import synth
    gyro, frames = classes_scene
    ids = [f[0] for f in frames]
    p = _feed(_problem(), gyro, frames, synth.READOUT)
    base_rays, base = _rays(p, ids), p.PreSync(*ARGS)
    for ro in (0.0, 0.02, 0.03):
        p.set_readout(ro)
        q = _feed(_problem(), gyro, frames, ro)
        _same_rays(_rays(p, ids), _rays(q, ids))
        assert p.PreSync(*ARGS) == q.PreSync(*ARGS)
    p.set_readout(synth.READOUT)
    _same_rays(_rays(p, ids), base_rays)
    # after a sweep each frame holds its own readout: streams, PreSync and Sync as before
    s = _feed(_problem(max_outer_iters=30), gyro, frames, synth.READOUT)
    r = _feed(_problem(max_outer_iters=30), gyro, frames, synth.READOUT)
    s.readout_sweep(READOUTS, *ARGS)
    _same_rays(_rays(s, ids), base_rays)
    assert s.PreSync(*ARGS) == base
    assert s.Sync(base[1], 0, len(SIZES) - 1, 0.0, 0.2) == r.Sync(base[1], 0, len(SIZES) - 1, 0.0, 0.2)


def test_each_candidate_matches_the_oracle_presync(built):
    """clean scene; the oracle gets the rays the reference driver would make with each candidate readout"""
    from oracle import oracle
    from oracle.oracle import OracleProblem
    from rssync_amd import synth
    gyro, frames = _pixel_scene([128] * 16, seed=4, noise_px=0.0, outliers=0.0)
    readouts = [0.0, 0.006, synth.READOUT, 0.016, 0.025]
    args = (0.0, 0, 16, 0.002, 0.1)
    costs, delays = _feed(_problem(), gyro, frames, 0.0).readout_sweep(readouts, *args)
    for i, ro in enumerate(readouts):
        o = OracleProblem(seed=SEED, threads=os.cpu_count() or 1, faithful=False)
        o.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
        for fr, ta, tb, pa, pb in frames:
            o.SetTrackResult(fr, *oracle.pixels_to_tracks(_lens(ro), ta, tb, synth.IMAGE_ROWS, pa, pb))
        co, do = o.PreSync(*args)
        assert delays[i] == do, (ro, delays[i], do)
        assert abs(costs[i] - co) <= 5e-3 * abs(co), (ro, costs[i], co)   # the noise-free tolerance of smoke()
    assert int(np.argmin(costs)) == 2


def _recovery_scene():
    from rssync_amd import synth
    F = 120
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=1)
    return gyro, list(synth.make_pixel_frames(gyro, 0, F, 256, seed=1))


def _delay_after_sync(p, F):
    _, d = p.PreSync(0.0, 0, F, 0.0005, 0.1)
    for _ in range(4):
        _, d = p.Sync(d, 0, F - 1, 0.0, 0.2)
    return d


def test_the_sweep_recovers_the_readout_and_with_it_the_delay(built):
    """the oracle probe of the readout issue (120 frames x 256 tracks, seed 1, true readout 11.11 ms, 0.3 px noise, 10 %
    outliers) installed with readout 0: the arg-min lies within 1 ms of the truth, and with it installed PreSync + 4 x Sync
    land within 1 ms of the true delay, where readout 0 leaves them at least 3 ms off.  Measured on the MI355X: arg-min
    12.0 ms (the oracle's fp64 sweep: 11.5), parabola vertex 11.93 ms; delay 36.70 ms with it, 44.22 ms with readout 0."""
    from rssync_amd import synth
    from rssync_amd.readout import estimate_readout
    gyro, frames = _recovery_scene()
    F = len(frames)
    p = _feed(_problem(), gyro, frames, 0.0)
    est = estimate_readout(p, np.arange(0.0, 0.02501, 0.0005), 0.0, 0, F, 0.0005, 0.1)
    print("readout arg-min %.4f s (vertex %.5f), presync delay %.4f s" % (est.readout, est.vertex, est.delay))
    assert abs(est.readout - synth.READOUT) <= 1e-3
    assert abs(est.vertex - synth.READOUT) <= 1e-3
    zero = _delay_after_sync(_feed(_problem(), gyro, frames, 0.0), F)
    p.set_readout(est.readout)
    d = _delay_after_sync(p, F)
    print("delay after PreSync + 4 x Sync: %.6f s with the estimate, %.6f s with readout 0 (truth %.4f)" % (d, zero, synth.D_TRUE))
    assert abs(d - synth.D_TRUE) <= 1e-3
    assert abs(zero - synth.D_TRUE) >= 3e-3


# measured on the MI355X: the features of the rendered clip (true readout 11.11 ms) put the arg-min of a 1 ms grid at
# 12.0 ms, 0.89 ms off; the bound leaves one grid step beyond that
VIDEO_READOUT_TOL = 2e-3


def test_end_to_end_from_rendered_video(built):
    from rssync_amd import synth, synth_video as sv
    F0, n, rows, cols = 30, 41, 760, 1352
    gyro = synth.make_gyro(1.0, 1.0 + (n + 2) / synth.FPS, seed=77)
    lens = sv.half_lens()
    frames, times = sv.render(gyro, F0, F0 + n, lens=lens, rows=rows, cols=cols, seed=77)[:2]
    p = _problem()
    p.set_gyro_rates(gyro.times, gyro.rates)
    assert p.features_frames(frames, times, _lens(0.0, lens), first_frame=F0) == n - 1
    grid = np.arange(0.0, 0.02501, 0.001)
    costs, delays = p.readout_sweep(grid, 0.0, F0, F0 + n - 1, 0.002, 0.1)
    k = min(range(grid.size), key=lambda i: (costs[i], delays[i]))
    print("rendered clip: readout arg-min %.4f s (truth %.5f), presync delay %.4f" % (grid[k], lens[0], delays[k]))
    assert abs(grid[k] - lens[0]) <= VIDEO_READOUT_TOL


def test_two_contexts_in_one_object_give_the_same_bits(built):
    """frames spread over two contexts (cut at 64 frames) on the box's device: every shard re-times its own frames"""
    gyro, frames = _pixel_scene([48] * 130, seed=8)
    args = (0.0, 0, 130, 0.004, 0.06)
    readouts = [0.0, 0.008, 0.012, 0.02]
    one = _feed(_problem(), gyro, frames, 0.0).readout_sweep(readouts, *args)
    p = _problem()
    p.set_devices([0, 0])
    many = _feed(p, gyro, frames, 0.0).readout_sweep(readouts, *args)
    for a, b in zip(one, many):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    q = _feed(_problem(), gyro, frames, 0.0)
    q.set_readout(0.012)
    assert q.PreSync(*args) == (one[0][2], one[1][2])


def test_two_ranks_one_exchange_per_sweep(built, tmp_path):
    """two gloo ranks on the box's device, each with half the frames: the same arg-mins as one process, and one exchange
    for the whole [readout][candidate] matrix (tests/gpu_readout_worker.py)"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    outs = [str(tmp_path / f"r{r}.json") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "gpu_readout_worker.py"), str(r), "2", str(port), outs[r]])
             for r in range(2)]
    for pr in procs:
        assert pr.wait(timeout=300) == 0
    res = [json.load(open(o)) for o in outs]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_readout_worker as w
    gyro, frames = w.scene()
    c, d = _feed(_problem(), gyro, frames, 0.0).readout_sweep(w.READOUTS, *w.ARGS)
    for r in res:
        assert r["exchanges"] == 1
        assert r["delays"] == d.tolist()
        np.testing.assert_allclose(r["costs"], c, rtol=1e-12)
    assert res[0]["costs"] == res[1]["costs"]
