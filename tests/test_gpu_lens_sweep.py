"""The lens sweep on the device (rssync_ext_lens_sweep, rssync_ext_set_lens; csrc/kernels/support.hpp:
relens_pixels_kernel): the same bits on every route, the re-lens kernel against a full repack, the oracle per candidate,
recovery of the focal length a scene was made with (rssync_amd.lens.estimate_lens), end to end from rendered video, and
across ranks and devices."""
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


def _pixel_scene(sizes, fs=400.0, seed=3, **kw):
    from rssync_amd import synth
    F = len(sizes)
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, fs=fs, seed=seed)
    frames = [next(iter(synth.make_pixel_frames(gyro, fr, fr + 1, n, seed=seed, **kw))) for fr, n in enumerate(sizes)]
    return gyro, frames


def _set_frames(p, frames, lens):
    from rssync_amd import synth
    for fr, ta, tb, pa, pb in frames:
        p.set_track_pixels(fr, ta, tb, pa, pb, lens, synth.IMAGE_ROWS)
    return p


def _feed(p, gyro, frames, lens):
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return _set_frames(p, frames, lens)


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


def _moved(lens, f=1.0, k1=0.0, cx=0.0, cy=0.0, ro=None):
    ro0, fx, fy, cx0, cy0, k10, k2, k3, k4 = lens
    return (ro0 if ro is None else ro, f * fx, f * fy, cx0 + cx, cy0 + cy, k10 + k1, k2, k3, k4)


def _start_lens(lens):
    """a guess without a calibration profile: the focal lengths 15 % low, no distortion terms"""
    ro, fx, fy, cx, cy = lens[:5]
    return np.array((ro, 0.85 * fx, 0.85 * fy, cx, cy, 0.0, 0.0, 0.0, 0.0))


class _Loop:
    """lens_sweep written with the calls that existed before it: every frame set again with the lens (`reset`), then
    PreSync -- what estimate_lens is handed to run the whole search through that loop"""

    def __init__(self, problem, reset):
        self.problem, self.reset = problem, reset

    def lens_sweep(self, lenses, *args):
        res = []
        for lens in np.asarray(lenses):
            self.reset(self.problem, lens)
            res.append(self.problem.PreSync(*args))
        return np.array([r[0] for r in res]), np.array([r[1] for r in res])


# the readout tests' scene: three size classes (the one-wave kernels, four waves of 4 and of 16 rows), a 2 kHz gyro: a
# pair spans ~67 knots at readout 0 and ~127 at 30 ms, so the sweeps' spline windows move from the compiled-in 80 knots to
# dynamic LDS between two candidates
SIZES = [64] * 6 + [600] * 3 + [3000] * 2
ARGS = (0.0, 0, len(SIZES), 0.004, 0.06)


def _lenses():
    from rssync_amd import synth
    L = synth.LENS
    return np.array([_moved(L, f=0.85), _moved(L, f=1.1), _moved(L, k1=-0.08), L, _moved(L, k1=0.06, ro=0.0), _moved(L, cx=70.0, cy=-40.0),
                     _moved(L, ro=0.03), _moved(L, f=0.95, k1=-0.05, cx=-40.0, ro=0.02)])


@pytest.fixture(scope="module")
def classes_scene():
    return _pixel_scene(SIZES, fs=2000.0)


def test_every_route_gives_the_same_bits(built, classes_scene):
    from rssync_amd import synth
    gyro, frames = classes_scene
    lenses = _lenses()
    want_c, want_d, dyn = [], [], []
    loop = _feed(_problem(), gyro, frames, synth.LENS)  # the plain loop: every frame set again, then PreSync
    for lens in lenses:
        _set_frames(loop, frames, lens)
        c, d = loop.PreSync(*ARGS)
        want_c.append(c)
        want_d.append(d)
        dyn.append(loop.window_info()["presync_window_dynamic"])
    assert not dyn[4] and dyn[6], dyn                    # the plan moves to dynamic LDS windows inside the sweep
    assert len(set(want_c)) == len(lenses)
    calls = _feed(_problem(), gyro, frames, synth.LENS)  # per-candidate calls: set_lens (the re-lens kernel), PreSync
    calls.PreSync(*ARGS)
    got = []
    for lens in lenses:
        calls.set_lens(lens)
        got.append(calls.PreSync(*ARGS))
    np.testing.assert_array_equal(_bits([g[0] for g in got]), _bits(want_c))
    np.testing.assert_array_equal(_bits([g[1] for g in got]), _bits(want_d))
    swp = _feed(_problem(), gyro, frames, synth.LENS)
    swp.upload()
    swp.profile(True)
    c1, d1 = swp.lens_sweep(lenses, *ARGS)              # the pipeline
    prof = swp.profile_get()
    assert prof["relens"][0] >= len(lenses) + 1 and prof["pixels"][0] == 0, prof   # a launch per candidate, one to restore; no repack
    os.environ["RSSYNC_SWEEP_PIPELINE"] = "0"
    try:
        c0, d0 = swp.lens_sweep(lenses, *ARGS)          # one lens after the other
    finally:
        del os.environ["RSSYNC_SWEEP_PIPELINE"]
    for c, d in ((c1, d1), (c0, d0)):
        np.testing.assert_array_equal(_bits(c), _bits(want_c))
        np.testing.assert_array_equal(_bits(d), _bits(want_d))
    # lenses that differ only in ro: the readout sweep's arrays
    readouts = np.arange(0.0, 0.03001, 0.005)
    cr, dr = swp.readout_sweep(readouts, *ARGS)
    cl, dl = swp.lens_sweep([_moved(synth.LENS, ro=ro) for ro in readouts], *ARGS)
    np.testing.assert_array_equal(_bits(cl), _bits(cr))
    np.testing.assert_array_equal(_bits(dl), _bits(dr))


def test_relensed_streams_equal_a_repack(built, classes_scene):
    from rssync_amd import synth
    gyro, frames = classes_scene
    ids = [f[0] for f in frames]
    end = len(SIZES) - 1
    p = _feed(_problem(max_outer_iters=30), gyro, frames, synth.LENS)
    base_rays, base = _rays(p, ids), p.PreSync(*ARGS)
    for lens in _lenses()[[0, 5, 7]]:
        p.set_lens(lens)
        q = _feed(_problem(max_outer_iters=30), gyro, frames, lens)
        _same_rays(_rays(p, ids), _rays(q, ids))
        pre = p.PreSync(*ARGS)
        assert pre == q.PreSync(*ARGS)
        # the fp64 streams: Sync (its sampler streams follow an object's count of Sync calls, so from an object that
        # has made as many as the fresh one -- none)
        s = _feed(_problem(max_outer_iters=30), gyro, frames, synth.LENS)
        s.upload()
        s.set_lens(lens)
        assert s.Sync(pre[1], 0, end, 0.0, 0.2) == q.Sync(pre[1], 0, end, 0.0, 0.2)
    p.set_lens(synth.LENS)
    _same_rays(_rays(p, ids), base_rays)
    # after a sweep each frame holds its own lens, frames with different lenses included: streams, PreSync, Sync as before
    s = _feed(_problem(max_outer_iters=30), gyro, frames, synth.LENS)
    r = _feed(_problem(max_outer_iters=30), gyro, frames, synth.LENS)
    for x in (s, r):
        _set_frames(x, frames[2:3], _lenses()[7])
        _set_frames(x, frames[9:10], _lenses()[1])
    own_rays, own = _rays(r, ids), r.PreSync(*ARGS)
    s.lens_sweep(_lenses(), *ARGS)
    _same_rays(_rays(s, ids), own_rays)
    assert s.PreSync(*ARGS) == own
    assert s.Sync(own[1], 0, end, 0.0, 0.2) == r.Sync(own[1], 0, end, 0.0, 0.2)


def test_errors_and_broken_lenses(built):
    """the complaints before anything is touched, and a lens that is finite and positive but turns the rays non-finite
    (focal lengths so small that the normalised coordinates overflow): counted by the re-lens kernel, reported after the
    sweep's one wait with the candidate's number, every frame restored; set_lens with it behaves as setting the frames
    again does -- the next use complains"""
    import rssync_amd
    from rssync_amd import synth
    gyro, frames = _pixel_scene([64] * 4 + [600] * 2)
    ids = [f[0] for f in frames]
    args = (0.0, 0, 6, 0.004, 0.06)
    p = _feed(_problem(), gyro, frames, synth.LENS)
    base_rays, base = _rays(p, ids), p.PreSync(*args)
    broken = np.array(synth.LENS)
    broken[1:3] = 1e-300
    for env in (None, "0"):
        if env:
            os.environ["RSSYNC_SWEEP_PIPELINE"] = env
        try:
            with pytest.raises(rssync_amd.RsSyncError, match=r"lens sweep: lens 2: non-finite numbers in rays \(1456 tracks"):
                p.lens_sweep([synth.LENS, _moved(synth.LENS, f=0.9), broken, broken], *args)
        finally:
            os.environ.pop("RSSYNC_SWEEP_PIPELINE", None)
        _same_rays(_rays(p, ids), base_rays)
        assert p.PreSync(*args) == base
    for bad, what in ((_moved(synth.LENS, ro=-1e-3), "readout"), (_moved(synth.LENS, f=0.0), "focal"), (_moved(synth.LENS, k1=float("nan")), "non-finite")):
        with pytest.raises(rssync_amd.RsSyncError, match="lens sweep: lens 1 .*" + what):
            p.lens_sweep([synth.LENS, bad], *args)
        with pytest.raises(rssync_amd.RsSyncError, match="set-lens: .*" + what):
            p.set_lens(bad)
    with pytest.raises(rssync_amd.RsSyncError, match="no lenses"):
        p.lens_sweep(np.zeros((0, 9)), *args)
    p.SetTrackResult(*next(iter(synth.make_frames(gyro, 6, 7, 50, seed=3))))
    with pytest.raises(rssync_amd.RsSyncError, match="frame 6 was set as rays"):
        p.lens_sweep(_lenses(), 0.0, 0, 7, 0.004, 0.06)
    assert p.PreSync(*args) == base
    p.set_lens(broken)
    with pytest.raises(rssync_amd.RsSyncError, match="non-finite numbers in rays"):
        p.PreSync(*args)
    p.set_lens(synth.LENS)
    assert p.PreSync(*args) == base


def test_each_candidate_matches_the_oracle_presync(built):
    """clean scene; the oracle gets the rays the reference driver would make with each candidate lens"""
    from oracle import oracle
    from oracle.oracle import OracleProblem
    from rssync_amd import synth
    gyro, frames = _pixel_scene([128] * 16, seed=4, noise_px=0.0, outliers=0.0)
    L = synth.LENS
    lenses = [_moved(L, f=0.9), _moved(L, k1=-0.05), L, _moved(L, cx=50.0), _moved(L, f=1.1, ro=0.016)]
    args = (0.0, 0, 16, 0.002, 0.1)
    costs, delays = _feed(_problem(), gyro, frames, _start_lens(L)).lens_sweep(lenses, *args)
    for i, lens in enumerate(lenses):
        o = OracleProblem(seed=SEED, threads=os.cpu_count() or 1, faithful=False)
        o.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
        for fr, ta, tb, pa, pb in frames:
            o.SetTrackResult(fr, *oracle.pixels_to_tracks(lens, ta, tb, synth.IMAGE_ROWS, pa, pb))
        co, do = o.PreSync(*args)
        assert delays[i] == do, (i, delays[i], do)
        assert abs(costs[i] - co) <= 5e-3 * abs(co), (i, costs[i], co)   # the noise-free tolerance of smoke()
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


# The bound of the recovery test: 1 %, from the CPU runs of the search through set_track_pixels + PreSync (40 x 200
# tracks: 0.35 % off; the final grid step is 1 %).  The MI355X's loop through the same calls on this scene ends 0.021 %
# off (below), so the bound stays as the CPU runs set it.
RECOVERY_FX_TOL = 0.01


def test_the_search_recovers_the_focal_length_and_with_it_the_delay(built):
    """120 frames x 256 tracks, seed 1 (true lens synth.LENS, 0.3 px noise, 10 % outliers), installed with the focal
    lengths 15 % low and no distortion terms; the search over ("f", "k1") with a fine PreSync (0.5 ms step).
    Measured on the MI355X, through the sweep and, with the same bits, through the loop of set_track_pixels + PreSync: fx
    1179.76 against 1180 (0.021 % low), k1 0.0560 against 0.05 (it absorbs the zeroed higher terms), cost 916.617, no
    parameter unresolved.  Delay after set_lens, PreSync and 4 x Sync: 37.503 ms with the estimate against 38.051 ms with
    the start lens (truth 37.0 ms; the true lens itself gives 37.931 ms on this noise)."""
    from rssync_amd import synth
    from rssync_amd.lens import estimate_lens
    gyro, frames = _recovery_scene()
    F = len(frames)
    start = _start_lens(synth.LENS)
    p = _feed(_problem(), gyro, frames, start)
    est = estimate_lens(p, start, 0.0, 0, F, 0.0005, 0.1)
    print("fx %.2f (truth %.0f, %.3f %% off), k1 %.4f (truth %.2f), cost %.3f, presync delay %.4f s, unresolved %s"
          % (est.lens[1], synth.LENS[1], 100 * (est.lens[1] / synth.LENS[1] - 1), est.lens[5], synth.LENS[5], est.cost, est.delay, est.unresolved))
    assert abs(est.lens[1] / synth.LENS[1] - 1.0) <= RECOVERY_FX_TOL
    assert est.unresolved == ()
    wrong = _delay_after_sync(_feed(_problem(), gyro, frames, start), F)
    p.set_lens(est.lens)
    d = _delay_after_sync(p, F)
    print("delay after PreSync + 4 x Sync: %.6f s with the estimate, %.6f s with the start lens (truth %.4f)" % (d, wrong, synth.D_TRUE))
    assert abs(d - synth.D_TRUE) < abs(wrong - synth.D_TRUE)


# measured on the MI355X through the loop that detects and tracks the clip again for every candidate lens
# (features_frames + PreSync, 55 times): the search ends at fx 595.26 against 590, 0.891 % off; the bound leaves one
# final grid step (1 %) beyond that, as VIDEO_READOUT_TOL of the readout tests is stated
VIDEO_FX_TOL = 0.00891 + 0.01


@pytest.fixture(scope="module")
def video_clip():
    """test_gpu_readout_sweep.py::test_end_to_end_from_rendered_video's clip"""
    from rssync_amd import synth, synth_video as sv
    F0, n, rows, cols = 30, 41, 760, 1352
    gyro = synth.make_gyro(1.0, 1.0 + (n + 2) / synth.FPS, seed=77)
    lens = sv.half_lens()
    frames, times = sv.render(gyro, F0, F0 + n, lens=lens, rows=rows, cols=cols, seed=77)[:2]
    return gyro, lens, frames, times, F0, n


def _video_problem(clip, lens):
    gyro, _, frames, times, F0, n = clip
    p = _problem()
    p.set_gyro_rates(gyro.times, gyro.rates)
    assert p.features_frames(frames, times, lens, first_frame=F0) == n - 1
    return p


def _video_reset(clip):
    _, _, frames, times, F0, n = clip
    return lambda p, lens: p.features_frames(frames, times, lens, first_frame=F0)


def test_end_to_end_from_rendered_video(built, video_clip):
    """the readout tests' rendered clip (sv.half_lens(), 41 frames of 1352 x 760), features detected and tracked with the
    start lens -- focal lengths 15 % low, no distortion terms.  A sweep equals the loop through features_frames + PreSync
    bit for bit, and the search built on it finds the focal length within VIDEO_FX_TOL.  Measured on the MI355X: fx
    595.26 against 590 (0.891 % high), k1 0.0555 against 0.05, PreSync delay 38 ms, no parameter unresolved (the first
    pass over "f" ends on its grid's edge, +25 %, and the later passes come back from there)."""
    from rssync_amd.lens import estimate_lens, shifted
    _, lens, _, _, F0, n = video_clip
    start = _start_lens(lens)
    args = (0.0, F0, F0 + n - 1, 0.002, 0.1)
    p = _video_problem(video_clip, start)
    # one sweep against the loop that detects and tracks the clip again for every lens
    cands = np.stack([shifted(start, "f", g) for g in (-0.1, 0.0, 0.15, 0.3)] + [shifted(start, "k1", 0.08)])
    want_c, want_d = _Loop(_video_problem(video_clip, start), _video_reset(video_clip)).lens_sweep(cands, *args)
    got_c, got_d = p.lens_sweep(cands, *args)
    np.testing.assert_array_equal(_bits(got_c), _bits(want_c))
    np.testing.assert_array_equal(_bits(got_d), _bits(want_d))
    est = estimate_lens(p, start, *args)
    print("rendered clip: fx %.2f (truth %.1f, %.3f %% off), k1 %.4f, presync delay %.4f, unresolved %s"
          % (est.lens[1], lens[1], 100 * (est.lens[1] / lens[1] - 1), est.lens[5], est.delay, est.unresolved))
    assert abs(est.lens[1] / lens[1] - 1.0) <= VIDEO_FX_TOL


def test_two_contexts_in_one_object_give_the_same_bits(built):
    """frames spread over two contexts (cut at 64 frames) on the box's device: every shard re-lenses its own frames"""
    from rssync_amd import synth
    gyro, frames = _pixel_scene([48] * 130, seed=8)
    args = (0.0, 0, 130, 0.004, 0.06)
    lenses = _lenses()[[0, 3, 5, 7]]
    one = _feed(_problem(), gyro, frames, synth.LENS).lens_sweep(lenses, *args)
    p = _problem()
    p.set_devices([0, 0])
    many = _feed(p, gyro, frames, synth.LENS).lens_sweep(lenses, *args)
    for a, b in zip(one, many):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    p.set_lens(lenses[2])
    assert p.PreSync(*args) == (one[0][2], one[1][2])


def test_two_ranks_one_exchange_per_sweep(built, tmp_path):
    """two gloo ranks on the box's device, each with half the frames: the same arg-mins as one process, and one exchange
    for the whole [lens][candidate] matrix (tests/gpu_lens_worker.py)"""
    from rssync_amd import synth
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    outs = [str(tmp_path / f"r{r}.json") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "gpu_lens_worker.py"), str(r), "2", str(port), outs[r]])
             for r in range(2)]
    for pr in procs:
        assert pr.wait(timeout=300) == 0
    res = [json.load(open(o)) for o in outs]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_lens_worker as w
    gyro, frames = w.scene()
    c, d = _feed(_problem(), gyro, frames, synth.LENS).lens_sweep(w.lenses(), *w.ARGS)
    for r in res:
        assert r["exchanges"] == 1
        assert r["delays"] == d.tolist()
        np.testing.assert_allclose(r["costs"], c, rtol=1e-12)
    assert res[0]["costs"] == res[1]["costs"]
