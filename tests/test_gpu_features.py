"""The feature tracker on the device (include/rssync_features.h, csrc/kernels/features.hpp) against the numpy restatement
(tests/feature_reference.py), the grid tracker's kernel, and the synthetic video's ground truth."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import feature_reference as fr
import track_reference as tr

pytestmark = pytest.mark.gpu

F0, N_FRAMES, SEED = 30, 41, 77
ROWS, COLS = 760, 1352
FLAT = ((-7.0, 2.0, -7.0), (7.0, 7.0, 7.0))   # the +y part of the box, rendered flat (tools/feature_cpu_delay.py)
# tools/feature_cpu_delay.py: the flat-region clip below, the numpy detector and tracker at the defaults, then the oracle's
# PreSync + Sync fed the driver's way, lands 6.2e-4 s from D_TRUE (21 .. 35 kept tracks per pair; their error against
# the ground truth: median 0.098 px, 99th percentile 0.31 px).
FEATURE_CPU_DELAY_ERROR = 6.2e-4
TRACK_MEDIAN_PX, TRACK_P99_PX = 0.133, 1.16   # tests/test_gpu_track.py: the grid tracker on the plain clip


def _render(flat=None, n=N_FRAMES):
    from rssync_amd import synth, synth_video as sv
    gyro = synth.make_gyro(1.0, 1.0 + (n + 2) / synth.FPS, seed=SEED)
    lens = sv.half_lens()
    out = sv.render(gyro, F0, F0 + n, lens=lens, rows=ROWS, cols=COLS, seed=SEED, flat=flat)
    return (gyro, lens) + tuple(out)


@pytest.fixture(scope="module")
def video():
    return _render()


@pytest.fixture(scope="module")
def flat_video():
    return _render(FLAT)


def _problem():
    import rssync_amd
    return rssync_amd.SyncProblem(seed=321)


def _raw(p, frames, **kw):
    from rssync_amd import features
    return features.raw_features(p, frames, **kw)


def test_detector_is_the_numpy_restatement_bit_for_bit(built, video):
    p = _problem()
    frames = video[2][:2]
    for cell in (16, 64, 128):
        for block in (3, 5, 9):
            for quality in (1e-3, 0.01, 0.5):
                cnt, pts, *_ = _raw(p, frames, cell=cell, block=block, quality=quality)
                want = fr.detect(frames[0], cell, block, quality)
                assert cnt[0] == len(want), (cell, block, quality)
                np.testing.assert_array_equal(pts[0, :cnt[0]], want, err_msg="%d %d %g" % (cell, block, quality))
    rng = np.random.default_rng(11)
    for h, w in ((197, 331), (29, 37), (120, 64), (333, 250)):
        wide = rng.integers(0, 256, size=(3, h, w + 45), dtype=np.uint8)
        frames = wide[:, :, 7:7 + w]                                   # pitch > width, uniform noise
        for cell, block, quality in ((16, 3, 1e-3), (64, 9, 0.01), (128, 5, 0.5), (16, 9, 0.01)):
            cnt, pts, *_ = _raw(p, frames, cell=cell, block=block, quality=quality)
            for k in range(2):
                want = fr.detect(frames[k], cell, block, quality)
                np.testing.assert_array_equal(pts[k, :cnt[k]], want, err_msg="%dx%d %d %d %g" % (w, h, cell, block, quality))


def test_list_lk_equals_grid_lk(built, video):
    from rssync_amd import features
    frames = video[2][:5]
    p = _problem()
    pa, pb, st, res = p.track_points(frames, grid_step=100)
    n, P = pb.shape[:2]
    pts = np.broadcast_to(pa.astype(np.int32), (n, P, 2)).copy()
    flow, lst, lres = features.track_list(p, frames, pts, np.full(n, P, np.uint32))
    np.testing.assert_array_equal(flow, (pb - pa).astype(np.float32))   # (pa + flow in fp64 is exact: the flow comes back)
    np.testing.assert_array_equal(lst, st)
    np.testing.assert_array_equal(lres, res)


_fb_ok = fr.fb_ok


def test_against_the_reference(built, video):
    frames = video[2][:5]
    p = _problem()
    cnt, pts, ff, fbk, st, fb = _raw(p, frames)
    pyrs = [tr.pyramid(f) for f in frames]
    total = 0
    for k in range(len(frames) - 1):
        a = fr.detect(frames[k])
        n = cnt[k]
        np.testing.assert_array_equal(pts[k, :n], a)
        rf, rb, rst, rfb = fr.track_fb(pyrs[k], pyrs[k + 1], a)
        assert _fb_ok(st[k, :n], rst, rfb).all(), (st[k, :n], rst)
        ok = rst == 0
        assert np.abs(ff[k, :n] - rf)[ok].max() <= 1e-3
        assert np.abs(fbk[k, :n] - rb)[ok].max() <= 1e-3
        assert np.abs(fb[k, :n] - rfb)[ok].max() <= 2e-3
        assert np.isnan(fb[k, :n][st[k, :n] % 4 != 0]).all()     # forward failures: no backward pass
        total += ok.sum()
    assert total >= 100


def test_error_against_the_ground_truth(built, video):
    from rssync_amd import synth_video as sv
    gyro, lens, frames, _ = video
    f = _problem().track_features(frames)
    errs = []
    for k in range(len(frames) - 1):
        n = f.counts[k]
        ok = f.status[k, :n] == 0
        a = f.points_a[k, :n][ok]
        truth = sv.true_points(gyro, F0 + k, F0 + k + 2, a, lens=lens, rows=ROWS, seed=SEED)[0]
        errs.append(np.linalg.norm(f.points_b[k, :n][ok] - truth, axis=-1))
    err = np.concatenate(errs)
    assert len(err) >= 20 * (len(frames) - 1)
    assert np.median(err) <= TRACK_MEDIAN_PX * 1.05 and np.percentile(err, 99) <= TRACK_P99_PX * 1.05, \
        (np.median(err), np.percentile(err, 99))


def test_forward_backward_check_drops_a_changed_patch(built, video):
    frames = video[2][:2].copy()
    y0, x0, S = 300, 600, 120
    frames[1, y0:y0 + S, x0:x0 + S] = np.random.default_rng(5).integers(0, 256, size=(S, S), dtype=np.uint8)
    p = _problem()
    f = p.track_features(frames, cell=32, quality=1e-3)
    n = f.counts[0]
    a, b, st = f.points_a[0, :n], f.points_b[0, :n], f.status[0, :n]
    kept = st == 0
    inside = (b[:, 0] >= x0 - 0.5) & (b[:, 0] <= x0 + S - 0.5) & (b[:, 1] >= y0 - 0.5) & (b[:, 1] <= y0 + S - 0.5)
    assert not (kept & inside).any(), b[kept & inside]
    # features whose level-0 windows (21 x 21 plus the gradient's pixel) at a and at the unchanged pair's b stay clear
    clean = p.track_features(video[2][:2], cell=32, quality=1e-3)
    assert clean.counts[0] == n                               # (frame 0 is the same: the same features)
    bt = clean.points_b[0, :n]
    m = 11 + 1

    def clear(q):
        return (q[:, 0] + m < x0) | (q[:, 0] - m > x0 + S - 1) | (q[:, 1] + m < y0) | (q[:, 1] - m > y0 + S - 1)
    far = clear(a) & clear(bt) & (clean.status[0, :n] == 0)
    assert far.sum() >= 100 and (inside | ~kept).sum() > 0
    assert kept[far].mean() >= 0.95, kept[far].mean()


def test_host_device_and_pitched_inputs_agree(built, video):
    f = np.ascontiguousarray(video[2][:5])
    p = _problem()
    want = p.track_features(f)
    wide = np.zeros((5, ROWS, COLS + 61), np.uint8)
    wide[:, :, 13:13 + COLS] = f
    dev = torch.from_numpy(f).to("cuda:0")
    dwide = torch.from_numpy(wide).to("cuda:0")
    for src in (wide[:, :, 13:13 + COLS], dev, dwide[:, :, 13:13 + COLS]):
        got = p.track_features(src)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_overlapping_batches_equal_one_call(built, video):
    frames = video[2]
    p = _problem()
    one = p.track_features(frames[:9])
    first = p.track_features(frames[:5])
    second = p.track_features(frames[4:9])
    for g, a, b in zip(one, first, second):
        np.testing.assert_array_equal(g, np.concatenate([a, b]))


def test_chunk_boundaries_do_not_change_the_result(built, video):
    """20 frames of 2704 x 1520 exceed one chunk slot of the tracker's budget (tests/test_gpu_track.py)"""
    big = np.repeat(np.repeat(video[2][:20], 2, axis=1), 2, axis=2)
    assert big.shape == (20, 1520, 2704)
    p = _problem()
    one = p.track_features(big)
    a = p.track_features(big[:11])
    b = p.track_features(big[10:])
    assert one.status.shape[0] == 19
    for g, x, y in zip(one, a, b):
        np.testing.assert_array_equal(g, np.concatenate([x, y]))
    assert (one.counts > 20).all(), one.counts


def test_features_frames_is_track_then_set_track_pixels(built, video):
    gyro, lens, frames, times = video
    a, b = _problem(), _problem()
    for p in (a, b):
        p.set_gyro_rates(gyro.times, gyro.rates)
    n_set = a.features_frames(frames[:8], times[:8], lens, first_frame=F0)
    f = b.track_features(frames[:8])
    assert n_set == 7
    for k in range(7):
        n = f.counts[k]
        ok = f.status[k, :n] == 0
        b.set_track_pixels(F0 + k, times[k], times[k + 1], f.points_a[k, :n][ok], f.points_b[k, :n][ok], lens, ROWS)
    for k in range(7):
        ra, rb = a.frame_rays(F0 + k)
        sa, sb = b.frame_rays(F0 + k)
        assert ra.shape[0] == (f.status[k, :f.counts[k]] == 0).sum()
        np.testing.assert_array_equal(ra, sa)
        np.testing.assert_array_equal(rb, sb)


def test_pairs_below_min_tracks_are_skipped(built, video):
    gyro, lens, frames, times = video
    p = _problem()
    p.set_gyro_rates(gyro.times, gyro.rates)
    f = p.track_features(frames[:6])
    kept = np.array([(f.status[k, :f.counts[k]] == 0).sum() for k in range(5)])
    m = int(np.median(kept)) + 1
    # an earlier frame at every index: the skipped ones keep it
    old = np.array([[100.0, 100.0], [200.0, 300.0], [400.0, 500.0]])
    for k in range(5):
        p.set_track_pixels(F0 + k, times[k], times[k + 1], old, old + 1.0, lens, ROWS)
    before = [p.frame_rays(F0 + k) for k in range(5)]
    n_set = p.features_frames(frames[:6], times[:6], lens, first_frame=F0, min_tracks=m)
    assert n_set == (kept >= m).sum() and 0 < n_set < 5, (kept, m)
    for k in range(5):
        ra, rb = p.frame_rays(F0 + k)
        if kept[k] >= m:
            assert ra.shape[0] == kept[k]
        else:
            np.testing.assert_array_equal(ra, before[k][0])
            np.testing.assert_array_equal(rb, before[k][1])


def test_constant_frames_give_nothing(built, video):
    _, lens, _, times = video
    p = _problem()
    flat = np.full((3, 300, 400), 77, np.uint8)
    f = p.track_features(flat)
    assert (f.counts == 0).all()
    assert p.features_frames(flat, times[:3], lens) == 0


def test_bad_arguments_raise(built, video):
    import rssync_amd
    from rssync_amd import features
    _, lens, frames, times = video
    p = _problem()
    f = frames[:3]
    cases = [(dict(cell=8), "cell"), (dict(cell=129), "cell"), (dict(block=4), "block"), (dict(block=11), "block"),
             (dict(quality=1.5), "quality"), (dict(quality=-0.1), "quality"), (dict(max_fb_error=-1.0), "max_fb_error"),
             (dict(min_tracks=-1), "min_tracks"), (dict(window=22), "window")]
    for kw, msg in cases:
        with pytest.raises(rssync_amd.RsSyncError, match=msg):
            p.track_features(f, **kw)
    with pytest.raises(rssync_amd.RsSyncError, match="too small"):
        p.track_features(np.zeros((2, 40, 10), np.uint8), block=9, levels=1)    # 2 b + 1 = 11 > 10
    with pytest.raises(rssync_amd.RsSyncError, match="at least 2 frames"):
        p.track_features(f[:1])
    with pytest.raises(rssync_amd.RsSyncError, match="non-finite frame time"):
        p.features_frames(f, [0.0, np.nan, 0.1], lens)
    lib = features.library()
    S = features.n_cells(COLS, ROWS)
    out = [np.zeros(2 * 2 * S), np.zeros(2 * 2 * S), np.zeros(2 * S, np.uint8), np.zeros(2 * S, np.float32), np.zeros(2, np.uint32)]
    args = [o.ctypes.data_as(t) for o, t in zip(out, (C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p,
                                                      C.POINTER(C.c_float), C.POINTER(C.c_uint32)))]
    n = C.c_size_t()
    ptr = f.ctypes.data
    assert lib.rssync_features_track(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, None, *args, S, C.byref(n)) == 0
    assert n.value == S
    assert lib.rssync_features_track(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, None, *args, S - 1, C.byref(n)) != 0
    assert n.value == S and "room" in lib.rssync_last_error().decode()
    assert lib.rssync_features_track(p._h, ptr, 3, COLS, ROWS, COLS - 1, COLS * ROWS, None, *args, S, C.byref(n)) != 0
    assert "pitch" in lib.rssync_last_error().decode()
    prm = features.params()
    prm.lk.grid_step = 200
    assert lib.rssync_features_track(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, C.byref(prm), *args, S, C.byref(n)) != 0
    assert "grid_step" in lib.rssync_last_error().decode()
    t = np.ascontiguousarray(times[:3])
    assert lib.rssync_features_frames(p._h, ptr, 3, COLS, ROWS, COLS, COLS * ROWS, t.ctypes.data_as(C.POINTER(C.c_double)),
                                      0, None, None, None) != 0
    assert "lens" in lib.rssync_last_error().decode()


def _delay(p, frames, times, lens, **kw):
    from rssync_amd import synth
    _, d = p.PreSync(0.0, F0, F0 + len(frames) - 1, 0.002, 0.1)
    _, d = p.Sync(d, F0, F0 + len(frames) - 2, 0.0, 0.2)
    return d, abs(d - synth.D_TRUE)


def test_frames_and_gyro_in_delay_out_on_a_flat_region(built, flat_video):
    gyro, lens, frames, times, mask = flat_video
    grid = tr.grid(COLS, ROWS, 100).astype(int)
    seen = mask[:, grid[:, 1], grid[:, 0]].mean(axis=1)
    assert (seen >= 0.25).all() and (seen <= 0.5).all(), seen
    p = _problem()
    p.set_gyro_rates(gyro.times, gyro.rates)
    assert p.features_frames(frames, times, lens, first_frame=F0) == N_FRAMES - 1
    d, err = _delay(p, frames, times, lens)
    # the grid tracker on the same clip, for the record
    g = _problem()
    g.set_gyro_rates(gyro.times, gyro.rates)
    g.track_frames(frames, times, lens, first_frame=F0, grid_step=100)
    _, gerr = _delay(g, frames, times, lens)
    print("flat clip: features delay error %.3g s, grid tracker %.3g s" % (err, gerr))
    assert err <= 2 * FEATURE_CPU_DELAY_ERROR, (d, err)


def test_frames_and_gyro_in_delay_out_with_many_tracks(built, video):
    """cell 32 and quality 1e-4 on the plain clip: more than 512 kept tracks per pair (of up to 1032 cells), so PreSync
    runs its four-wave kernels on real feature tracks.  The clip's first 31 frames: its last ones turn towards less
    texture and carry only ~530 features at these settings, some of which leave the image."""
    gyro, lens, frames, times = video
    frames, times = frames[:31], times[:31]
    p = _problem()
    f = p.track_features(frames, cell=32, quality=1e-4)
    kept = np.array([(f.status[k, :f.counts[k]] == 0).sum() for k in range(len(frames) - 1)])
    assert (kept > 512).all(), kept
    p.set_gyro_rates(gyro.times, gyro.rates)
    assert p.features_frames(frames, times, lens, first_frame=F0, cell=32, quality=1e-4) == len(frames) - 1
    d, err = _delay(p, frames, times, lens)
    print("cell 32: %d .. %d kept tracks per pair, delay error %.3g s" % (kept.min(), kept.max(), err))
    assert err <= 2 * FEATURE_CPU_DELAY_ERROR, (d, err)
