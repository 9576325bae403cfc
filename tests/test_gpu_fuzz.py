"""Randomised differential cases, HIP against the CPU restatement: gyro rate (200 Hz .. 6.4 kHz), number of frames, ragged track
counts (2 .. 2300: frames of one wave and of four with 4 / 8 / 16 rows per thread -- up to four SIZE CLASSES in one problem,
round 5), sparse frame ids, sweep
step / radius / centre all drawn per seed.  What is compared is what does not depend on rounding noise: the fp64
rows, the fp64 loss and its analytic gradient, PreSync's per-frame costs where both sides chose the same
hypothesis, the arg-min of the sweep, and Sync on noise-free scenes."""
import os

import numpy as np
import pytest

import rssync_amd
from rssync_amd import synth
from oracle.oracle import OracleProblem, sample_pair

from lmeds_reference import exact_winners, flip_interval, lower_quartile_fp64  # noqa: F401 (moved there: tests/test_gpu_guess_motion.py shares them)

pytestmark = pytest.mark.gpu

RATES = [200.0, 400.0, 500.0, 800.0, 1000.0, 1600.0, 2000.0, 3200.0, 4000.0, 6400.0]   # (above ~1.7 kHz: spline windows in dynamic LDS)
# RSSYNC_FUZZ_CASES=200 widens the seed ranges for a one-off soak; the committed default keeps the suite short
EXTRA = int(os.environ.get("RSSYNC_FUZZ_CASES", "0"))


def draw_case(seed, clean):
    rng = np.random.default_rng(1000 + seed)
    fs = RATES[int(rng.integers(len(RATES)))]
    F = int(rng.integers(3, 15))
    first = int(rng.integers(0, 40))
    ids = first + np.sort(rng.choice(3 * F, size=F, replace=False))
    n_max = int(rng.choice([40, 130, 256, 300, 520, 700, 1100, 2300], p=[.15, .15, .15, .15, .15, .15, .05, .05]))
    counts = [int(rng.integers(2, n_max + 1)) for _ in range(F)]
    counts[int(rng.integers(F))] = n_max
    g = synth.make_gyro(first / synth.FPS, (int(ids[-1]) + 2) / synth.FPS, fs=fs, seed=seed)
    kw = dict(noise=0.0, outliers=0.0) if clean else {}
    frames = []
    for fid, n in zip(ids, counts):
        (fr, ta, tb, ra, rb), = list(synth.make_frames(g, int(fid), int(fid) + 1, n_max, seed=seed, **kw))
        frames.append((fr, ta[:n], tb[:n], ra[:n], rb[:n]))
    return rng, g, frames, counts


def build(seed, g, frames, **kw):
    h = rssync_amd.SyncProblem(seed=seed, verbose=False, **kw)
    o = OracleProblem(seed=seed, faithful=False, threads=min(os.cpu_count() or 1, 8), **kw)
    for p in (h, o):
        p.SetGyroQuaternions(g.quats, g.fs, g.t0)
        for fr in frames:
            p.SetTrackResult(*fr)
    return h, o


@pytest.mark.parametrize("seed", range(10 + EXTRA))
def test_random_noisy_case(seed):
    rng, g, frames, counts = draw_case(seed, clean=False)
    h, o = build(seed, g, frames)
    ids = [fr[0] for fr in frames]
    lo, hi = ids[0], ids[-1] + 1
    # fp64 rows of a random frame at a random delay (also outside the gyro span)
    for _ in range(3):
        k = int(rng.integers(len(frames)))
        delay = float(rng.choice([rng.uniform(-0.05, 0.08), rng.uniform(-3.0, 3.0)]))
        P = h.problem_matrix64(ids[k], delay, counts[k])
        Po = o.problem_matrix(ids[k], delay)
        assert P.shape == Po.shape
        assert np.abs(P - Po).max() < 1e-13 * max(1.0, np.abs(Po).max())
    # the sweep
    step = float(rng.choice([0.0005, 0.001, 0.002, 0.004]))
    radius = float(rng.uniform(0.005, 0.06))
    centre = synth.D_TRUE + float(rng.uniform(-0.01, 0.01))
    nf = len(frames)
    dh, ch, fch, bhh = h.presync_curve(centre, lo, hi, step, radius, per_frame=nf)
    do, co, fco, bho = o.presync_curve(centre, lo, hi, step, radius, per_frame=nf)
    np.testing.assert_array_equal(dh, do)
    # With a handful of rows the lower quartile sits at the two rows that define the hypothesis, whose residuals
    # are rounding noise (1e-16 in fp64, 1e-8 in fp32): which hypothesis wins there is not comparable, and a
    # frame's cost follows the winner.  The comparison is therefore made on the frames with >= 48 tracks, and
    # the curve / arg-min checks on their share of the sum (the cost is a plain sum over frames).
    big = np.array([n >= 48 for n in counts])
    res_h, res_o = h.PreSync(centre, lo, hi, step, radius), o.PreSync(centre, lo, hi, step, radius)
    assert res_h[0] == pytest.approx(float(ch.min()), rel=1e-12) and res_h[1] == dh[int(np.argmin(ch))]
    if big.any():
        same = (bhh == bho)[:, big]
        assert same.mean() > 0.9
        np.testing.assert_allclose(fch[:, big][same], fco[:, big][same], rtol=3e-3)
        cbh, cbo = fch[:, big].sum(axis=1), fco[:, big].sum(axis=1)
        rel = np.abs(cbh - cbo) / cbo   # a candidate where one frame's near-tie went the other way moves by a few %
        # A TOLERANCE WIDENED TO PASS, on the record: until round 4 this read "> 90 % of the candidates within 3e-3".  Soak
        # case 360 (gpurun_out/r4l_fuzz_check.log: a sweep of FOUR candidates, one frame's near-tie between two hypotheses
        # fell the other way in fp32 at one of them: 1 of 4 = 25 % outside) failed that form without anything being wrong --
        # a single flip is the fp32 search's stated behaviour -- so the count allowed is now
        # max(1, 10 %): one flip however few candidates a case draws.
        assert np.sum(rel > 3e-3) <= max(1, 0.1 * len(rel))
        # ... and HOW FAR a flip moves a candidate's cost says nothing (round 5, soak case 230: the only flip of the case, on
        # one of three frames, moved that candidate by 16 % and failed the blanket "< 10 %" that stood here).  What makes a
        # flip legitimate is that the two hypotheses TIE in the reference's own arithmetic as far as the fp32 search can
        # tell: their lower-quartile residuals, recomputed here in fp64 from the oracle's rows, differ by no more than the
        # fp32 rows' error can move either of them.  A direction v = P[i0] x P[i1] built from rows known to 5e-7 absolute
        # (profiles/r4_config2_parity.json) is off by up to err_v = 5e-7 (1/|P[i0]| + 1/|P[i1]|) / sin(angle) radians, and a
        # residual n.v by as much.  Allowed: 0.2 err_v (of the worse-conditioned of the two) + 0.5 % of the residual.
        # Measured on 6000 soaked cases (profiles/r5_fuzz_soak.txt): 10 flips above 1 % of the quartile, every one with a
        # defining row below 1.3e-4 or a pair within 0.6 degrees of parallel, the largest at 0.066 err_v; well-conditioned
        # pairs flip at <= 1e-4.  A winner chosen WRONGLY would be off by O(1): quartiles of unrelated hypotheses differ by
        # factors.
        # And the quartile is an ORDER STATISTIC of residuals that each carry the error of their own row: a row of norm |P_i|
        # is off by up to 5e-7 / |P_i| in direction, so residuals within that of the quartile value may change sides, and
        # with m such rows the fp32 quartile is any of the order statistics kq - m .. kq + m (at 50 tracks neighbouring
        # order statistics at the quartile lie ~7 % apart: soak cases 3809 and 3963 of run 5, 2.2 % and 0.6 %).  So what is
        # compared is the INTERVAL each hypothesis' quartile can lie in: flip_interval() below.
        flips = [(c, j) for c, j in zip(*np.nonzero(bhh != bho)) if big[j] and bhh[c, j] >= 0 and bho[c, j] >= 0]
        for c, j in flips[:12]:
            P = o.problem_matrix(ids[j], float(do[c]))
            iv = [flip_interval(P, *sample_pair(seed, ids[j], int(c), int(w), counts[j])) for w in (bhh[c, j], bho[c, j])]
            gap = max(iv[0][0], iv[1][0]) - min(iv[0][1], iv[1][1])        # > 0: the intervals do not meet
            assert gap <= 5e-3 * iv[1][2], (seed, int(c), int(ids[j]), iv)
        srt = np.sort(cbo)
        if len(srt) > 1 and srt[1] - srt[0] > 0.08 * srt[0]:   # a clear minimum: the same candidate wins
            assert int(np.argmin(cbh)) == int(np.argmin(cbo))
    # fp64 loss and gradient at the GPU's own motion estimates
    d0 = res_h[1]
    Mh, kh = h.init_motion(d0, lo, hi - 1)
    for dd in (d0, d0 + 7e-4):
        Lh, Gh = h.loss([dd], grad=True)
        L = G = 0.0
        for j, fid in enumerate(ids):
            l, _, da, _ = o.loss(fid, dd, Mh[j], kh[j])
            L += l
            G += da
        assert Lh[0] == pytest.approx(L, rel=1e-11)
        assert Gh[0] == pytest.approx(G, rel=1e-9, abs=1e-9 * abs(L))


@pytest.mark.parametrize("seed", range(300, 306 + EXTRA))
def test_the_winner_is_the_exact_argmin_of_the_devices_own_residuals(seed, variants_lib):
    """THE TOLERANCE-FREE ANCHOR under the flip check (a check that grows a term per failure ends up explaining
    anything).  flip_interval() above explains device-vs-fp64 differences with the fp32 rows' conditioning; it says nothing
    about whether the device's selection is RIGHT on its own numbers.  This does, exactly: the TEST-VARIANTS build of the
    library dumps the |residuals| its sweep worked on -- every hypothesis of every (frame, candidate), from the same tile
    and the same directions -- and for EVERY pair of the case the kernel's winner must be the exact arg-min of the
    residuals' lower quartile (np.partition on the device's own floats) with the reference's first-wins rule
    (core_private.cpp:48-56): lazy brackets, provisional bounds, contenders, early rejection, the one-wave kernels'
    sequential search and the large-frame kernels' bisection included -- assert_array_equal, no tolerance.  And the PRODUCT
    library (no dump code in its kernels) must return the same winners as the variants build (and its costs to fp32 rounding)."""
    rng, g, frames, counts = draw_case(seed, clean=bool(seed % 3 == 0))
    ids = [fr[0] for fr in frames]
    lo, hi = ids[0], ids[-1] + 1
    step = float(rng.choice([0.0005, 0.001, 0.002]))
    radius = float(rng.uniform(0.004, 0.02))                         # <= 80 candidates: the dump stays below a few hundred MB
    centre = synth.D_TRUE + float(rng.uniform(-0.01, 0.01))
    nf = len(frames)
    v = rssync_amd.SyncProblem(seed=seed, verbose=False, _lib=variants_lib)
    hprod = rssync_amd.SyncProblem(seed=seed, verbose=False)
    for p in (v, hprod):
        p.SetGyroQuaternions(g.quats, g.fs, g.t0)
        for fr in frames:
            p.SetTrackResult(*fr)
    v.debug_residuals(True, cap_rows=max(counts))
    dv, cv, fcv, bhv = v.presync_curve(centre, lo, hi, step, radius, per_frame=nf)
    res = v.debug_residuals_get()
    assert res.shape == (len(dv), nf, 20, max(counts))
    for j, n in enumerate(counts):                                   # every row of every frame was written, nothing beyond
        assert not np.isnan(res[:, j, :, :n]).any() and np.isnan(res[:, j, :, n:]).all()
    np.testing.assert_array_equal(bhv, exact_winners(res, counts))
    dp, cp, fcp, bhp = hprod.presync_curve(centre, lo, hi, step, radius, per_frame=nf)
    # The product against the variants build: the same sources, but two BUILDS -- the dump's loop follows stage D, and the fp32
    # kernels are compiled under -ffp-contract=fast, so the two schedule and contract stage A and stage D differently (costs:
    # 7e-8 on 1 of 490 in seed 300).  On frames of >= 48 tracks the winners are the same; with a handful of rows the lower
    # quartile sits at the hypothesis' own defining rows, whose residuals are rounding noise (1e-8): there a last bit of a row
    # decides and the two builds may differ (seed 389: 4 of 322 pairs, all on frames of 5 .. 30 tracks) -- each build's winner
    # being the exact arg-min of ITS OWN residuals is what the anchor above demands, of the build that can show them.
    big = np.array([n >= 48 for n in counts])
    diff = np.argwhere(bhp != bhv)
    assert all(not big[j] for _, j in diff), [(int(c), int(j), counts[j]) for c, j in diff]
    np.testing.assert_allclose(fcp[:, big], fcv[:, big], rtol=2e-6)
    with pytest.raises(rssync_amd.RsSyncError):                      # the product has no such code
        hprod.debug_residuals(True, cap_rows=8)


@pytest.mark.parametrize("seed", range(500, 508 + EXTRA))
def test_random_mixtures_of_near_static_and_ordinary_frames(seed):
    """Round 6's fp64 rows (kernels/lmeds.hpp) under random shapes: 3-12 frames of ragged sizes (one wave per frame up to the
    eight-wave tile), each near-static (translation 3e-6 .. 3e-4 m per frame, ray noise in proportion) or ordinary, a random
    gyro rate, candidates a few microseconds apart around the truth in chunks of random length.  Against the oracle: the
    winners of every frame of >= 48 tracks agree in >= 98 % of the pairs (near-static or not; one flip allowed however few), costs to 3e-3 where they do;
    exactly the pairs whose fp64 rows (the oracle's) say so took the fp64 form -- a near-static frame is only near-static close to
    the true delay --, no pair of an ordinary frame did; a second sweep finds the
    bitmap clean (the same bits, the count doubled)."""
    rng = np.random.default_rng(7000 + seed)
    fs = RATES[int(rng.integers(len(RATES)))]
    F = int(rng.integers(3, 13))
    sizes = [int(rng.choice([60, 130, 300, 520, 700, 1100, 2300, 5000], p=[.1, .2, .15, .15, .1, .1, .15, .05])) for _ in range(F)]
    g = synth.make_gyro(0.0, (F + 2) / synth.FPS, fs=fs, seed=seed)
    frames, kind = [], []
    for fr, n in enumerate(sizes):
        if rng.random() < 0.5:
            tr = float(10 ** rng.uniform(-5.5, -3.5))
            frames += list(synth.make_frames(g, fr, fr + 1, n, seed=seed, noise=tr / 50.0, outliers=float(rng.choice([0.0, 0.1, 0.2])), translation=tr))
            kind.append(tr)
        else:
            frames += list(synth.make_frames(g, fr, fr + 1, n, seed=seed))
            kind.append(None)
    h, o = build(seed, g, frames)
    step = float(rng.choice([2e-6, 5e-6, 2e-5]))
    radius = step * float(rng.uniform(5, 40))
    centre = synth.D_TRUE + float(rng.uniform(-1e-4, 1e-4))
    dh, ch, fch, bhh = h.presync_curve(centre, 0, F, step, radius, per_frame=F)
    do, co, fco, bho = o.presync_curve(centre, 0, F, step, radius, per_frame=F)
    np.testing.assert_array_equal(dh, do)
    nc = len(dh)
    big = np.array([n >= 48 for n in sizes])
    same = (bhh == bho)[:, big]
    # (one flip however few pairs a case draws: a near-tie that falls the other way is the fp32 search's stated behaviour, as in
    # test_random_noisy_case; seed 1040 of the soak: 1 of 48)
    assert np.sum(~same) <= max(1, 0.02 * same.size), (same.mean(), sizes, kind)
    np.testing.assert_allclose(fch[:, big][same], fco[:, big][same], rtol=3e-3)
    st = h.near_static_stats()
    # which pairs SHOULD have taken the fp64 form, from the oracle's fp64 rows: a quarter or more of the frame's first 64 rows
    # with |P| < 2e-4 (a near-static frame is only near-static close to the true delay: 0.5 ms away its rows are ordinary).
    # Pairs whose fraction is within one row of the quarter may fall either way (the device counts fp32 rows).
    sure = unsure = 0
    for fr, n in enumerate(sizes):
        if kind[fr] is None:
            continue
        m = min(n, 64)
        for c in range(nc):
            P = o.problem_matrix(fr, float(do[c]))[:m]
            k = int(np.sum(np.einsum("ij,ij->i", P, P) < 4e-8))
            if 4 * (k - 1) >= m:
                sure += 1
            elif 4 * (k + 1) >= m:
                unsure += 1
    assert sure <= st["pairs"] <= sure + unsure, (st, sure, unsure, nc, kind)
    assert sure > 0 or all(k is None for k in kind) or unsure > 0 or st["pairs"] == 0
    d2, c2, fc2, bh2 = h.presync_curve(centre, 0, F, step, radius, per_frame=F)
    np.testing.assert_array_equal(fc2.view(np.uint64), fch.view(np.uint64))
    np.testing.assert_array_equal(bh2, bhh)
    assert h.near_static_stats()["pairs"] == 2 * st["pairs"]


@pytest.mark.parametrize("noise", [1e-3, 0.0])
def test_the_anchor_in_every_size_class(noise, variants_lib):
    """the same anchor with one frame of every kernel family in one problem: one wave per frame (130, 400 tracks), four waves
    with 4 / 8 / 16 / 24 rows per thread (900, 2000, 3500, 6000), EIGHT waves of 16 rows (7000, 8192: round 6's shape for 6145 ..
    8192 tracks) and the large-frame kernel (9000) -- every winner the exact arg-min of the kernel's own residuals, first wins"""
    counts = [130, 400, 900, 2000, 3500, 6000, 7000, 8192, 9000]
    F = len(counts)
    g = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=77)
    kw = dict(noise=0.0, outliers=0.0) if noise == 0.0 else dict(noise=noise)
    frames = [next(iter(synth.make_frames(g, fr, fr + 1, n, seed=77, **kw))) for fr, n in enumerate(counts)]
    v = rssync_amd.SyncProblem(seed=5, verbose=False, _lib=variants_lib)
    hprod = rssync_amd.SyncProblem(seed=5, verbose=False)
    for p in (v, hprod):
        p.SetGyroQuaternions(g.quats, g.fs, g.t0)
        for fr in frames:
            p.SetTrackResult(*fr)
    v.debug_residuals(True, cap_rows=max(counts))
    dv, cv, fcv, bhv = v.presync_curve(synth.D_TRUE, 0, F, 0.0005, 0.004, per_frame=F)      # 16 candidates
    res = v.debug_residuals_get()
    assert res.shape == (len(dv), F, 20, max(counts))
    for j, n in enumerate(counts):
        assert not np.isnan(res[:, j, :, :n]).any() and np.isnan(res[:, j, :, n:]).all()
    np.testing.assert_array_equal(bhv, exact_winners(res, counts))
    dp, cp, fcp, bhp = hprod.presync_curve(synth.D_TRUE, 0, F, 0.0005, 0.004, per_frame=F)
    np.testing.assert_array_equal(bhp, bhv)
    np.testing.assert_allclose(fcp, fcv, rtol=2e-6)


@pytest.mark.parametrize("seed", range(100, 106 + EXTRA))
def test_random_clean_case_sync(seed):
    """without noise the minimum is sharp and Sync is not chaotic: both sides end at the true delay"""
    rng, g, frames, counts = draw_case(seed, clean=True)
    if min(counts) < 16:   # GuessMotion on a handful of rows is a coin toss on either side
        frames = [fr for fr, n in zip(frames, counts) if n >= 16]
    h, o = build(seed, g, frames, max_outer_iters=60)
    ids = [fr[0] for fr in frames]
    lo, hi = ids[0], ids[-1]
    start = synth.D_TRUE + float(rng.uniform(-0.002, 0.002))
    ch, dh = h.Sync(start, lo, hi, 0.0, 0.5)
    co, do = o.Sync(start, lo, hi, 0.0, 0.5)
    # the two solvers agree far better than either agrees with the truth (a few frames, capped iterations)
    assert abs(dh - do) < 2e-6, (dh, do)
    # (how near the truth both end is a property of the ALGORITHM on the draw -- a few frames, 60 capped iterations --, not of
    # the device: 1 of 3000 soaked draws, seed 983, ends 1.6 ms away ON BOTH SIDES, the two 2e-10 s apart)
    assert abs(dh - synth.D_TRUE) < (1e-3 if seed < 200 else 3e-3), (dh, do)
    assert ch == pytest.approx(co, rel=1e-3, abs=1e-9)


@pytest.mark.parametrize("seed", range(200, 203 + EXTRA // 5))
def test_random_batched_windows_device_loop_equals_host_loop(seed):
    """random sets of overlapping windows through the device-driven loop (groups of windows on concurrent streams)
    and through the host loop: the same bits"""
    rng = np.random.default_rng(seed)
    F = int(rng.integers(150, 500))
    N = int(rng.choice([20, 64, 130, 200, 300]))
    window = int(rng.integers(8, 40))
    dist = int(rng.integers(3, 15))
    repeats = int(rng.integers(1, 4))
    max_outer = int(rng.integers(5, 40))
    g = synth.make_gyro(0, (F + 2) / synth.FPS, seed=seed)
    pos = list(range(0, F - window - 1, dist))
    out = []
    for host in (False, True):
        p = rssync_amd.SyncProblem(seed=seed, verbose=False, max_outer_iters=max_outer)
        synth.fill(p, g, 0, F, N, seed=seed)
        p.set_host_loop(host)
        c, d = p.sync_points(pos, window, 0.0, 0.002, 0.06, repeats=repeats)
        out.append((np.array(c), np.array(d), [np.array(p.window_trace(w)) for w in range(len(pos))]))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][2], out[1][2]):
        np.testing.assert_array_equal(a, b)
