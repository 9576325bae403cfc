"""GuessMotion's search (MODE 1 of the LMedS tile kernel, kernels/lmeds.hpp: 200 hypotheses in batches of 64, the last one
ragged with 8) against an EXACT arg-min, without a tolerance -- the anchor tests/test_gpu_fuzz.py holds PreSync's sweep to.  The
test-variants build dumps the |residuals| the search worked on, every hypothesis of every frame against the kernel's own tile,
and the winner must be the first-wins arg-min of their lower quartile (lmeds_reference.exact_winners, np.partition on the
device's own floats); the product, which has no such code, must return the variants build's winners.  The search is the only
path on which the 24-entry contender table can overflow, so the cases are aimed there: every tile shape, ragged tiles, clusters
of near-equal quartiles (a noise-free scene), quartiles equal BIT FOR BIT (tiled tracks) with the table overflowing -- the
record counts the search asked for are read back, so the overflow is asserted, not hoped for -- and frames whose winner comes
LATE, out of the overflow path itself (the exact key of a hypothesis that found no room for a record).

Against the oracle (the first three cases): the product's winner index per frame; where it is the oracle's, M to 1e-12 and k as
in tests/test_gpu_mid_sizes.py; where it is not, the flip has to be a tie as far as fp32 rows can tell (flip_interval on the
oracle's rows, test_random_noisy_case's constants), at most max(1, 10 %) of a case's frames.  The scene seeds were chosen on the
CPU: the stand-in of tests/cpu_device (the search restated in fp32) against the oracle, flips per case --
    benchmark scene (seed 81) at 0.03: 0 of 6, at -0.17: 0 of 6; every tile shape (seed 77), noise 1e-3: 0 of 7, noise 0:
    0 of 7; ragged tiles (seed 91): 0 of 5.
Tiled frames are compared with the oracle in print only: see test_exact_ties_* below and DESIGN.md (stated differences)."""
import os

import numpy as np
import pytest

import rssync_amd
from rssync_amd import synth
from oracle import oracle as ora
from oracle.oracle import OracleProblem, sample_pair

from lmeds_reference import exact_winners, flip_interval

pytestmark = pytest.mark.gpu

SEED = 4242                          # the problems' sampler seed
STREAM = ora.STREAM_SYNC_INIT + 0    # a problem's first Sync-type call
N_HYP = 200                          # core_private.cpp:127
CONT_CAP = 24                        # kernels/lmeds.hpp: kContCap


def _fill(p, gyro, frames):
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr in frames:
        p.SetTrackResult(*fr)
    return p


def _scene(counts, seed, ids=None, **kw):
    """one frame per entry of counts (ids: 0, 1, ..), each with its own number of tracks"""
    ids = list(range(len(counts))) if ids is None else list(ids)
    gyro = synth.make_gyro(0.0, (max(ids) + 2) / synth.FPS, seed=seed)
    return gyro, [next(iter(synth.make_frames(gyro, fr, fr + 1, n, seed=seed, **kw))) for fr, n in zip(ids, counts)]


def _tiled(frames, copies):
    """every frame's tracks repeated: copies an int (t0 t1 .. t0 t1 ..: track = row mod m), or one count per track (t0 .. t0 t1 .. t1)"""
    if isinstance(copies, int):
        return [(fr, np.tile(ta, copies), np.tile(tb, copies), np.tile(ra, (copies, 1)), np.tile(rb, (copies, 1)))
                for fr, ta, tb, ra, rb in frames]
    return [(fr, np.repeat(ta, copies), np.repeat(tb, copies), np.repeat(ra, copies, axis=0), np.repeat(rb, copies, axis=0))
            for fr, ta, tb, ra, rb in frames]


def _anchor(variants_lib, gyro, frames, d0):
    """the common procedure -> dict(win: the winners, ncont: the records each frame's search asked for, res: the dump,
    M, k: the product's motion estimates)"""
    ids = [fr[0] for fr in frames]
    counts = [len(fr[1]) for fr in frames]
    assert min(counts) >= 48          # (below that the quartile sits at the hypothesis' own rows: two builds may differ)
    v = _fill(rssync_amd.SyncProblem(seed=SEED, verbose=False, _lib=variants_lib), gyro, frames)
    prod = _fill(rssync_amd.SyncProblem(seed=SEED, verbose=False), gyro, frames)
    for p in (v, prod):
        p.record_init_winners()
    v.debug_residuals(True, cap_rows=max(counts))
    v.init_motion(d0, ids[0], ids[-1])
    M, k = prod.init_motion(d0, ids[0], ids[-1])
    res = v.debug_residuals_get()
    assert res.shape == (1, len(frames), N_HYP, max(counts))
    for j, n in enumerate(counts):                                   # every row of every frame was written, nothing beyond
        assert not np.isnan(res[:, j, :, :n]).any() and np.isnan(res[:, j, :, n:]).all(), (j, n)
    ncont = v.debug_contenders_get()
    assert ncont.shape == (len(frames),)
    win_v, win_p = v.last_init_winners(), prod.last_init_winners()
    print("records asked for per frame:", ncont.tolist(), " winners:", win_v.tolist())
    np.testing.assert_array_equal(win_v, exact_winners(res, counts)[0])
    np.testing.assert_array_equal(win_p, win_v)
    return dict(win=win_p, ncont=ncont, res=res, M=M, k=k, counts=counts, ids=ids)


def _oracle(gyro, frames):
    return _fill(OracleProblem(seed=SEED, faithful=False, threads=min(os.cpu_count() or 1, 8)), gyro, frames)


def _against_oracle(gyro, frames, d0, got):
    """-> the number of frames whose winner is not the oracle's (each of them justified as a tie of fp32 rows)"""
    o = _oracle(gyro, frames)
    flips = 0
    for j, (fid, n) in enumerate(zip(got["ids"], got["counts"])):
        Mo, bh, med = o.guess_motion(fid, d0, N_HYP, STREAM)
        P = o.problem_matrix(fid, d0)
        if int(got["win"][j]) == bh:
            assert np.abs(got["M"][j] - Mo).max() < 1e-12                     # search in fp32, winner and k recomputed in fp64
            assert got["k"][j] == pytest.approx(np.clip(100 / np.linalg.norm(P @ Mo), 10, 1000), rel=1e-12)
            continue
        flips += 1
        iv = [flip_interval(P, *sample_pair(SEED, fid, STREAM, int(w), n)) for w in (got["win"][j], bh)]
        gap = max(iv[0][0], iv[1][0]) - min(iv[0][1], iv[1][1])               # > 0: the intervals do not meet
        assert gap <= 5e-3 * iv[1][2], (fid, n, int(got["win"][j]), bh, iv)
    print("winners that are not the oracle's: %d of %d" % (flips, len(frames)))
    assert flips <= max(1, 0.1 * len(frames))
    return flips


def _report_tiled(gyro, frames, d0, got, track_of):
    """tiled frames against the oracle, in print: the oracle's cross product of two copies of a track is exactly 0 and wins
    with M = 0; the device forms n_i0 x n_i1 with fma(a, b, -(b a)), for bit-equal rows the product's rounding error"""
    o = _oracle(gyro, frames)
    same_all = True
    for j, (fid, n) in enumerate(zip(got["ids"], got["counts"])):
        _, bh, med = o.guess_motion(fid, d0, N_HYP, STREAM)
        i0, i1 = sample_pair(SEED, fid, STREAM, int(got["win"][j]), n)
        same = track_of(i0) == track_of(i1)
        same_all &= same
        print("frame %d: device winner %d (%s pair, |M| = %.3g), oracle's %d (quartile %.3g)"
              % (fid, int(got["win"][j]), "a same-track" if same else "a two-track", np.linalg.norm(got["M"][j]), bh, med))
    return same_all


@pytest.fixture(scope="module")
def bench_scene(built):
    gyro = synth.make_gyro(0.0, (6 + 2) / synth.FPS, seed=81)          # tests/test_gpu_eager_bound.py's scene
    return gyro, list(synth.make_frames(gyro, 0, 6, 2048, seed=81))


@pytest.mark.parametrize("d0", [0.03, -0.17])
def test_benchmark_instantiation(variants_lib, bench_scene, d0):
    """6 x 2048 tracks: eight rows per thread, the benchmark's shape; at a start like Sync's, and at a delay far from the truth"""
    gyro, frames = bench_scene
    got = _anchor(variants_lib, gyro, frames, d0)
    _against_oracle(gyro, frames, d0, got)


@pytest.mark.parametrize("noise", [1e-3, 0.0])
def test_every_tile_shape_in_one_problem(variants_lib, noise):
    """4 / 8 / 16 / 24 rows per thread and the eight-wave shape; without noise and outliers the inliers' residuals vanish at the
    true delay and the quartiles of the hypotheses drawn from inliers lie close together 7 ms from it"""
    kw = dict(noise=0.0, outliers=0.0) if noise == 0.0 else dict(noise=noise)
    gyro, frames = _scene([520, 900, 2000, 3500, 6000, 7000, 8192], seed=77, **kw)
    got = _anchor(variants_lib, gyro, frames, 0.03)
    _against_oracle(gyro, frames, 0.03, got)


def test_ragged_tiles(variants_lib):
    """one row into a tile's second wave, one short of and one past the 2048-row tile, and sizes that fill no thread evenly"""
    gyro, frames = _scene([513, 1000, 2047, 2049, 3000], seed=91)
    got = _anchor(variants_lib, gyro, frames, 0.03)
    _against_oracle(gyro, frames, 0.03, got)


def test_one_wave_frames(variants_lib):
    """the one-wave kernel's sequential search (at most 512 tracks; it shares the dump, not the eager bound), beside one tile"""
    gyro, frames = _scene([48, 130, 257, 400, 512, 600], seed=92)
    got = _anchor(variants_lib, gyro, frames, 0.03)
    assert (got["ncont"][:5] == 0).all() and got["ncont"][5] > 0      # (records are the tile kernel's)


def test_exact_ties_at_the_benchmark_tile_size(variants_lib):
    """128 tracks x 16: pairs that are copies of each other give the same direction and the same quartile bit for bit, a few at
    a time -- the table does not overflow; the earliest hypothesis of the best quartile wins (core_private.cpp:53, strict <)"""
    gyro, base = _scene([128] * 6, seed=83)
    frames = _tiled(base, 16)
    got = _anchor(variants_lib, gyro, frames, 0.03)
    _report_tiled(gyro, frames, 0.03, got, lambda i: i % 128)


def test_exact_ties_with_the_record_table_overflowing(variants_lib):
    """3 tracks x 682 (2046 rows) and 4 tracks x 512: a third / a quarter of the 200 hypotheses pair two copies of ONE track, and
    all pairs of one track give the same direction -- the rounding residue of a x a -- and so the same quartile, bit for bit; so do
    the pairs of two given tracks in a given order (tests/test_lmeds_reference_cpu.py: the census).  Each member of the class
    that is best at the time asks for a record: more than the table's 24.  That these quartiles are rounding noise does not
    matter: the anchor is on the device's own floats; the first-wins rule over dozens of bit-equal quartiles is what is tested."""
    for m, copies, track_seed in ((3, 682, 87), (4, 512, 83)):
        # (the track seed of the three-track frames: of 83 .. 94 the one whose frames ask for most records on the device, 35 and 36
        # on two of the six -- which track's residue is smallest is the device's rounding, the census only says how many pairs)
        gyro, base = _scene([m] * 6, seed=track_seed)
        frames = _tiled(base, copies)
        got = _anchor(variants_lib, gyro, frames, 0.03)
        if m == 3:
            assert got["ncont"].max() > CONT_CAP, got["ncont"]       # the overflow path (s_exact, the decision's ovf terms) ran
        _report_tiled(gyro, frames, 0.03, got, lambda i: i % m)


# frames of TWO tracks, 1800 copies of A then 248 of B (2048 rows): 77 % of the hypotheses pair two copies of A (one quartile, bit
# for bit), 1.5 % two copies of B.  The frame ids are those (of 0 .. 20, seed 4242) whose first B-B pair comes after 30 or more
# A-A pairs: by then the table is full, so where B's quartile is the smaller one -- the device's rounding decides, either is as
# likely -- the WINNER is a hypothesis that found no room for a record and was closed at once: the key in s_exact alone, all 24
# records dead.  (In the other frames, and in every other case of this file, the winner is one of the first records, and a wrong
# decision about the overflowed keys would go unseen.)
LATE_IDS = [0, 7, 9, 11, 13, 14, 17, 20]
LATE_COPIES = (1800, 248)


def late_winner_census(ids=range(40), n_a=LATE_COPIES[0], n=sum(LATE_COPIES)):
    """-> {frame id: (index of the first B-B pair, A-A pairs before it)} for the ids that have a B-B pair"""
    out = {}
    for f in ids:
        aa = 0
        for h in range(N_HYP):
            i0, i1 = sample_pair(SEED, f, STREAM, h, n)
            if i0 >= n_a and i1 >= n_a:
                out[f] = (h, aa)
                break
            aa += int(i0 < n_a and i1 < n_a)
    return out


def test_a_winner_out_of_the_overflow_path(variants_lib):
    census = late_winner_census(LATE_IDS)
    assert all(f in census and census[f][1] >= 30 for f in LATE_IDS), census
    gyro, base = _scene([2] * len(LATE_IDS), seed=83, ids=LATE_IDS)
    frames = _tiled(base, list(LATE_COPIES))
    got = _anchor(variants_lib, gyro, frames, 0.03)
    # frames whose winner is the first B-B pair, with more than 24 records asked for before it could ask
    late = [f for j, f in enumerate(LATE_IDS) if int(got["win"][j]) == census[f][0] and got["ncont"][j] > CONT_CAP]
    print("frames whose winner came out of the overflow path:", late)
    assert late, (got["win"].tolist(), got["ncont"].tolist(), census)
    _report_tiled(gyro, frames, 0.03, got, lambda i: int(i >= LATE_COPIES[0]))
