"""The corner detector on the device (csrc/kernels/features.hpp: corner_cell_kernel, corner_select_kernel) where its tie
rule decides -- "p beats q iff R(p) > R(q), or they are equal and p's raster index is smaller" (include/rssync_features.h)
-- and at the edges of its layout and range: sliver cells, cells without a positive response, quality 1.0 and T = 1,
responses above 2^48, the select kernel's 256-cell rounds, an empty frame inside a batch.  Bit for bit against the numpy
restatement (tests/feature_reference.py) on the inputs of tests/feature_cases.py; tests/test_features_cpu.py shows from
the restatement alone that those inputs hold the ties and edges they are here for.

Which test reaches which path of the two kernels:

  the strict / non-strict split of the eight comparisons   test_ties_in_the_suppression_and_in_the_cell_winner, ::test_ties_in_a_pitched_view
                                                           (thousands of plateau pixels, both raster orders of every tie)
  corner_beats in a thread's own rows                      the same, at cells 64 and 128 (tied bests in one column of one band)
  the 64-lane shuffle butterfly                            the same, every frame (tied bests in two lanes of one wave)
  the four-wave reduction through LDS                      the same, every frame (tied bests in two waves)
  best_r >= T, T = R_max                                   test_quality_one_keeps_exactly_the_ties_for_the_maximum,
                                                           test_full_range_of_the_response_and_of_the_threshold (quality 1.0)
  T = 1                                                    test_full_range_... (quality 1e-18), test_compaction_rounds,
                                                           test_cells_without_a_positive_response_in_a_textured_frame
  R above 2^48                                             test_full_range_...[9]
  cw = 1 (85 bands of 1 and 2 rows)                        test_sliver_cells, e = 1 and "width+1" (cells 16 and 128)
  a cell without a valid pixel (best_idx = -1)             test_sliver_cells, e = 1 and e = b
  a cell with one valid column or row                      test_sliver_cells, e = b + 1
  cells whose largest R is 0 or negative                   test_cells_without_a_positive_response_in_a_textured_frame
  the select kernel's 256-cell round boundary              test_compaction_rounds (255, 256 and 272 kept cells)
  a pair with a count of zero inside a batch               test_a_pair_without_features_between_pairs_with_many

Each of these one-line changes to features.hpp fails the file: `R >= mid[t + 1]` to `>` (17 of the 20 tests fail: all but
test_full_range_...[7], test_sliver_cells[128-3] and the repeatability test), `ip < iq` to `ip > iq` in corner_beats (19:
all but the repeatability test), `>= T` to `> T` in corner_select_kernel (10: the four tie frames, the pitched view,
quality one, the four full-range blocks)."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import feature_cases as fc
import feature_reference as fr

pytestmark = pytest.mark.gpu


def _problem():
    import rssync_amd
    return rssync_amd.SyncProblem(seed=321)


def _levels(frames):
    """the default four pyramid levels where the frame has room for them (2^L + 1 px on each side), fewer below that"""
    return min(4, int(np.log2(min(frames.shape[1:]) - 1)))


def _raw(p, frames, cell, block, quality):
    from rssync_amd import features
    return features.raw_features(p, frames, cell=cell, block=block, quality=quality, levels=_levels(frames))


def _check(p, frames, cell, block, quality, what=""):
    """the detector's lists of every a-side frame (0 .. n - 2) against the reference -> counts, points"""
    cnt, pts, *_ = _raw(p, frames, cell, block, quality)
    for k in range(len(frames) - 1):
        want = fc.detect(frames[k], cell, block, quality)
        msg = "%s frame %d of %dx%d, cell %d block %d quality %g" % (what, k, frames.shape[2], frames.shape[1], cell, block, quality)
        assert cnt[k] == len(want), msg
        np.testing.assert_array_equal(pts[k, :cnt[k]], want, err_msg=msg)
    return cnt, pts


def _both_orders(K):
    """[K, K turned by 180 degrees, K]: the same responses with the raster order of every tie reversed"""
    return np.stack([K, K[::-1, ::-1], K])


@pytest.mark.parametrize("h,w,P,seed", fc.TIE_FRAMES)
def test_ties_in_the_suppression_and_in_the_cell_winner(built, h, w, P, seed):
    p = _problem()
    frames = _both_orders(fc.kaleidoscope(h, w, P, seed))
    for cell, block, quality in fc.TIE_CONFIGS:
        _check(p, frames, cell, block, quality)


def test_ties_in_a_pitched_view(built):
    h, w, P, seed = fc.PITCHED
    wide = np.random.default_rng(3).integers(0, 256, size=(3, h, w + 45), dtype=np.uint8)
    wide[:, :, 7:7 + w] = _both_orders(fc.kaleidoscope(h, w, P, seed))
    frames = wide[:, :, 7:7 + w]                                       # pitch > width
    assert not frames.flags["C_CONTIGUOUS"]
    p = _problem()
    for cell, block, quality in fc.TIE_CONFIGS:
        _check(p, frames, cell, block, quality, "pitched")


def test_quality_one_keeps_exactly_the_ties_for_the_maximum(built):
    """T = R_max: every listed point has the frame's largest response, more than one cell has one, cells in order; the
    public door with quality=1.0 (the top of its range) hands out the same points as doubles"""
    p = _problem()
    for h, w, P, seed in fc.TIE_FRAMES:
        frames = _both_orders(fc.kaleidoscope(h, w, P, seed))
        for cell, block, quality in fc.TIE_CONFIGS:
            if quality != 1.0 or (cell >= h and cell >= w):            # (one cell: one feature)
                continue
            cnt, pts = _check(p, frames, cell, block, 1.0)
            f = p.track_features(frames, cell=cell, block=block, quality=1.0)
            ncy = -(-h // cell)
            for k in range(2):
                R = fr.response(frames[k], block)
                got = pts[k, :cnt[k]]
                assert cnt[k] > 1, (h, w, cell, block)
                assert (R[got[:, 1], got[:, 0]] == R.max()).all()
                cid = got[:, 0] // cell * ncy + got[:, 1] // cell
                assert (np.diff(cid) > 0).all(), cid
                assert f.counts[k] == cnt[k] and f.points_a.dtype == np.float64
                np.testing.assert_array_equal(f.points_a[k, :cnt[k]], fc.detect(frames[k], cell, block, 1.0).astype(np.float64))


@pytest.mark.parametrize("block", fc.RANGE_BLOCKS)
def test_full_range_of_the_response_and_of_the_threshold(built, block):
    """a 0/255 pattern (R_max up to 2^48.9 at block 9) at quality 1.0, in between, and so small that T = 1"""
    img = fc.range_frame()
    frames = _both_orders(img)
    R = fr.response(img, block)
    assert fr.threshold(R, 1e-18) == 1 and fr.threshold(R, 1.0) == R.max()
    p = _problem()
    for cell in fc.RANGE_CELLS:
        for quality in fc.RANGE_QUALITIES:
            cnt, _ = _check(p, frames, cell, block, quality)
            assert cnt[0] > 1


@pytest.mark.parametrize("block", fc.SLIVER_BLOCKS)
@pytest.mark.parametrize("cell", fc.SLIVER_CELLS)
def test_sliver_cells(built, cell, block):
    """a last column and row of cells 1, b and b + 1 px wide: without a valid pixel (twice), then with exactly one valid
    column or row; 1 px in width only (cw = 1 beside full-height cells: 85 bands of 1 or 2 rows) and in height only"""
    p = _problem()
    for h, w, what in fc.sliver_sizes(cell, block):
        img = fc.sliver_frame(h, w)
        cnt, pts = _check(p, _both_orders(img), cell, block, fc.SLIVER_QUALITY, what)
        n = fc.cell_counts(pts[0, :cnt[0]].astype(np.int64), h, w, cell)
        b = block // 2 + 1
        if what == "e=%d" % (b + 1):
            assert n[-1].sum() >= 1 and n[:, -1].sum() >= 1
        else:
            assert w % cell == 0 or n[-1].sum() == 0
            assert h % cell == 0 or n[:, -1].sum() == 0


def test_cells_without_a_positive_response_in_a_textured_frame(built):
    """a constant rectangle (R = 0 on a plateau of thousands of pixels) and a ramp (R < 0) inside texture: equal to the
    reference, and nothing listed strictly inside the rectangle"""
    img = fc.patch_frame()
    p = _problem()
    y0, y1, x0, x1 = fc.PATCH_FLAT
    m = fc.PATCH_BLOCK // 2 + 1
    for quality in fc.PATCH_QUALITIES:
        cnt, pts = _check(p, _both_orders(img), fc.PATCH_CELL, fc.PATCH_BLOCK, quality)
        x, y = pts[0, :cnt[0], 0], pts[0, :cnt[0], 1]
        assert 0 < cnt[0] < pts.shape[1]
        assert not ((x >= x0 + m) & (x < x1 - m) & (y >= y0 + m) & (y < y1 - m)).any()


@pytest.mark.parametrize("h,w", fc.ROUND_FRAMES)
def test_compaction_rounds(built, h, w):
    """255, 256 and 272 cells, every one kept: an exactly full round of the select kernel's 256 threads, one short of it,
    and a round boundary inside the list"""
    img = fc.round_frame(h, w)
    cnt, pts = _check(_problem(), _both_orders(img), fc.ROUND_CELL, fc.ROUND_BLOCK, fc.ROUND_QUALITY)
    assert cnt[0] == cnt[1] == pts.shape[1] == (h // fc.ROUND_CELL) * (w // fc.ROUND_CELL)


def test_a_pair_without_features_between_pairs_with_many(built):
    """[K, flat, K, K']: the middle pair lists nothing, and its neighbours' results are those of the two-frame calls (the
    forward pass into a flat frame is chaotic, so only the device's own batch independence is asserted for it)"""
    from rssync_amd import synth, synth_video as sv
    frames = fc.mixed_frames()
    cell, block, quality = fc.MIXED_CONFIG
    p = _problem()
    four = _raw(p, frames, cell, block, quality)
    n_ref = len(fc.detect(frames[0], cell, block, quality))
    assert n_ref > 100 and list(four[0]) == [n_ref, 0, n_ref]
    for k in (0, 2):
        np.testing.assert_array_equal(four[1][k, :n_ref], fc.detect(frames[k], cell, block, quality))
        two = _raw(_problem(), frames[k:k + 2], cell, block, quality)
        assert two[0][0] == n_ref
        for name, g, t in zip(("points", "flow_fwd", "flow_bwd", "status", "fb_error"), four[1:], two[1:]):
            np.testing.assert_array_equal(g[k, :n_ref], t[0, :n_ref], err_msg="pair %d %s" % (k, name))
    st = four[4]
    kept = np.array([(st[k, :four[0][k]] == 0).sum() for k in range(3)])
    print("kept tracks per pair:", kept)
    # the hand-over (tests/test_gpu_features.py::test_pairs_below_min_tracks_are_skipped): an earlier frame at every index
    first, m = 30, 8
    gyro = synth.make_gyro(1.0, 1.0 + (len(frames) + 2) / synth.FPS, seed=77)
    times = np.arange(first, first + len(frames)) / synth.FPS
    lens = sv.half_lens()
    q = _problem()
    q.set_gyro_rates(gyro.times, gyro.rates)
    old = np.array([[100.0, 100.0], [200.0, 150.0], [300.0, 50.0]])
    for k in range(3):
        q.set_track_pixels(first + k, times[k], times[k + 1], old, old + 1.0, lens, frames.shape[1])
    before = [q.frame_rays(first + k) for k in range(3)]
    n_set = q.features_frames(frames, times, lens, first_frame=first, cell=cell, block=block, quality=quality, min_tracks=m)
    assert kept[1] == 0 and kept[2] >= m, kept
    assert n_set == (kept >= m).sum()
    for k in range(3):
        ra, rb = q.frame_rays(first + k)
        if kept[k] >= m:
            assert ra.shape[0] == kept[k]
        else:
            np.testing.assert_array_equal(ra, before[k][0])
            np.testing.assert_array_equal(rb, before[k][1])


def test_repeatable_on_one_problem_and_on_a_fresh_one(built):
    h, w, P, seed = fc.TIE_FRAMES[0]
    frames = _both_orders(fc.kaleidoscope(h, w, P, seed))
    cell, block, quality = fc.TIE_CONFIGS[0]
    p = _problem()
    a = _raw(p, frames, cell, block, quality)
    b = _raw(p, frames, cell, block, quality)
    c = _raw(_problem(), frames, cell, block, quality)
    assert a[0][0] > 100
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[0], c[0])
    for k, n in enumerate(a[0]):                                       # (the slots past a pair's count are not set)
        for x, y, z in zip(a[1:], b[1:], c[1:]):
            np.testing.assert_array_equal(x[k, :n], y[k, :n])
            np.testing.assert_array_equal(x[k, :n], z[k, :n])
