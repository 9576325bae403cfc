"""The tile kernel's EAGER BOUND (kernels/lmeds.hpp, round 8): the waves of a workgroup read the bound after their sweep,
publish every upper end a counting pass lowers at once, and abandon a narrowing whose lower end has reached the bound.
Which hypotheses end as records now depends on how the four waves interleave -- the WINNER must not: it stays the exact
arg-min of (quartile, index), so against round 2's exact selection of every quartile (the test-variants build,
tests/test_gpu_lazy_select.py) best_h, the per-frame costs and the curve are identical bit for bit, and so is PreSync's
return.  The cases are the ones where the protocol could go wrong: the first candidate of a chunk (no provisional bound),
a ragged last chunk, clusters of near-equal quartiles, quartiles equal BIT FOR BIT at the benchmark's tile size (an abandon
rule with > in place of >=, or an inclusive bound, would drop the earlier hypothesis), the smallest shape with the early
rejection, 16 rows per thread, and GuessMotion's 200-hypothesis search, whose record table can overflow.

GuessMotion's search (MODE 1) has no exact-selection KERNEL to be compared with; its anchor is the dump of its own residuals,
tests/test_gpu_guess_motion.py: the winner is the exact first-wins arg-min of the lower quartile, table overflow included.
Here three runs of the product are compared with each other."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _problem(seed, lib=None, env=None, **kw):
    import rssync_amd
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return rssync_amd.SyncProblem(seed=seed, **kw) if lib is None else rssync_amd.SyncProblem(seed=seed, _lib=lib, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fill(p, gyro, frames):
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr in frames:
        p.SetTrackResult(*fr)
    return p


def _scene(F, N, seed, **kw):
    from rssync_amd import synth
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=seed)
    return gyro, list(synth.make_frames(gyro, 0, F, N, seed=seed, **kw))


def _tiled(frames, copies):
    return [(fr, np.tile(ta, copies), np.tile(tb, copies), np.tile(ra, (copies, 1)), np.tile(rb, (copies, 1)))
            for fr, ta, tb, ra, rb in frames]


def _compare(variants_lib, gyro, frames, step, radius, shape, own_shape=False):
    """product against exact selection: winners, per-frame costs and curve as bits, PreSync's return; -> the product's curve"""
    F = len(frames)
    lazy = _fill(_problem(4242, env={"RSSYNC_NO_SUBSHAPES": "1"} if own_shape else None), gyro, frames)
    exact = _fill(_problem(4242, lib=variants_lib, env={"RSSYNC_K2_EXACT_SELECT": "1"}), gyro, frames)
    dl, cl, fl, bl = lazy.presync_curve(0.0, 0, F, step, radius, per_frame=F)
    assert shape in lazy.lmeds_shapes(), lazy.lmeds_shapes()       # (rows / 256 of the tile: the instantiation meant ran)
    de, ce, fe, be = exact.presync_curve(0.0, 0, F, step, radius, per_frame=F)
    assert len(dl) == len(de) and bl.shape == be.shape and (bl >= 0).all()
    np.testing.assert_array_equal(bl, be)
    np.testing.assert_array_equal(fl.view(np.uint64), fe.view(np.uint64))
    np.testing.assert_array_equal(cl.view(np.uint64), ce.view(np.uint64))
    assert lazy.PreSync(0.0, 0, F, step, radius) == exact.PreSync(0.0, 0, F, step, radius)
    return lazy, (dl, cl, fl, bl)


@pytest.fixture(scope="module")
def bench_scene(built):
    return _scene(6, 2048, seed=81)


def test_benchmark_instantiation_three_chunks_the_last_ragged(built, variants_lib, bench_scene):
    gyro, frames = bench_scene
    _, (d, _, _, _) = _compare(variants_lib, gyro, frames, 0.001, 0.035, shape=8)
    assert 64 < len(d) < 96 and len(d) % 32 != 0, len(d)             # three chunks of up to 32 candidates, the last one ragged


def test_noise_free_scene_near_equal_quartiles(built, variants_lib):
    gyro, frames = _scene(6, 2048, seed=82, noise=0.0, outliers=0.0)
    _compare(variants_lib, gyro, frames, 0.001, 0.035, shape=8)


def test_equal_quartiles_at_the_benchmark_tile_size_go_to_the_earlier_hypothesis(built, variants_lib):
    """128 tracks tiled 16 times: row pairs that are copies of each other give the same direction and the same quartile, bit
    for bit; the earlier hypothesis wins under both selections (core_private.cpp:53, strict <)"""
    gyro, frames = _scene(6, 128, seed=83)
    tiled = _tiled(frames, 16)
    assert len(tiled[0][1]) == 2048
    _compare(variants_lib, gyro, tiled, 0.001, 0.035, shape=8)


@pytest.mark.parametrize("F,N,shape,own_shape", [
    (8, 1000, 4, False),       # 16 residual registers: the smallest shape with the early-rejection path
    (4, 3000, 12, False),      # as the product sweeps it: the 3072-row sub-shape
    (4, 3000, 16, True),       # 16 rows per thread, the class's own shape
])
def test_other_shapes(built, variants_lib, F, N, shape, own_shape):
    gyro, frames = _scene(F, N, seed=84 + N)
    _compare(variants_lib, gyro, frames, 0.001, 0.035, shape=shape, own_shape=own_shape)


def test_guess_motion_search_is_repeatable(built, bench_scene):
    """Sync's start: GuessMotion's 200 hypotheses per frame in batches of 64 (MODE 1 of the tile kernel).  That each winner
    is the exact arg-min is tests/test_gpu_guess_motion.py's; here three runs of the product are compared with each other: the
    same trace bits, the same return."""
    gyro, frames = bench_scene
    F = len(frames)
    runs = []
    for _ in range(3):
        p = _fill(_problem(4242, max_outer_iters=2), gyro, frames)
        ret = p.Sync(0.03, 0, F - 1, 0.0, 0.1)
        runs.append((ret, np.array(p.sync_trace(), dtype=np.float64).copy()))
    assert len(runs[0][1]) > 0 and np.isfinite(runs[0][0]).all()
    for ret, tr in runs[1:]:
        assert ret == runs[0][0]
        np.testing.assert_array_equal(tr.view(np.uint64), runs[0][1].view(np.uint64))


def test_the_curve_is_repeatable(built, bench_scene):
    """which hypotheses are recorded depends on timing; per-frame costs and winners may not"""
    gyro, frames = bench_scene
    F = len(frames)
    p = _fill(_problem(4242), gyro, frames)
    first = p.presync_curve(0.0, 0, F, 0.001, 0.035, per_frame=F)
    for _ in range(2):
        again = p.presync_curve(0.0, 0, F, 0.001, 0.035, per_frame=F)
        np.testing.assert_array_equal(again[3], first[3])
        np.testing.assert_array_equal(again[2].view(np.uint64), first[2].view(np.uint64))
        np.testing.assert_array_equal(again[1].view(np.uint64), first[1].view(np.uint64))
