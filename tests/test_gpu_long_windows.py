"""Window sums of LONG windows on every single-device route of Sync and PreSync, bit for bit.

A window's loss, derivative, line-search trials and PreSync costs are sums over its frames in one association (chunks at
the multiples of 64 of the frame table, a chunk in slot order, the chunks in order: kernels/support.hpp:7-18), which the
device implements three times, each with another branch for a window too long for its staging area:

  plan_sum_kernel    kernels/support.hpp:19-56   host loop, rssync_ext_loss, PreSync: a thread takes a second chunk beyond
                                                 64 chunks; `idx` for overlapping PreSync windows
  window_sums        kernels/syncloop.hpp:81-143 the chain of launches: staged in LDS while rows * span <= 2048
                                                 (204 / 205 slots with the 10 trial rows, 1024 / 1025 with the 2 rows of
                                                 loss + derivative), else from global memory (:108-123)
  exec_window_sums   kernels/executor.hpp:239-265 the window executor: staged while rows * n_slots <= 1280 (128 / 129
                                                 slots with 10 rows, 640 / 641 with 2, 1280 / 1281 with 1), else one
                                                 cache-bypassing load per addition (:259)

The references are the association restated in numpy (tests/window_sum_reference.py) on the device's own per-frame
values, and the CPU stand-in of the device ABI, which tests/test_window_sums_cpu.py ties to that restatement.  Every
comparison prints what it measured before it asserts.
"""
import os

import numpy as np
import pytest

import window_sum_reference as ws

pytestmark = pytest.mark.gpu

SEED = 123
D0 = ws.LOSS_DELAYS[0]


def _device(scene=None, chain=False, host_loop=False, **kw):
    import rssync_amd
    if chain:
        os.environ["RSSYNC_EXECUTOR"] = "0"       # read when a problem is created
    try:
        p = rssync_amd.SyncProblem(**kw)
    finally:
        if chain:
            del os.environ["RSSYNC_EXECUTOR"]
    if host_loop:
        p.set_host_loop(True)
    if scene is not None:
        scene.fill(p)
    return p


def _same_bits(what, ref_name, ref, others):
    """print how every route's values differ from the first route's, then require that none does"""
    ref = np.ascontiguousarray(ref, np.float64)
    bad = []
    for name, x in others:
        x = np.ascontiguousarray(x, np.float64)
        if x.shape != ref.shape:
            print("%s: %s has shape %r, %s %r" % (what, name, x.shape, ref_name, ref.shape))
            bad.append(name)
            continue
        n = int(np.sum(ws.bits(x) != ws.bits(ref)))
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(x - ref))) if x.size else 0.0
        print("%s: %s differs from %s in %d of %d values, max |difference| %.3g" % (what, name, ref_name, n, x.size, worst))
        if n:
            bad.append(name)
    assert not bad, "%s: %s differ(s) from %s" % (what, ", ".join(bad), ref_name)


def _run_routes(hosttest_lib, scene, call, trace, routes=("executor", "chain", "host loop", "stand-in"), **kw):
    """`call` on fresh objects with the same seed on every route -> {route: (result, traces)} and the executor object.
    The stand-in starts from the chain's GuessMotion winners (its own fp32 search is sequential IEEE and may fall the other
    way on a near-tie: tests/test_gpu_bitexact.py)."""
    import rssync_amd
    out, winners, ex = {}, None, None
    for name in routes:
        if name == "stand-in":
            p = rssync_amd.SyncProblem(_lib=hosttest_lib, **kw)
            scene.fill(p)
            p.set_init_override(winners)
        else:
            p = _device(scene, chain=name == "chain", host_loop=name == "host loop", **kw)
            if name == "chain":
                p.record_init_winners()       # (recording keeps a problem out of the executor: only the chain records)
        out[name] = (call(p), trace(p))
        if name == "chain":
            winners = p.last_init_winners()
        if name == "executor":
            ex = p
    return out, ex


def _compare_routes(what, out):
    names = list(out)
    first = names[0]
    res = {n: np.concatenate([np.ravel(x) for x in out[n][0]]) for n in names}
    _same_bits(what + ", returned (cost, delay)", first, res[first], [(n, res[n]) for n in names[1:]])
    for w in range(len(out[first][1])):
        _same_bits(what + ", trace of window %d (%d rows)" % (w, len(out[first][1][w])), first, out[first][1][w],
                   [(n, out[n][1][w]) for n in names[1:]])


def _sync_one(hosttest_lib, scene, begin, length, **kw):
    out, ex = _run_routes(hosttest_lib, scene, lambda p: p.Sync(D0, begin, begin + length - 1, 0.0, 0.1),
                          lambda p: [p.sync_trace()], **kw)
    assert len(out["executor"][1][0]) >= 3
    _compare_routes("Sync of %d frames from %d" % (length, begin), out)
    st = ex.executor_stats()
    print("executor:", st)
    assert st["runs"] > 0, st
    return out


# ---- (a) loss and derivative against the numpy association, on the device's own per-frame values --------------------

@pytest.fixture(scope="module")
def per_frame(built):
    """4300 frames of a uniform 16 tracks (a selection's kernel instantiation follows its largest frame: a frame evaluated
    alone must run the instantiation it runs inside the window); motions once from the whole range, every frame alone once"""
    scene = ws.uniform_scene(4300, 16)
    p = _device(scene, seed=SEED)
    M, k = p.init_motion(D0, 0, scene.F - 1)
    return (p, M, k) + ws.per_frame_values(p, M, k, D0, range(scene.F))


@pytest.mark.parametrize("b,n", ws.GPU_LOSS_WINDOWS)
def test_window_loss_is_the_plan_order_sum_of_the_frames_alone(per_frame, b, n):
    """plan_sum_kernel (kernels/support.hpp:19-56) behind rssync_ext_loss: loss and derivative at two delays and the
    five-delay batch of a window are plan_sum (tests/window_sum_reference.py) of the values the device gives each frame
    alone, in every bit.  65: two chunks; 129 .. 1281 from 37 or 5: ragged first chunks, chunk tails other than a multiple
    of 8 (:32-39), 3 .. 21 chunks, thread 0's groups of 16 chunk sums with a tail (:46-53); 4161 from 0 and 4200 from 100:
    66 and 67 chunks, more than the block's 64 threads, so threads 0 .. 2 take a second chunk (:28)."""
    p, M, k, L, G, B = per_frame
    Lw, Gw, Bw = ws.window_values(p, M, k, D0, b, n)
    for name, got, per in (("loss", Lw, L), ("derivative", Gw, G), ("five-delay batch", Bw, B)):
        want = ws.plan_sums(per, b, n)
        flat = np.array([ws.flat_sum(per[b:b + n, c]) for c in range(per.shape[1])])
        print("window (%d, %d) %s: device - plan_sum %r, device - flat sum %r" % (b, n, name, (got - want).tolist(), (got - flat).tolist()))
    for name, got, per in (("loss", Lw, L), ("derivative", Gw, G), ("five-delay batch", Bw, B)):
        np.testing.assert_array_equal(ws.bits(got), ws.bits(ws.plan_sums(per, b, n)), err_msg=name)


# ---- (b) PreSync -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def presync_problem(built):
    return _device(ws.uniform_scene(4300, 8), seed=SEED)


@pytest.mark.parametrize("b,n", ws.PRESYNC_WINDOWS)
def test_presync_curve_is_the_plan_order_sum_of_the_frame_costs(presync_problem, b, n):
    """plan_sum_kernel (kernels/support.hpp:19-56) behind PreSync: every candidate's cost is plan_sum of the per-frame
    costs of the same sweep -- 129 frames from 37 (three chunks), 4161 from 0 (66 chunks: a second chunk for threads 0
    and 1, :28) and 4200 from 100 (67 chunks, ragged at both ends)"""
    d0, step, radius = ws.PRESYNC_ARGS
    d, curve, per, _ = presync_problem.presync_curve(d0, b, b + n, step, radius, per_frame=n)
    assert per.shape == (len(d), n) and len(d) >= 5
    want = np.array([ws.plan_sum(per[c], b) for c in range(len(d))])
    print("PreSync window (%d, %d): curve - plan_sum %r, curve - flat sum %r" % (
        b, n, (curve - want).tolist(), [float(curve[c] - ws.flat_sum(per[c])) for c in range(len(d))]))
    np.testing.assert_array_equal(ws.bits(curve), ws.bits(want))


def test_batched_presync_on_overlapping_long_windows_is_the_single_calls(built):
    """plan_sum_kernel with a non-null `idx` (kernels/support.hpp:35,39: overlapping windows, a frame has a position in
    several of them) and 66 chunks in the first window: pre_sync_windows returns, per window, the bits of a single PreSync
    call on that window (idx == NULL) -- 4161, 129, 641 and 1281 frames"""
    scene = ws.uniform_scene(4300, 8)
    d0, step, radius = ws.PRESYNC_ARGS
    c, d = _device(scene, seed=SEED).pre_sync_windows(d0, ws.PRESYNC_BATCH_BEGINS, ws.PRESYNC_BATCH_ENDS, step, radius)
    single = _device(scene, seed=SEED)
    one = [single.PreSync(d0, b, e, step, radius) for b, e in zip(ws.PRESYNC_BATCH_BEGINS, ws.PRESYNC_BATCH_ENDS)]
    _same_bits("batched PreSync, costs", "single calls", [r[0] for r in one], [("batched", c)])
    _same_bits("batched PreSync, delays", "single calls", [r[1] for r in one], [("batched", d)])


# ---- (c) one long Sync window on four routes ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", ws.SYNC_LENGTHS)
def test_one_long_sync_window_on_four_routes(hosttest_lib, n):
    """One window from frame 37 (a ragged first chunk), frames of 2 .. 40 tracks and a 130-track frame every 16th, six
    iterations: executor == chain of launches == host loop == stand-in in every trace row, cost and delay.
    129: exec_window_sums un-staged with the 10 trial rows (kernels/executor.hpp:243,259; 10 * 129 > 1280).
    205: window_sums un-staged with the 10 trial rows (kernels/syncloop.hpp:87,108-123; 10 * 205 > 2048).
    641: exec_window_sums un-staged with the 2 rows of loss + derivative as well.
    1025: window_sums un-staged with 2 rows as well.
    1281: exec_window_sums un-staged with the 1 row of the final loss as well; 21 chunks: window_sums' groups of 16 chunk
    sums with a tail (kernels/syncloop.hpp:132-139)."""
    _sync_one(hosttest_lib, ws.ragged_scene(), ws.SYNC_BEGIN, n, seed=SEED, max_outer_iters=6)


def test_long_sync_window_whose_searches_wait_for_their_later_trials(hosttest_lib, monkeypatch):
    """641 frames with RSSYNC_LOOP_FIRST_TRIALS=1: a line search gets its first trial only, waits an iteration for the
    rest, and the trial rows are summed under a PARTIAL mask -- exec_window_sums un-staged with some of the 10 rows
    switched off (kernels/executor.hpp:253,259), window_sums un-staged (kernels/syncloop.hpp:108-123)"""
    monkeypatch.setenv("RSSYNC_LOOP_FIRST_TRIALS", "1")
    out = _sync_one(hosttest_lib, ws.ragged_scene(), ws.SYNC_BEGIN, 641, seed=SEED, max_outer_iters=6)
    assert out["executor"][1][0][:, 5].max() > 1      # (a search did need more than its first trial)


def test_sync_window_of_more_than_64_chunks_on_four_routes(hosttest_lib):
    """4161 frames of 8 tracks from index 0, four iterations: 65 full chunks and one slot.  The host loop's
    plan_sum_kernel gives threads 0 and 1 a second chunk and adds 4 x 16 + 2 chunk sums (kernels/support.hpp:28,46-53);
    window_sums adds 66 chunk sums in groups of 16 (kernels/syncloop.hpp:132-139) and is un-staged at 10 and 2 rows;
    exec_window_sums is un-staged at 10, 2 and 1 rows (kernels/executor.hpp:259)"""
    _sync_one(hosttest_lib, ws.uniform_scene(4300, 8), 0, 4161, seed=SEED, max_outer_iters=4)


# ---- (d) staged and un-staged windows in one call ----------------------------------------------------------------------

def test_staged_and_unstaged_windows_in_one_call(hosttest_lib):
    """sync_windows on five overlapping windows of 40, 129, 641, 1281 and 661 frames, seven iterations at most, from
    delays spread over 0.034 .. 0.039 so that they stop at different iterations: every window takes its own branch of
    exec_window_sums (kernels/executor.hpp:243: staged at 40 slots; un-staged at 10 rows from 129, at 2 from 641, at 1
    from 1281) and of window_sums (kernels/syncloop.hpp:87: staged at 40 and 129, un-staged at 10 rows from 641 on and
    at 2 rows at 1281) in the same launch.  Executor == chain == host loop == stand-in."""
    b, e = ws.SYNC_BATCH_BEGINS, ws.SYNC_BATCH_ENDS
    d0 = np.linspace(0.034, 0.039, len(b))
    out, ex = _run_routes(hosttest_lib, ws.ragged_scene(), lambda p: p.sync_windows(d0, b, e, 0.0, 0.2),
                          lambda p: [p.window_trace(w) for w in range(len(b))], seed=SEED, max_outer_iters=7)
    _compare_routes("sync_windows", out)
    lengths = [len(t) for t in out["executor"][1]]
    print("trace lengths", lengths, "executor:", ex.executor_stats())
    assert len(set(lengths)) > 1, lengths
    assert ex.executor_stats()["runs"] > 0


def test_sync_points_of_200_frame_windows(hosttest_lib):
    """sync_points with sync_window = 200 (201 slots) at three positions, PreSync and two chained Sync calls each: past
    the executor's trial staging (kernels/executor.hpp:243: 10 * 201 > 1280, un-staged at :259) but inside the loop's
    (kernels/syncloop.hpp:87: 10 * 201 <= 2048, staged).  Executor == chain == host loop.  (The stand-in is not among
    the routes: set_init_override carries the winners of one call, a sync point makes two.)"""
    pos, window, repeats = ws.POINTS_POSITIONS, ws.POINTS_WINDOW, ws.POINTS_REPEATS
    out, ex = _run_routes(hosttest_lib, ws.ragged_scene(), lambda p: p.sync_points(pos, window, 0.0, 0.002, 0.1, repeats=repeats),
                          lambda p: [p.window_trace(w) for w in range(len(pos))], routes=("executor", "chain", "host loop"),
                          seed=SEED, max_outer_iters=7)
    _compare_routes("sync_points", out)
    assert all(len(t) > 7 for t in out["executor"][1])      # (rows of both calls)
    print("executor:", ex.executor_stats())
    assert ex.executor_stats()["runs"] > 0


# ---- (e) a long window with stragglers ---------------------------------------------------------------------------------

def test_long_window_with_frames_of_more_than_512_tracks(hosttest_lib):
    """700 frames from index 5, every tenth of 600 tracks (one slot in ten: within the one-in-eight share the executor
    accepts, rssync_kernels.hip rship_exec_supported), the rest 16 .. 130: the executor's BIG instantiation
    (kernels/executor.hpp sync_exec_kernel<R, true>), whose trial phase counts a task per trial of a big frame, with
    exec_window_sums un-staged at 10 and 2 rows (kernels/executor.hpp:259).  Executor == chain == stand-in."""
    out, ex = _run_routes(hosttest_lib, ws.straggler_scene(), lambda p: p.Sync(D0, 5, 704, 0.0, 0.1), lambda p: [p.sync_trace()],
                          routes=("executor", "chain", "stand-in"), seed=SEED, max_outer_iters=4)
    _compare_routes("Sync of 700 frames with stragglers", out)
    print("executor:", ex.executor_stats())
    assert ex.executor_stats()["runs"] > 0


# ---- (f) the wave's LDS region larger than the staging area ------------------------------------------------------------

def test_long_window_with_a_compact_fp64_window(built):
    """fs = 5000 Hz, 300 frames of 130 tracks: the regime of tests/test_gpu_executor.py::
    test_large_windows_with_compact_fp64_windows_equal_the_chain, where the wave's LDS region follows the (compact) fp64
    spline window, not the staging area -- with a window that is NOT staged at 10 rows (kernels/executor.hpp:243,259:
    10 * 300 > 1280) next to phases that are (2 * 300 <= 1280).  Executor == chain."""
    scene = ws.uniform_scene(300, 130, seed=77, fs=5000.0)
    out, ex = _run_routes(None, scene, lambda p: p.Sync(D0, 0, scene.F - 1, 0.0, 0.1), lambda p: [p.sync_trace()],
                          routes=("executor", "chain"), seed=77, max_outer_iters=6)
    _compare_routes("Sync at 5 kHz", out)
    info = ex.window_info()
    print("executor:", ex.executor_stats(), info)
    assert ex.executor_stats()["runs"] > 0
    assert info["fp64_window_compact"], info


# ---- (g) against the oracle --------------------------------------------------------------------------------------------

def test_long_window_loss_against_the_oracle(per_frame):
    """A reference outside the project's host code: the oracle's per-frame loss and analytic derivative with the device's
    motions (as tests/test_gpu_mid_sizes.py::test_more_than_2048_tracks_per_frame), added with plan_sum, against the
    device's loss of window (5, 641) -- rel 1e-12 for the loss, rel 1e-10 / abs 1e-10 |L| for the derivative, the bounds of
    that test.  A dropped or doubled slot is 1.6e-3 of such a sum."""
    from oracle.oracle import OracleProblem
    p, M, k, L, G, _ = per_frame
    b, n = 5, 641
    scene = ws.uniform_scene(4300, 16)
    o = OracleProblem(seed=SEED, threads=min(os.cpu_count() or 1, 16), faithful=False)
    scene.fill(o, end=b + n)
    Lw, Gw, _ = ws.window_values(p, M, k, D0, b, n)
    per = [[o.loss(f, d, M[f], k[f]) for f in range(b, b + n)] for d in ws.LOSS_DELAYS]
    checks = []
    for j, d in enumerate(ws.LOSS_DELAYS):
        Lo = np.array([x[0] for x in per[j]], np.float64)
        Go = np.array([x[2] for x in per[j]], np.float64)
        wantL, wantG = ws.plan_sum(Lo, b), ws.plan_sum(Go, b)
        print("delay %.4f: loss %.17g, oracle in plan order %.17g: relative difference %.3g (to the exact sum of the oracle's "
              "values %.3g; plan order against exact sum %.3g); per frame, device against oracle: max relative %.3g" % (
                  d, Lw[j], wantL, abs(Lw[j] - wantL) / abs(wantL), abs(Lw[j] - ws.exact_sum(Lo)) / abs(wantL),
                  abs(wantL - ws.exact_sum(Lo)) / abs(wantL), np.max(np.abs(L[b:b + n, j] - Lo) / np.abs(Lo))))
        print("delay %.4f: derivative %.17g, oracle in plan order %.17g: difference %.3g = %.3g |L| (to the exact sum %.3g); "
              "per frame, device against oracle: max |difference| %.3g" % (
                  d, Gw[j], wantG, abs(Gw[j] - wantG), abs(Gw[j] - wantG) / abs(Lw[j]), abs(Gw[j] - ws.exact_sum(Go)),
                  np.max(np.abs(G[b:b + n, j] - Go))))
        checks.append((Lw[j], wantL, Gw[j], wantG))
    for Lj, wantL, Gj, wantG in checks:
        assert Lj == pytest.approx(wantL, rel=1e-12)
        assert Gj == pytest.approx(wantG, rel=1e-10, abs=1e-10 * abs(Lj))


def test_long_window_sync_against_the_oracle(built):
    """like for like, as tests/test_gpu_mid_sizes.py:241-245: window (37, 129) of the uniform scene, a fresh pair, the
    oracle's GuessMotion winners installed on the device, the same twelve iterations -- delays within 1e-6 s, costs
    within 1e-6 relative"""
    from oracle.oracle import OracleProblem
    b, n = 37, 129
    scene = ws.uniform_scene(4300, 16)
    o = OracleProblem(seed=SEED, max_outer_iters=12, threads=min(os.cpu_count() or 1, 16), faithful=False)
    scene.fill(o, end=b + n)
    h = _device(seed=SEED, max_outer_iters=12)
    scene.fill(h, end=b + n)
    co, do = o.Sync(0.036, b, b + n - 1, 0.0, 0.2)
    h.set_init_override(o.last_init_winners())
    c, d = h.Sync(0.036, b, b + n - 1, 0.0, 0.2)
    print("Sync of window (%d, %d): delay %.12g, oracle %.12g, difference %.3g s; cost %.12g, oracle %.12g, relative %.3g" % (
        b, n, d, do, abs(d - do), c, co, abs(c - co) / abs(co)))
    assert abs(d - do) < 1e-6 and abs(c - co) <= 1e-6 * abs(co), (c, d, co, do)
