"""The CPU stand-in of the device ABI (tests/cpu_device/rship_cpu.cpp, linked with the product's host solver) tied to the
numpy restatement of the window sums' association (tests/window_sum_reference.py): on windows of up to 4200 frames the
stand-in's loss, derivative, five-delay batch and PreSync curve are, bit for bit, plan_sum of the values it gives every
frame alone.  From there on the stand-in is the reference for whole Sync traces on long windows
(tests/test_gpu_long_windows.py); these tests need no GPU.
"""
import numpy as np
import pytest

import window_sum_reference as ws


def _problem(hosttest_lib, scene, **kw):
    import rssync_amd
    p = rssync_amd.SyncProblem(_lib=hosttest_lib, **kw)
    scene.fill(p)
    return p


@pytest.fixture(scope="module")
def per_frame(hosttest_lib):
    """4300 frames of 16 tracks: motions once from the whole range, then every frame's values alone"""
    scene = ws.uniform_scene(4300, 16)
    p = _problem(hosttest_lib, scene, seed=7)
    M, k = p.init_motion(ws.LOSS_DELAYS[0], 0, scene.F - 1)
    return (p, M, k) + ws.per_frame_values(p, M, k, ws.LOSS_DELAYS[0], range(scene.F))


def test_window_loss_is_the_plan_order_sum_of_the_frames_alone(per_frame):
    """rship_cpu.cpp plan_sum (the stand-in's copy of plan_sum_kernel, kernels/support.hpp:19-56) against plan_sum of
    tests/window_sum_reference.py: loss and derivative at two delays and the five-delay batch of a window equal the
    plan-order sum of the single-frame values in every bit -- windows of one chunk, of two, with ragged first chunks,
    of one and two slots, and the long ones of the GPU tests (129 .. 1281: kernels/executor.hpp:243 and
    kernels/syncloop.hpp:87 stop staging there; 4161 from 0: 66 chunks).  A flat sequential sum of the same values must
    differ from the window's loss somewhere among the long windows, or the comparison could not tell associations apart."""
    p, M, k, L, G, B = per_frame
    flat_differs = 0
    for b, n in ws.CPU_LOSS_WINDOWS:
        Lw, Gw, Bw = ws.window_values(p, M, k, ws.LOSS_DELAYS[0], b, n)
        np.testing.assert_array_equal(ws.bits(Lw), ws.bits(ws.plan_sums(L, b, n)), err_msg="loss, window %r" % ((b, n),))
        np.testing.assert_array_equal(ws.bits(Gw), ws.bits(ws.plan_sums(G, b, n)), err_msg="derivative, window %r" % ((b, n),))
        np.testing.assert_array_equal(ws.bits(Bw), ws.bits(ws.plan_sums(B, b, n)), err_msg="batch, window %r" % ((b, n),))
        if ws.n_chunks(b, n) > 1:
            flat = [ws.flat_sum(L[b:b + n, c]) for c in range(2)] + [ws.flat_sum(G[b:b + n, c]) for c in range(2)]
            flat_differs += int(np.any(ws.bits(flat) != ws.bits(np.concatenate([Lw, Gw]))))
    assert flat_differs >= 1, "a flat sum gives the window's bits everywhere: the anchor is blind to the association"


@pytest.fixture(scope="module")
def presync_problem(hosttest_lib):
    return _problem(hosttest_lib, ws.uniform_scene(4300, 8), seed=7)


@pytest.mark.parametrize("b,n", ws.PRESYNC_WINDOWS)
def test_presync_curve_is_the_plan_order_sum_of_the_frame_costs(presync_problem, b, n):
    """every candidate's cost of a PreSync sweep is plan_sum of the per-frame costs the same call returns: 129 frames from
    37 (three chunks, the first ragged), 4161 from 0 (66 chunks) and 4200 from 100 (67 chunks, ragged at both ends)"""
    d0, step, radius = ws.PRESYNC_ARGS
    d, curve, per, _ = presync_problem.presync_curve(d0, b, b + n, step, radius, per_frame=n)
    assert per.shape == (len(d), n) and len(d) >= 5
    want = [ws.plan_sum(per[c], b) for c in range(len(d))]
    np.testing.assert_array_equal(ws.bits(curve), ws.bits(want))


def test_batched_presync_on_overlapping_long_windows_is_the_single_calls(hosttest_lib):
    """pre_sync_windows on overlapping windows (a frame has a position in several windows: the plan carries an index
    list, `plan_has_idx` in rship_cpu.cpp plan_sum, idx != NULL in kernels/support.hpp:19-56) returns per window the bits
    of a single PreSync call on that window -- 4161, 129, 641 and 1281 frames"""
    scene = ws.uniform_scene(4300, 8)
    d0, step, radius = ws.PRESYNC_ARGS
    batch = _problem(hosttest_lib, scene, seed=7)
    c, d = batch.pre_sync_windows(d0, ws.PRESYNC_BATCH_BEGINS, ws.PRESYNC_BATCH_ENDS, step, radius)
    single = _problem(hosttest_lib, scene, seed=7)
    for w, (b, e) in enumerate(zip(ws.PRESYNC_BATCH_BEGINS, ws.PRESYNC_BATCH_ENDS)):
        cs, ds = single.PreSync(d0, b, e, step, radius)
        assert (float(c[w]).hex(), float(d[w]).hex()) == (cs.hex(), ds.hex()), (w, b, e)
