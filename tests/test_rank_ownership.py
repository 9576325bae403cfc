"""Ranked runs whatever frames a rank holds: every entry point that exchanges, under the ownership patterns of
tests/ownership_worker.py (even and uneven splits, every frame on one rank, frames only outside the range, a rank with the
gyro and no frame, dist.shard's 5 frames over 4 ranks, ranks of two size classes), 2 to 4 gloo ranks on the host solver
linked against the CPU test double.  Every rank must make the same exchanges (the length-checking hook of
tests/rank_exchange.py: a mismatch is an error on every rank, not a hang), return the same bits, and agree with one
process that holds every frame -- bit for bit when one rank holds them all (the others add exact zeros), else within
tests/test_dist_gloo.py's tolerances.  And the rule that picks the batched sweeps' route (window_plan.hpp
plan_sweep_pipelined) reads nothing a rank holds alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ownership_worker as w
from ownership_worker import n_candidates
from rank_exchange import bits, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ownership_worker.py")
PATTERNS = ["even2", "even4", "uneven_13_3", "one_holds_all", "outside_range", "gyro_no_frames", "shard_5_over_4",
            "size_classes"]
PRESYNC_LIKE = {"presync", "pre_sync_windows", "orientation_sweep", "orientation_sweep_plain", "readout_sweep", "set_readout"}
PANICS = ["presync", "pre_sync_windows", "sync_points", "orientation_sweep", "orientation_sweep_plain"]

_ranked, _single = {}, {}


def ranked(lib, name, tmp_path_factory):
    """every rank's results of every entry point (one run of the pattern's ranks, kept for the module)"""
    if name not in _ranked:
        out = tmp_path_factory.mktemp(name)
        _ranked[name] = run_ranks(WORKER, w.PATTERNS[name]["world"], [lib._name, name], out, timeout=300)
    return _ranked[name]


def single(lib, name, entry):
    """the same entry point in one process that holds every frame of the pattern, without a hook"""
    if (name, entry) not in _single:
        pat = w.pattern(name)
        ids = sorted(fr for own in pat["owned"] for fr in own)
        _single[(name, entry)] = w.run_entry(lib, pat, ids, entry)
    return _single[(name, entry)]


@pytest.mark.parametrize("entry", w.ENTRIES)
@pytest.mark.parametrize("name", PATTERNS)
def test_every_rank_makes_the_same_exchanges_and_agrees_with_one_process(hosttest_lib, tmp_path_factory, name, entry):
    res = [r[entry] for r in ranked(hosttest_lib, name, tmp_path_factory)]
    for rank, r in enumerate(res):
        assert r["error"] is None, "rank %d: %s" % (rank, r["error"])
    for r in res[1:]:
        assert r["lengths"] == res[0]["lengths"]
        assert bits(r["out"]["costs"]) == bits(res[0]["out"]["costs"])
        assert bits(r["out"]["delays"]) == bits(res[0]["out"]["delays"])
    n = n_candidates(*w.pattern(name)["candidates"])
    n_or, n_ro = len(w.ORIENTATIONS), len(w.READOUTS)
    want = {"presync": [n + 4], "set_readout": [n + 4],
            "orientation_sweep": [n_or * n + 5 * n_or],     # ONE exchange of the [orientation][candidate] matrix
            "orientation_sweep_plain": [n + 4] * n_or,      # RSSYNC_SWEEP_PIPELINE=0: a PreSync per orientation
            "readout_sweep": [n + 4] * n_ro}                # (the CPU double has no re-timing launcher: a PreSync per readout)
    if entry in want:
        assert res[0]["lengths"] == want[entry]
    one, got = single(hosttest_lib, name, entry), res[0]["out"]
    if name == "one_holds_all":
        assert bits(got["costs"]) == bits(one["costs"]) and bits(got["delays"]) == bits(one["delays"])
    elif entry in PRESYNC_LIKE:
        assert got["delays"] == one["delays"]                              # the same arg-mins
        np.testing.assert_allclose(got["costs"], one["costs"], rtol=1e-12)
    else:
        np.testing.assert_allclose(got["delays"], one["delays"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got["costs"], one["costs"], rtol=1e-9)


def test_the_non_finite_r_panic_is_collective(hosttest_lib, tmp_path_factory):
    """rank 1 holds a frame whose rays are all zero (tests/test_gpu_parity.py
    test_rows_below_safe_normalizes_threshold_and_the_non_finite_r_panic): its flag rides along with the sums, so EVERY
    rank raises the same panic after the same exchange -- the one a single process raises"""
    from rssync_amd.problem import RsSyncError
    out = tmp_path_factory.mktemp("zero_rays")
    res = run_ranks(WORKER, 2, [hosttest_lib._name, "zero_rays"] + PANICS, out, timeout=300)
    pat = w.pattern("zero_rays")
    for entry in PANICS:
        with pytest.raises(RsSyncError) as one:
            w.run_entry(hosttest_lib, pat, list(range(30, 46)), entry)
        assert str(one.value) == "pre-sync: non-finite r"
        for r in res:
            assert r[entry]["error"] == "pre-sync: non-finite r", entry
            assert r[entry]["lengths"] == res[0][entry]["lengths"], entry


SHIM = r'''
#include "window_plan.hpp"
extern "C" int pipelined(unsigned long items, unsigned long cand, unsigned long win, unsigned long sel, long b, long e, int dist) {
    return rs::plan_sweep_pipelined(items, cand, win, sel, b, e, dist != 0) ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    d = tmp_path_factory.mktemp("route")
    (d / "shim.cpp").write_text(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "rs-sync_amd", "csrc"),
                           "-o", str(d / "libroute.so"), str(d / "shim.cpp")])
    L = ctypes.CDLL(str(d / "libroute.so"))
    L.pipelined.argtypes = [ctypes.c_ulong] * 4 + [ctypes.c_long, ctypes.c_long, ctypes.c_int]
    return lambda items, cand, win, sel, b, e, dist: bool(L.pipelined(items, cand, win, sel, b, e, int(dist)))


def old_rule(items, cand, win, sel):
    """the single-process rule before the ranks had their own (kept: one process routes as it did)"""
    slice_ = max(64, (256 << 20) // (8 * max(sel, 1)))
    return not (items > 255 or cand > slice_ or not sel or items * cand * (win + 1) > (1 << 28))


def test_the_sweep_route_reads_nothing_a_rank_holds_alone(route):
    rng = np.random.default_rng(5)
    cases = [(5, 11000, 1, 3000, 0, 6500), (5, 11000, 1, 3500, 0, 6500), (5, 50, 1, 0, 30, 42), (2, 64, 1, 0, 0, 1 << 40),
             (255, 1000, 1, 7, 0, 7), (256, 10, 1, 7, 0, 7), (5, 9586, 1, 3500, 0, 3500), (5, 9587, 1, 3500, 0, 3500),
             (4, 1 << 20, 1, 1, 0, 1), (3, 30, 1, 0, 10, 10), (3, 30, 1, 0, 10, 5)]
    cases += [(int(rng.integers(1, 300)), int(rng.integers(1, 40000)), 1, int(rng.integers(0, 5000)), 0,
               int(rng.integers(0, 9000))) for _ in range(300)]
    for items, cand, win, sel, b, e in cases:
        # one process: exactly the old rule
        assert route(items, cand, win, sel, b, e, False) == old_rule(items, cand, win, sel), (items, cand, sel)
        # ranks: the same answer whatever the rank holds of the range -- nothing, part, all of it
        width = max(e - b, 0)
        got = {route(items, cand, win, s, b, e, True) for s in {0, 1, sel if sel <= width else width, width}}
        assert len(got) == 1, (items, cand, sel, b, e)
        # ... and that answer is the one process's for the whole range when the range holds a frame
        if width:
            assert got == {old_rule(items, cand, win, width)}, (items, cand, b, e)
    # the GPU test's case across the old bound: 3000 frames pipelined, 3500 not -- now both ranks go the plain way
    assert old_rule(5, 11000, 1, 3000) and not old_rule(5, 11000, 1, 3500)
    assert not route(5, 11000, 1, 3000, 0, 6500, True) and not route(5, 11000, 1, 3500, 0, 6500, True)
    # a range without frames on any rank is still one pipeline of zeros on every rank
    assert route(5, 50, 1, 0, 30, 42, True) and not route(5, 50, 1, 0, 30, 42, False)
