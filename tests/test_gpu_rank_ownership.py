"""Ranked runs on the device whatever frames a rank holds (the CPU side: tests/test_rank_ownership.py).  Two or three ranks
share the box's one GPU and exchange over gloo through the length-checking hook of tests/rank_exchange.py -- never the
library's RCCL communicator here: a mismatched exchange there is a collective that spins on the device.  Only here does the
readout sweep take its pipeline (the CPU double has no re-timing launcher).  Each run of the ranks has its own timeout; a
run that fails ends this module's GPU work (the later tests fail at once, without starting anything on the GPU)."""
import pytest

import ownership_worker as w
from ownership_worker import n_candidates
from rank_exchange import bits, run_ranks

WORKER = w.__file__

pytestmark = pytest.mark.gpu

_failed = []


def _ranks(name, entries, tmp_path, timeout):
    if _failed:
        pytest.fail("an earlier ranked run of this module failed (%s): nothing more is started on the GPU" % _failed[0])
    try:
        return run_ranks(WORKER, w.PATTERNS[name]["world"], ["product", name] + entries, tmp_path, timeout=timeout)
    except AssertionError:
        _failed.append(name)
        raise


def _check(name, res, entries):
    """no rank failed, every rank exchanged the same lengths and returned the same bits; -> rank 0's results"""
    for entry in entries:
        for rank, r in enumerate(res):
            assert r[entry]["error"] is None, "%s, rank %d: %s" % (entry, rank, r[entry]["error"])
            assert r[entry]["lengths"] == res[0][entry]["lengths"], entry
            assert bits(r[entry]["out"]["costs"]) == bits(res[0][entry]["out"]["costs"]), entry
            assert bits(r[entry]["out"]["delays"]) == bits(res[0][entry]["out"]["delays"]), entry
    return {entry: res[0][entry] for entry in entries}


def _against_one_process(name, got):
    """the same entry points in this process, holding every frame of the pattern, without a hook"""
    import numpy as np
    pat = w.pattern(name)
    ids = sorted(fr for own in pat["owned"] for fr in own)
    for entry, r in got.items():
        one = w.run_entry(None, pat, ids, entry.split(":")[0])
        if entry.startswith("sync"):
            np.testing.assert_allclose(r["out"]["delays"], one["delays"], rtol=0, atol=1e-9, err_msg=entry)
            np.testing.assert_allclose(r["out"]["costs"], one["costs"], rtol=1e-9, err_msg=entry)
        else:
            assert r["out"]["delays"] == one["delays"], entry                     # the same arg-mins
            np.testing.assert_allclose(r["out"]["costs"], one["costs"], rtol=1e-12, err_msg=entry)


def _one_exchange_per_sweep(got, name):
    n = n_candidates(*w.pattern(name)["candidates"])
    n_or, n_ro = len(w.ORIENTATIONS), len(w.READOUTS)
    assert got["orientation_sweep"]["lengths"] == [n_or * n + 5 * n_or]
    assert got["readout_sweep"]["lengths"] == [n_ro * n + 5 * n_ro]          # the pipeline: the device re-times


ENTRIES = ["presync", "sync", "sync:device_loop", "orientation_sweep", "readout_sweep"]


def test_a_rank_without_a_frame_of_the_range(built, tmp_path):
    """rank 0 holds frames 30 .. 41, rank 1 only frame 50; everything works on [30, 42) (before: rank 1 took the sweeps'
    per-item route, 54 doubles per exchange against the others' one matrix)"""
    got = _check("empty_in_range", _ranks("empty_in_range", ENTRIES, tmp_path, 300), ENTRIES)
    _one_exchange_per_sweep(got, "empty_in_range")
    assert got["sync"]["out"] == got["sync:device_loop"]["out"]              # the loop on the device: the same decisions
    _against_one_process("empty_in_range", got)


def test_a_rank_with_the_gyro_and_no_frames(built, tmp_path):
    got = _check("gyro_no_frames", _ranks("gyro_no_frames", ENTRIES, tmp_path, 300), ENTRIES)
    _one_exchange_per_sweep(got, "gyro_no_frames")
    assert got["sync"]["out"] == got["sync:device_loop"]["out"]
    _against_one_process("gyro_no_frames", got)


def test_ranks_on_either_side_of_the_sweep_slice(built, tmp_path):
    """3000 and 3500 frames of 8 tracks, ~11 000 candidates, five orientations: by the rank's OWN frames one rank's
    candidates fit the pipeline's [candidates][frames] matrix and the other's do not; by the range's 6500 frames neither
    does, so both ranks sweep orientation by orientation (one exchange of n + 4 doubles each)"""
    got = _check("across_slice", _ranks("across_slice", ["orientation_sweep"], tmp_path, 600), ["orientation_sweep"])
    n = n_candidates(*w.pattern("across_slice")["candidates"])
    assert 10000 < n < 12000
    assert got["orientation_sweep"]["lengths"] == [n + 4] * len(w.ORIENTATIONS)
    _against_one_process("across_slice", got)
