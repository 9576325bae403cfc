"""One rank of the ownership tests (tests/test_rank_ownership.py, tests/test_gpu_rank_ownership.py): this rank's frames of a
PATTERN in its own SyncProblem, gloo for the sums through the length-checking reduce hook (tests/rank_exchange.py), and
every entry point that exchanges, each on a fresh problem.  Per entry point: its result, the lengths this rank exchanged
and the error it raised, if any.  The parent computes the same cases in one process that holds every frame (run_entry).

    python ownership_worker.py RANK WORLD PORT OUT.json LIB PATTERN [ENTRY ...]

LIB: a path to a build of the library (the host solver on the CPU test double), or "product" (the package's library on
the GPU: every rank on device 0)."""
import ctypes
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIRST, LAST = 30, 46                         # the scene's frames: 30 .. 45
SEED = 77
ORIENTATIONS = ["XYZ", "xYz", "Xzy", "YXz", "zyx"]   # the true one first (the scene's rates are XYZ)
READOUTS = [0.006, 0.011, 0.016]


def _owned(world, fn):
    return [list(fn(r)) for r in range(world)]


def _shard(b, e, world):
    from rssync_amd.dist import shard
    return _owned(world, lambda r: range(*shard(b, e, r, world)))


# world size, each rank's frames, the range [begin, end) the entry points work on, tracks per frame, frames of zero rays
PATTERNS = {
    "even2": dict(world=2, owned=lambda: _shard(30, 46, 2), range=(30, 46)),
    "even4": dict(world=4, owned=lambda: _shard(30, 46, 4), range=(30, 46)),
    "uneven_13_3": dict(world=2, owned=lambda: [list(range(30, 43)), list(range(43, 46))], range=(30, 46)),
    "one_holds_all": dict(world=3, owned=lambda: [list(range(30, 46)), [], []], range=(30, 46)),
    "outside_range": dict(world=3, owned=lambda: [list(range(30, 38)), list(range(38, 42)), list(range(42, 46))],
                          range=(30, 42)),
    "gyro_no_frames": dict(world=3, owned=lambda: [list(range(30, 38)), [], list(range(38, 46))], range=(30, 46)),
    "shard_5_over_4": dict(world=4, owned=lambda: _shard(30, 35, 4), range=(30, 35)),
    "size_classes": dict(world=2, owned=lambda: [list(range(30, 38)), list(range(38, 46))], range=(30, 46),
                         tracks=lambda fr: 96 if fr < 38 else 600),
    # the collective panic: rank 1 holds a frame whose rays are all zero (r = NaN: "pre-sync: non-finite r")
    "zero_rays": dict(world=2, owned=lambda: [list(range(30, 38)), list(range(38, 46))], range=(30, 46), zero=(41,)),
    # the GPU cases: a rank whose only frame lies outside the range; the old slice bound (3000 / 3500 frames of 8 tracks)
    "empty_in_range": dict(world=2, owned=lambda: [list(range(30, 42)), [50]], range=(30, 42), last=51),
    "across_slice": dict(world=2, owned=lambda: [list(range(30, 3030)), list(range(3030, 6530))], range=(30, 6530),
                         last=6530, tracks=lambda fr: 8, candidates=(0.00002, 0.11)),
}

ENTRIES = ["presync", "pre_sync_windows", "sync", "sync_windows", "sync_points", "sync_simplified", "orientation_sweep",
           "orientation_sweep_plain", "readout_sweep", "set_readout"]


def pattern(name):
    pat = dict(PATTERNS[name])
    pat["owned"] = pat["owned"]()
    pat.setdefault("tracks", lambda fr: 64)
    pat.setdefault("zero", ())
    pat.setdefault("last", LAST)
    pat.setdefault("candidates", (0.004, 0.1))
    return pat


def gyro(pat):
    from rssync_amd import synth
    return synth.make_gyro(FIRST / synth.FPS, pat["last"] / synth.FPS + 2 / synth.FPS, seed=SEED)


def frames(pat, ids, pixels):
    """the frames `ids` of the pattern's scene: (frame, ...) tuples of set_track_pixels' or SetTrackResult's arguments;
    every frame is the same whichever rank holds it"""
    from rssync_amd import synth
    g = gyro(pat)
    make = synth.make_pixel_frames if pixels else synth.make_frames
    runs = []  # (synth keys every frame on (seed, frame): runs of consecutive frames of one size are made at once)
    for fr in ids:
        if runs and runs[-1][1] == fr and pat["tracks"](fr) == pat["tracks"](runs[-1][0]):
            runs[-1][1] = fr + 1
        else:
            runs.append([fr, fr + 1])
    out = []
    for b, e in runs:
        for f in make(g, b, e, pat["tracks"](b), seed=SEED):
            f = list(f)
            if f[0] in pat["zero"] and not pixels:
                f[3] = np.zeros_like(f[3])
                f[4] = np.zeros_like(f[4])
            out.append(f)
    return out


def problem(lib, pat, ids, kind):
    """a problem with the frames `ids`: kind "rays" (gyro as quaternions), "rates" (frames only: the sweep sets the gyro)
    or "pixels" (gyro as quaternions, pixel frames)"""
    import rssync_amd
    from rssync_amd import synth
    p = rssync_amd.SyncProblem(seed=SEED, max_outer_iters=10, _lib=lib)
    g = gyro(pat)
    if kind != "rates":
        p.SetGyroQuaternions(g.quats, g.fs, g.t0)
    for f in frames(pat, ids, kind == "pixels"):
        if kind == "pixels":
            p.set_track_pixels(*f, synth.LENS, synth.IMAGE_ROWS)
        else:
            p.SetTrackResult(*f)
    return p


def n_candidates(step, radius):
    """how many candidate delays PreSync's loop yields around 0 (core_private.cpp:69-70)"""
    n, d = 0, -radius
    while d < radius:
        n += 1
        d += step
    return n


KIND = {"orientation_sweep": "rates", "orientation_sweep_plain": "rates", "readout_sweep": "pixels", "set_readout": "pixels"}


def run_entry(lib, pat, ids, entry, hook=None, device_loop=False):
    """one entry point on a fresh problem with the frames `ids` -> {"costs": [...], "delays": [...]}"""
    p = problem(lib, pat, ids, KIND.get(entry, "rays"))
    if hook is not None:
        p.set_reduce_hook(hook)
        p.set_hook_device_loop(device_loop)
    b, e = pat["range"]
    mid = (b + e) // 2
    step, radius = pat["candidates"]
    if entry == "presync":
        c, d = p.PreSync(0.0, b, e, step, radius)
    elif entry == "pre_sync_windows":
        c, d = p.pre_sync_windows(0.02, [b, b + 1], [mid, e], step, radius)
    elif entry == "sync":
        c, d = p.Sync(0.03, b, e - 1, 0.0, 0.2)
    elif entry == "sync_windows":
        c, d = p.sync_windows([0.03, 0.036], [b, b + 1], [mid, e - 1], 0.0, 0.2)
    elif entry == "sync_points":
        c, d = p.sync_points([b, mid], 3 if e - b < 8 else 6, 0.02, 0.004, 0.04, repeats=2)
    elif entry == "sync_simplified":
        c, d = p.SyncSimplified(0.0355, b, e - 1, 0.0, 0.1)
    elif entry in ("orientation_sweep", "orientation_sweep_plain"):
        g = gyro(pat)
        plain = entry == "orientation_sweep_plain"
        if plain:
            os.environ["RSSYNC_SWEEP_PIPELINE"] = "0"
        try:
            c, d = p.orientation_sweep(g.times, g.rates, ORIENTATIONS, 0.0, b, e, step, radius)
        finally:
            if plain:
                del os.environ["RSSYNC_SWEEP_PIPELINE"]
    elif entry == "readout_sweep":
        c, d = p.readout_sweep(READOUTS, 0.0, b, e, step, radius)
    elif entry == "set_readout":
        p.set_readout(0.008)
        c, d = p.PreSync(0.0, b, e, step, radius)
    else:
        raise ValueError(entry)
    return dict(costs=np.atleast_1d(c).astype(np.float64).tolist(), delays=np.atleast_1d(d).astype(np.float64).tolist())


def main():
    rank, world, port, out, lib_arg, name = sys.argv[1:7]
    rank, world, port = int(rank), int(world), int(port)
    entries = sys.argv[7:] or ENTRIES
    if lib_arg == "product":
        import torch
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    from rssync_amd.problem import RsSyncError, bind
    from rank_exchange import checked_reduce_hook
    lib = None if lib_arg == "product" else bind(ctypes.CDLL(lib_arg))
    pat = pattern(name)
    res = {}
    for entry in entries:
        loop = entry.endswith(":device_loop")
        hook = checked_reduce_hook()
        try:
            r = dict(out=run_entry(lib, pat, pat["owned"][rank], entry.split(":")[0], hook, loop), error=None)
        except RsSyncError as exc:
            cause = exc.__cause__
            r = dict(out=None, error=str(exc) + (" <- %s: %s" % (type(cause).__name__, cause) if cause else ""))
        r["lengths"] = hook.lengths
        res[entry] = r
    with open(out, "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
