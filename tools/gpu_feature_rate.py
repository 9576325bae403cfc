"""Feature-tracker throughput on the GPU (include/rssync_features.h): frames per second for detect + forward + backward
LK at three frame sizes, batches of 64 frames, from host numpy arrays and from device tensors; and, from one
`rocprofv3 --kernel-trace --stats` run of the same workload, per-kernel times.

    python tools/gpu_feature_rate.py [--out profiles/feature_rate.json] [--reps 5] [--no-profile]

The frames are tools/gpu_track_rate.py's drifting texture.  The profiled pass is a child process (`--inner`) started
under rocprofv3; its kernel statistics are read back here.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_track_rate import BATCH, SIZES, frames_of  # noqa: E402

KERNELS = ("corner_cell_kernel", "corner_select_kernel", "lkfb_kernel", "pyr_down_kernel")


def inner():
    """the workload the profiler sees: one host and one device batch per size"""
    import torch
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=1)
    for w, h in SIZES:
        f = frames_of(w, h)
        p.track_features(f)
        p.track_features(torch.from_numpy(f).to("cuda:0"))
    torch.cuda.synchronize()


def kernel_stats(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    stats = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            for key in KERNELS:
                if key in name:
                    s = stats.setdefault(key, {"calls": 0, "total_ns": 0.0})
                    s["calls"] += int(row["Calls"])
                    s["total_ns"] += float(row["TotalDurationNs"])
    return stats


def timed(fn, reps):
    fn()                                                         # warm-up (buffers, code object)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                     # returns after the device synchronise
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--inner", action="store_true")
    a = ap.parse_args()
    if a.inner:
        inner()
        return
    import torch
    import rssync_amd
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    p = rssync_amd.SyncProblem(seed=1)
    res = {"batch_frames": BATCH, "cell": 64, "block": 5, "quality": 0.01, "window": 21, "levels": 4, "sizes": []}
    for w, h in SIZES:
        f = frames_of(w, h)
        out = p.track_features(f)
        row = {"width": w, "height": h, "cells_per_frame": int(out.points_a.shape[1]),
               "features_per_pair_median": float(np.median(out.counts)),
               "kept_per_pair_median": float(np.median([(out.status[k, :c] == 0).sum() for k, c in enumerate(out.counts)]))}
        row["host_numpy_s"] = timed(lambda: p.track_features(f), a.reps)
        row["host_numpy_fps"] = BATCH / row["host_numpy_s"]
        dev = torch.from_numpy(f).to("cuda:0")
        row["device_tensor_s"] = timed(lambda: p.track_features(dev), a.reps)
        row["device_tensor_fps"] = BATCH / row["device_tensor_s"]
        # the grid tracker on the same batch, for comparison
        row["grid_tracker_device_tensor_s"] = timed(lambda: p.track_points(dev), a.reps)
        res["sizes"].append(row)
        del dev
        print(json.dumps(row), flush=True)
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "features", "--", sys.executable,
                   os.path.abspath(__file__), "--inner"]
            rc = subprocess.run(cmd, cwd=ROOT, timeout=600).returncode
            stats = kernel_stats(d) if rc == 0 else None
        res["rocprofv3_rc"] = rc
        if stats:
            res["kernels"] = stats      # the profiled pass: every size twice (a host and a device batch of 64 frames)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "sizes"}, indent=1))


if __name__ == "__main__":
    main()
