"""Tracker throughput on the GPU (include/rssync_track.h): frames per second at three frame sizes, batches of 64
frames, from host numpy arrays and from device tensors; the upload rate of the frames against PCIe Gen5 x16 (63 GB/s
per direction, a spec number); and, from one `rocprofv3 --kernel-trace --stats` run of the same workload, per-kernel
times and the pyramid kernel's bytes / time against the measured achievable 6.29 TB/s (MI355X_MICROARCH.md).

    python tools/gpu_track_rate.py [--out profiles/track_rate.json] [--reps 5] [--no-profile]

The profiled pass is a child process (`--inner`) started under rocprofv3; its kernel statistics are read back here.
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

SIZES = [(1352, 760), (2704, 2028), (3840, 2160)]
BATCH = 64
HBM_ACHIEVABLE = 6.29e12
PCIE_SPEC = 63e9


def frames_of(w, h, n=BATCH, seed=0):
    """a smooth random texture drifting a few pixels per frame"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(h // 8 + 8, w // 8 + 8)).astype(np.float32)
    base = np.repeat(np.repeat(base, 8, 0), 8, 1)
    k = np.array([1, 4, 6, 4, 1], np.float32) / 16
    for ax in (0, 1):
        for _ in range(3):
            base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), ax, base)
    tex = np.clip(base, 0, 255).astype(np.uint8)
    out = np.empty((n, h, w), np.uint8)
    for i in range(n):
        out[i] = tex[(i * 3) % 40:(i * 3) % 40 + h, (i * 2) % 40:(i * 2) % 40 + w]
    return out


def pyramid_bytes(w, h, levels=4):
    """bytes pyr_down_kernel moves for one frame: each level reads the one below once (bytes at level 0, fp32 above) and
    writes itself in fp32"""
    total, lw, lh, src = 0, w, h, 1
    for _ in range(1, levels):
        nw, nh = (lw + 1) // 2, (lh + 1) // 2
        total += lw * lh * src + nw * nh * 4
        lw, lh, src = nw, nh, 4
    return total


def inner():
    """the workload the profiler sees: one host and one device batch per size"""
    import torch
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=1)
    for w, h in SIZES:
        f = frames_of(w, h)
        p.track_points(f)
        p.track_points(torch.from_numpy(f).to("cuda:0"))
    torch.cuda.synchronize()


def kernel_stats(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    stats = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            for key in ("pyr_down_kernel", "lk_kernel"):
                if key in name:
                    s = stats.setdefault(key + ("<u8>" if "ILb1E" in name or "<true>" in name else "<f32>" if key == "pyr_down_kernel" else ""),
                                         {"calls": 0, "total_ns": 0.0})
                    s["calls"] += int(row["Calls"])
                    s["total_ns"] += float(row["TotalDurationNs"])
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_rate.json"))
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
    res = {"batch_frames": BATCH, "grid_step": 200, "window": 21, "levels": 4, "sizes": []}
    for w, h in SIZES:
        f = frames_of(w, h)
        pts = len(range(200, w, 200)) * len(range(200, h, 200))
        row = {"width": w, "height": h, "points_per_pair": pts, "frame_bytes": w * h}
        p.track_points(f)                                            # warm-up (buffers, code object)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            p.track_points(f)                                        # returns after the device synchronise
            t.append(time.perf_counter() - t0)
        row["host_numpy_s"] = float(np.median(t))
        row["host_numpy_fps"] = BATCH / row["host_numpy_s"]
        dev = torch.from_numpy(f).to("cuda:0")
        p.track_points(dev)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            p.track_points(dev)
            t.append(time.perf_counter() - t0)
        row["device_tensor_s"] = float(np.median(t))
        row["device_tensor_fps"] = BATCH / row["device_tensor_s"]
        # the upload alone: pageable (what a numpy batch is) and pinned host memory -> device
        pinned = torch.from_numpy(f).pin_memory()
        for kind, src in (("pageable", torch.from_numpy(f)), ("pinned", pinned)):
            src.to("cuda:0")
            torch.cuda.synchronize()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                src.to("cuda:0", non_blocking=(kind == "pinned"))
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
            gbs = f.nbytes / float(np.median(t))
            row["upload_%s_GBps" % kind] = gbs / 1e9
            row["upload_%s_of_pcie_spec" % kind] = gbs / PCIE_SPEC
        row["pyramid_bytes_per_frame"] = pyramid_bytes(w, h)
        res["sizes"].append(row)
        del dev, pinned
        print(json.dumps(row), flush=True)
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "track", "--", sys.executable,
                   os.path.abspath(__file__), "--inner"]
            rc = subprocess.run(cmd, cwd=ROOT, timeout=600).returncode
            stats = kernel_stats(d) if rc == 0 else None
        res["rocprofv3_rc"] = rc
        if stats:
            res["kernels"] = stats
            # the profiled pass: every size twice (host + device batch) -> pyramid bytes of 2 * 64 frames per size
            pb = sum(2 * BATCH * pyramid_bytes(w, h) for w, h in SIZES)
            pyr_ns = sum(v["total_ns"] for k, v in stats.items() if k.startswith("pyr_down_kernel"))
            if pyr_ns:
                res["pyramid_bytes_per_s"] = pb / (pyr_ns * 1e-9)
                res["pyramid_of_hbm_achievable"] = res["pyramid_bytes_per_s"] / HBM_ACHIEVABLE
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "sizes"}, indent=1))


if __name__ == "__main__":
    main()
