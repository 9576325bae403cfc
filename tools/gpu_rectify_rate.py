"""Rectifier throughput on the GPU (include/rssync_rectify.h): frames per second at three frame sizes, batches of 16
frames, device-resident (tensor in, tensor out: read and written in place) and from host numpy arrays (upload, kernels,
download); and, from one `rocprofv3 --kernel-trace --stats` run of the same workload, per-kernel times and
rectify_kernel's HBM bytes / time against the measured achievable 6.29 TB/s (MI355X_MICROARCH.md).

    python tools/gpu_rectify_rate.py [--out profiles/rectify_rate.json] [--reps 5] [--no-profile]

The profiled pass is a child process (`--inner`) started under rocprofv3; its kernel statistics are read back here.
The gyro is synth.make_gyro's (up to 2 rad/s), the readout 11.11 ms, the lens synth.LENS scaled to the frame.
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

SIZES = [(1352, 760), (2704, 1520), (3840, 2160)]
BATCH = 16
HBM_ACHIEVABLE = 6.29e12
KERNELS = ("rectify_rays_kernel", "rectify_rows_kernel", "rectify_kernel", "rectify_points_kernel")


def lens_of(w, h):
    from rssync_amd import synth
    ro, fx, fy, cx, cy = synth.LENS[:5]
    return (ro, fx * w / synth.IMAGE_COLS, fy * h / synth.IMAGE_ROWS, cx * w / synth.IMAGE_COLS, cy * h / synth.IMAGE_ROWS) + \
        tuple(synth.LENS[5:])


def frames_of(w, h, n=BATCH, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w), dtype=np.uint8)


def problem():
    import rssync_amd
    from rssync_amd import synth
    gyro = synth.make_gyro(1.0, 1.0 + (BATCH + 2) / synth.FPS, seed=77)
    p = rssync_amd.SyncProblem(seed=1)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p, 1.0 + np.arange(BATCH) / synth.FPS, synth.D_TRUE


def kernel_bytes(w, h):
    """bytes rectify_kernel moves through HBM per frame: a 16 B ray per pixel, the frame read once (the four byte gathers
    of neighbouring pixels overlap and are served by the caches), one byte stored; the (h + 1) x 36 B table is noise"""
    return w * h * (16 + 1 + 1) + (h + 1) * 36


def table_bytes_requested(w, h, iterations=3):
    """what the lanes ask of the row table per frame: two 36 B entries per pixel and iteration -- the lanes of a wave ask for
    the same two or three entries, so this is broadcast traffic out of L2 / L1, not HBM"""
    return w * h * iterations * 72


def inner():
    """the workload the profiler sees: one host and one device batch per size"""
    import torch
    p, times, delay = problem()
    for w, h in SIZES:
        f = frames_of(w, h)
        p.rectify_frames(f, times, lens_of(w, h), delay)
        p.rectify_frames(torch.from_numpy(f).to("cuda:0"), times, lens_of(w, h), delay)
    torch.cuda.synchronize()


def kernel_stats(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    stats = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            for key in KERNELS:
                if key + "<" in row["Name"] or key + "(" in row["Name"] or row["Name"].endswith(key):
                    s = stats.setdefault(key, {"calls": 0, "total_ns": 0.0})
                    s["calls"] += int(row["Calls"])
                    s["total_ns"] += float(row["TotalDurationNs"])
    return stats


def median_time(fn, reps):
    fn()                                                             # warm-up (buffers, code object, the ray map)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                         # returns after the device synchronise
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--inner", action="store_true")
    a = ap.parse_args()
    if a.inner:
        inner()
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    p, times, delay = problem()
    res = {"batch_frames": BATCH, "iterations": 3, "readout_s": lens_of(8, 8)[0], "sizes": []}
    for w, h in SIZES:
        f, lens = frames_of(w, h), lens_of(w, h)
        row = {"width": w, "height": h, "frame_bytes": w * h, "kernel_hbm_bytes_per_frame": kernel_bytes(w, h),
               "table_bytes_requested_per_frame": table_bytes_requested(w, h)}
        dev = torch.from_numpy(f).to("cuda:0")
        out = torch.empty_like(dev)
        row["device_tensor_s"] = median_time(lambda: p.rectify_frames(dev, times, lens, delay, out=out), a.reps)
        row["device_tensor_fps"] = BATCH / row["device_tensor_s"]
        row["device_tensor_us_per_frame"] = 1e6 * row["device_tensor_s"] / BATCH
        host_out = np.empty_like(f)
        row["host_numpy_s"] = median_time(lambda: p.rectify_frames(f, times, lens, delay, out=host_out), a.reps)
        row["host_numpy_fps"] = BATCH / row["host_numpy_s"]
        row["host_numpy_GBps_each_way"] = f.nbytes / row["host_numpy_s"] / 1e9
        assert np.array_equal(host_out, out.cpu().numpy())
        row["map_s"] = median_time(lambda: p.rectify_map(w, h, lens, times[0], delay), a.reps)
        res["sizes"].append(row)
        del dev, out
        print(json.dumps(row), flush=True)
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "rectify", "--", sys.executable,
                   os.path.abspath(__file__), "--inner"]
            rc = subprocess.run(cmd, cwd=ROOT, timeout=600).returncode
            stats = kernel_stats(d) if rc == 0 else None
        res["rocprofv3_rc"] = rc
        if stats:
            res["kernels"] = stats
            # the profiled pass: every size twice (host + device batch)
            kb = sum(2 * BATCH * kernel_bytes(w, h) for w, h in SIZES)
            ns = stats.get("rectify_kernel", {}).get("total_ns", 0.0)
            if ns:
                res["rectify_kernel_hbm_bytes_per_s"] = kb / (ns * 1e-9)
                res["rectify_kernel_of_hbm_achievable"] = res["rectify_kernel_hbm_bytes_per_s"] / HBM_ACHIEVABLE
                res["rectify_kernel_ns_per_megapixel"] = ns / (sum(2 * BATCH * w * h for w, h in SIZES) / 1e6)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "sizes"}, indent=1))


if __name__ == "__main__":
    main()
