"""Stabiliser throughput on the GPU (include/rssync_stabilize.h): stabilised frames per second at three frame sizes,
batches of 16 frames along the path at sigma 0.1 s, device-resident (tensor in, tensor out) and from host numpy arrays
(upload, kernels, download): the lens's camera at the input's size, and a pinhole camera at 1920 x 1080.  rectify_frames
runs in the same process on the same frames, so every row carries the ratio stabilised / rectified.  From one
`rocprofv3 --kernel-trace --stats` run of the same workload: per-kernel times of both.

    python tools/gpu_stabilize_rate.py [--out profiles/stabilize_rate.json] [--reps 5] [--no-profile]

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
PINHOLE_OUT = (1920, 1080)
BATCH = 16
SIGMA = 0.1
KERNELS = ("stabilize_path_kernel", "stabilize_rows_kernel", "stabilize_kernel", "stabilize_coverage_kernel", "rectify_rays_kernel",
           "rectify_rows_kernel", "rectify_kernel")


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


def inner():
    """the workload the profiler sees: per size one device batch of each of the three kinds, and one coverage sweep"""
    import torch
    from rssync_amd import stabilize
    p, times, delay = problem()
    for w, h in SIZES:
        dev, lens = torch.from_numpy(frames_of(w, h)).to("cuda:0"), lens_of(w, h)
        p.rectify_frames(dev, times, lens, delay)
        p.stabilize_frames(dev, times, lens, delay, sigma=SIGMA)
        p.stabilize_frames(dev, times, lens, delay, sigma=SIGMA, camera=stabilize.CAMERA_PINHOLE, out_size=PINHOLE_OUT)
        p.stabilize_coverage(w, h, lens, times, delay, [1.0 + 0.02 * k for k in range(16)], sigma=SIGMA)
    torch.cuda.synchronize()


def kernel_stats(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    stats = {"by_name": {}}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            if "stabilize_" in row["Name"] or "rectify_" in row["Name"]:   # every instantiation under its full name
                stats["by_name"][row["Name"]] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"])}
            for key in KERNELS:
                if key + "<" in row["Name"] or key + "(" in row["Name"] or row["Name"].endswith(key):
                    s = stats.setdefault(key, {"calls": 0, "total_ns": 0.0})
                    s["calls"] += int(row["Calls"])
                    s["total_ns"] += float(row["TotalDurationNs"])
    # ... and every dispatch of them in launch order (inner() goes through SIZES in order): what a kind costs at each size
    traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if traces:
        rows = []
        with open(traces[0]) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                if "stabilize_" in name or "rectify_" in name:
                    short = name.split("(anonymous namespace)::")[1].split("(")[0] if "(anonymous namespace)::" in name else name
                    rows.append((int(row["Start_Timestamp"]), short, int(row["End_Timestamp"]) - int(row["Start_Timestamp"]),
                                 [int(row.get("Grid_Size_X", 0)), int(row.get("Grid_Size_Y", 0)), int(row.get("Grid_Size_Z", 0))]))
        stats["dispatches"] = [{"kernel": n, "ns": d, "grid": g} for _, n, d, g in sorted(rows)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stabilize_rate.json"))
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
    from rssync_amd import stabilize
    p, times, delay = problem()
    res = {"batch_frames": BATCH, "sigma_s": SIGMA, "iterations": 3, "readout_s": lens_of(8, 8)[0], "pinhole_out": list(PINHOLE_OUT),
           "sizes": []}
    pw, ph = PINHOLE_OUT
    for w, h in SIZES:
        f, lens = frames_of(w, h), lens_of(w, h)
        row = {"width": w, "height": h, "frame_bytes": w * h}
        dev = torch.from_numpy(f).to("cuda:0")
        out = torch.empty_like(dev)
        pin = torch.empty((BATCH, ph, pw), dtype=torch.uint8, device="cuda:0")
        host_out, host_pin = np.empty_like(f), np.empty((BATCH, ph, pw), np.uint8)
        runs = {
            "rectify_device": lambda: p.rectify_frames(dev, times, lens, delay, out=out),
            "lens_device": lambda: p.stabilize_frames(dev, times, lens, delay, sigma=SIGMA, out=out),
            "pinhole_device": lambda: p.stabilize_frames(dev, times, lens, delay, sigma=SIGMA, camera=stabilize.CAMERA_PINHOLE,
                                                         out_size=PINHOLE_OUT, out=pin),
            "rectify_host": lambda: p.rectify_frames(f, times, lens, delay, out=host_out),
            "lens_host": lambda: p.stabilize_frames(f, times, lens, delay, sigma=SIGMA, out=host_out),
            "pinhole_host": lambda: p.stabilize_frames(f, times, lens, delay, sigma=SIGMA, camera=stabilize.CAMERA_PINHOLE,
                                                       out_size=PINHOLE_OUT, out=host_pin),
        }
        # two alternating rounds, the mean of each kind's two medians: the kinds share whatever else the host is doing
        secs = {k: [] for k in runs}
        for _ in range(2):
            for k, fn in runs.items():
                secs[k].append(median_time(fn, a.reps))
        for k in runs:
            s = float(np.mean(secs[k]))
            row[k + "_s"] = s
            row[k + "_fps"] = BATCH / s
            row[k + "_us_per_frame"] = 1e6 * s / BATCH
        assert np.array_equal(host_pin, pin.cpu().numpy())
        for kind in ("device", "host"):
            row["lens_over_rectify_" + kind] = row["lens_%s_fps" % kind] / row["rectify_%s_fps" % kind]
            row["pinhole_over_rectify_" + kind] = row["pinhole_%s_fps" % kind] / row["rectify_%s_fps" % kind]
        zooms = [1.0 + 0.02 * k for k in range(16)]
        row["coverage_16_zooms_s"] = median_time(lambda: p.stabilize_coverage(w, h, lens, times, delay, zooms, sigma=SIGMA), a.reps)
        row["path_s"] = median_time(lambda: p.stabilize_path(times, lens[0], delay, SIGMA), a.reps)
        res["sizes"].append(row)
        del dev, out, pin
        print(json.dumps(row), flush=True)
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "stabilize", "--", sys.executable,
                   os.path.abspath(__file__), "--inner"]
            rc = subprocess.run(cmd, cwd=ROOT, timeout=600).returncode
            stats = kernel_stats(d) if rc == 0 else None
        res["rocprofv3_rc"] = rc
        if stats:
            res["kernels"] = stats
            # the profiled pass: per size one batch through rectify_kernel, one through stabilize_kernel at the same size
            # and one at the pinhole's size
            same = sum(BATCH * w * h for w, h in SIZES) / 1e6
            both = same + len(SIZES) * BATCH * pw * ph / 1e6
            if stats.get("rectify_kernel", {}).get("total_ns"):
                res["rectify_kernel_ns_per_output_megapixel"] = stats["rectify_kernel"]["total_ns"] / same
            if stats.get("stabilize_kernel", {}).get("total_ns"):
                res["stabilize_kernel_ns_per_output_megapixel"] = stats["stabilize_kernel"]["total_ns"] / both
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "sizes"}, indent=1))


if __name__ == "__main__":
    main()
