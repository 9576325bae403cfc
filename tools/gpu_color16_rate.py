"""Throughput of the 16-bit colour front on the GPU (include/rssync_color16.h): device-resident frames per second of P010,
I010 and GRAY16 at 1920 x 1080 and 3840 x 2160 -- batches of 8 frames along the path at sigma 0.1 s, the lens's camera at
the input's size and a pinhole camera at 1920 x 1080 -- and beside each, from the same process on the same frame times and
geometry, its 8-bit sibling: NV12, I420 and GRAY8.  The 8-bit kernels are the yardstick: a 16-bit frame moves twice the
bytes through the same map arithmetic, so a ratio of 0.5 is what bandwidth alone would give and 1 what arithmetic alone would.

    python tools/gpu_color16_rate.py [--out profiles/color16_rate.json] [--reps 5]

Every timing sample is a run of calls lasting at least 0.25 s (each call returns after the device synchronise), after a
warm-up of the same shape; a kind's figure is the mean of the medians of two alternating rounds, and the rounds' spread is the
noise the ratios are read against.  Before anything is timed the 16-bit result on the widened 8-bit frames is compared with
the 8-bit result with the same fills, byte for byte.  The gyro is synth.make_gyro's (up to 2 rad/s), the readout 11.11 ms,
the lens synth.LENS scaled to the frame.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1920, 1080), (3840, 2160)]
PINHOLE_OUT = (1920, 1080)
BATCH = 8
SIGMA = 0.1
WINDOW_S = 0.25


def lens_of(w, h):
    from rssync_amd import synth
    ro, fx, fy, cx, cy = synth.LENS[:5]
    return (ro, fx * w / synth.IMAGE_COLS, fy * h / synth.IMAGE_ROWS, cx * w / synth.IMAGE_COLS, cy * h / synth.IMAGE_ROWS) + \
        tuple(synth.LENS[5:])


def problem():
    import rssync_amd
    from rssync_amd import synth
    gyro = synth.make_gyro(1.0, 1.0 + (BATCH + 2) / synth.FPS, seed=77)
    p = rssync_amd.SyncProblem(seed=1)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p, 1.0 + np.arange(BATCH) / synth.FPS, synth.D_TRUE


def median_time(fn, reps):
    """seconds per call: the median of `reps` samples, each a run of calls of at least WINDOW_S"""
    fn()                                                             # warm-up (buffers, code object, the ray maps)
    t0 = time.perf_counter()
    fn()
    calls = max(1, int(np.ceil(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()                                                     # returns after the device synchronise
        t.append((time.perf_counter() - t0) / calls)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color16_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import color, stabilize
    p, times, delay = problem()
    res = {"batch_frames": BATCH, "sigma_s": SIGMA, "iterations": 3, "chroma_site": "center", "pinhole_out": list(PINHOLE_OUT),
           "window_s": WINDOW_S, "reps": a.reps, "rows": []}
    rng = np.random.default_rng(0)

    def pair(*shape):
        """the same 8-bit values as uint8 and widened to uint16, on the device"""
        v = rng.integers(0, 256, size=shape, dtype=np.uint8)
        return torch.from_numpy(v).to("cuda:0"), torch.from_numpy(v.astype(np.uint16)).to("cuda:0")

    def empty(dtype, *shape):
        return torch.empty(shape, dtype=dtype, device="cuda:0")

    for w, h in SIZES:
        lens = lens_of(w, h)
        (y8, y16), (u8, u16), (v8, v16) = pair(BATCH, h, w), pair(BATCH, h // 2, w // 2), pair(BATCH, h // 2, w // 2)
        uv8 = torch.stack([u8, v8], dim=-1).contiguous()
        y10 = torch.from_numpy(y16.cpu().numpy() << 6).to("cuda:0")
        uv10 = torch.from_numpy(np.stack([u16.cpu().numpy(), v16.cpu().numpy()], axis=-1) << 6).to("cuda:0")
        for camera, (ow, oh) in ((stabilize.CAMERA_LENS, (w, h)), (stabilize.CAMERA_PINHOLE, PINHOLE_OUT)):
            if camera == stabilize.CAMERA_PINHOLE and (w, h) != (1920, 1080):
                continue
            # (the same fill values on both sides: the defaults follow the depth, 128 against 512)
            kw = dict(sigma=SIGMA, camera=camera, out_size=(ow, oh), fills=(0, 128, 128))
            o8 = {"y": empty(torch.uint8, BATCH, oh, ow), "u": empty(torch.uint8, BATCH, oh // 2, ow // 2),
                  "v": empty(torch.uint8, BATCH, oh // 2, ow // 2), "uv": empty(torch.uint8, BATCH, oh // 2, ow // 2, 2)}
            o16 = {"y": empty(torch.uint16, BATCH, oh, ow), "u": empty(torch.uint16, BATCH, oh // 2, ow // 2),
                   "v": empty(torch.uint16, BATCH, oh // 2, ow // 2), "uv": empty(torch.uint16, BATCH, oh // 2, ow // 2, 2)}
            runs = {
                "nv12": lambda: p.stabilize_color(color.NV12, (y8, uv8), times, lens, delay, out=(o8["y"], o8["uv"]), **kw),
                "p010": lambda: p.stabilize_color(color.P010, (y10, uv10), times, lens, delay, out=(o16["y"], o16["uv"]), **kw),
                "i420": lambda: p.stabilize_color(color.I420, (y8, u8, v8), times, lens, delay, out=(o8["y"], o8["u"], o8["v"]), **kw),
                "i010": lambda: p.stabilize_color(color.I010, (y16, u16, v16), times, lens, delay, out=(o16["y"], o16["u"], o16["v"]), **kw),
                "gray8": lambda: p.stabilize_color(color.GRAY8, y8, times, lens, delay, out=o8["y"], **kw),
                "gray16": lambda: p.stabilize_color(color.GRAY16, y16, times, lens, delay, out=o16["y"], **kw),
            }
            # the 16-bit formats compute what their siblings compute: checked once, on the first frame, before anything is timed
            runs["nv12"]()
            want_y, want_uv = o8["y"][0].cpu().numpy().astype(np.uint16), o8["uv"][0].cpu().numpy().astype(np.uint16)

            def same(name, got, want):
                got = got[0].cpu().numpy()
                assert (got == want).all(), "%s differs from its 8-bit sibling in %d samples" % (name, int((got != want).sum()))

            runs["p010"]()
            same("P010 Y", o16["y"], want_y << 6)
            same("P010 UV", o16["uv"], want_uv << 6)
            runs["i010"]()
            same("I010 Y", o16["y"], want_y)
            same("I010 U", o16["u"], want_uv[..., 0])
            same("I010 V", o16["v"], want_uv[..., 1])
            runs["gray16"]()
            same("GRAY16", o16["y"], want_y)
            secs = {k: [] for k in runs}
            for _ in range(2):
                for k, fn in runs.items():
                    secs[k].append(median_time(fn, a.reps))
            row = {"width": w, "height": h, "out_width": ow, "out_height": oh, "camera": "lens" if camera == stabilize.CAMERA_LENS else "pinhole"}
            for k in runs:
                s = float(np.mean(secs[k]))
                row[k + "_s"] = s
                row[k + "_fps"] = BATCH / s
                row[k + "_round_spread"] = abs(secs[k][0] - secs[k][1]) / s
            row["p010_over_nv12"] = row["p010_fps"] / row["nv12_fps"]
            row["i010_over_i420"] = row["i010_fps"] / row["i420_fps"]
            row["gray16_over_gray8"] = row["gray16_fps"] / row["gray8_fps"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del y8, y16, u8, u16, v8, v16, uv8, y10, uv10
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
