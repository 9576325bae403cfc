"""What the bicubic sampler costs on the GPU (include/rssync_stabilize.h "Sampling", csrc/kernels/resample.hpp):
device-resident frames per second for GRAY8, NV12, RGBA32 and P010 at 1920 x 1080 and 3840 x 2160 -- batches of 8 frames
along the path at sigma 0.1 s, the lens's camera at the input's size -- with FILTER_BILINEAR beside FILTER_BICUBIC in the
same process on the same frames, and the ratio bicubic / bilinear of the frame rates.

    python tools/gpu_resample_rate.py [--out profiles/resample_rate.json] [--reps 5]

No ratio is a target: sixteen taps instead of four on kernels whose map evaluation is the same either way.  The frames are
noise (the taps' worst case for the caches is the map's geometry, which does not depend on the content).  Two alternating
rounds of each kind, the mean of each kind's two medians; the rounds' spread is the noise the ratios are read against.  The
gyro is synth.make_gyro's (up to 2 rad/s), the readout 11.11 ms, the lens synth.LENS scaled to the frame.
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
BATCH = 8
SIGMA = 0.1


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
    fn()                                                             # warm-up (buffers, code object, the ray maps)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                         # returns after the device synchronise
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import color, stabilize
    p, times, delay = problem()
    res = {"batch_frames": BATCH, "sigma_s": SIGMA, "iterations": 3, "camera": "lens", "rows": []}
    rng = np.random.default_rng(0)

    def dev(*shape, top=256, dtype=np.uint8, shift=0):
        a_ = rng.integers(0, top, size=shape, dtype=dtype)
        return torch.from_numpy(a_ << shift if shift else a_).to("cuda:0")

    for w, h in SIZES:
        lens = lens_of(w, h)
        y, uv, rgba = dev(BATCH, h, w), dev(BATCH, h // 2, w // 2, 2), dev(BATCH, h, w, 4)
        y10 = dev(BATCH, h, w, top=1024, dtype=np.uint16, shift=6)
        uv10 = dev(BATCH, h // 2, w // 2, 2, top=1024, dtype=np.uint16, shift=6)
        inputs = {"gray8": (color.GRAY8, y), "nv12": (color.NV12, (y, uv)), "rgba32": (color.RGBA32, rgba), "p010": (color.P010, (y10, uv10))}
        row = {"width": w, "height": h}
        for name, (fmt, frames) in inputs.items():
            planes = [frames] if isinstance(frames, torch.Tensor) else list(frames)
            outs = [torch.empty_like(t) for t in planes]
            out = outs[0] if len(outs) == 1 else tuple(outs)

            def run(flt, fmt=fmt, frames=frames, out=out):
                return p.stabilize_color(fmt, frames, times, lens, delay, out=out, sigma=SIGMA, filter=flt)

            # the two filters see the same map: the same pixels are filled, and the pictures differ
            _, n_lin = run(stabilize.FILTER_BILINEAR)
            lin0 = outs[0].clone()
            _, n_cub = run(stabilize.FILTER_BICUBIC)
            assert (n_lin == n_cub).all() and bool((lin0 != outs[0]).any()), name
            del lin0
            secs = {"bilinear": [], "bicubic": []}
            for _ in range(2):
                for kind, flt in (("bilinear", stabilize.FILTER_BILINEAR), ("bicubic", stabilize.FILTER_BICUBIC)):
                    secs[kind].append(median_time(lambda flt=flt: run(flt), a.reps))
            for kind in secs:
                s = float(np.mean(secs[kind]))
                row["%s_%s_s" % (name, kind)] = s
                row["%s_%s_fps" % (name, kind)] = BATCH / s
                row["%s_%s_round_spread" % (name, kind)] = abs(secs[kind][0] - secs[kind][1]) / s
            row[name + "_bicubic_over_bilinear"] = row[name + "_bicubic_fps"] / row[name + "_bilinear_fps"]
            del outs, out
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del y, uv, rgba, y10, uv10, inputs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
