"""Colour stabiliser throughput on the GPU (include/rssync_color.h): device-resident frames per second for NV12, I420 and
RGBA32 at 1920 x 1080 and 3840 x 2160 -- batches of 8 frames along the path at sigma 0.1 s, the lens's camera at the
input's size and a pinhole camera at 1920 x 1080 -- and, in the same process on the same frames, what the gray
stabiliser alone can do: ``stabilize_frames`` on Y, and "three gray calls" over Y, U and V with the chroma lens, the chroma
frame times and the chroma output camera (the result the fused I420 call gives, byte for byte).

    python tools/gpu_color_rate.py [--out profiles/color_rate.json] [--reps 5]

Every row carries the ratios fused I420 / three gray calls (the condition: above 1), NV12 / I420 (within the run-to-run
noise of 1, which the two alternating rounds of each kind show) and I420 / gray Y.  The gyro is synth.make_gyro's (up to
2 rad/s), the readout 11.11 ms, the lens synth.LENS scaled to the frame.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import color, stabilize
    p, times, delay = problem()
    res = {"batch_frames": BATCH, "sigma_s": SIGMA, "iterations": 3, "chroma_site": "center", "pinhole_out": list(PINHOLE_OUT), "rows": []}
    rng = np.random.default_rng(0)

    def dev(*shape):
        return torch.from_numpy(rng.integers(0, 256, size=shape, dtype=np.uint8)).to("cuda:0")

    def empty(*shape):
        return torch.empty(shape, dtype=torch.uint8, device="cuda:0")

    for w, h in SIZES:
        lens = lens_of(w, h)
        y, u, v, rgba = dev(BATCH, h, w), dev(BATCH, h // 2, w // 2), dev(BATCH, h // 2, w // 2), dev(BATCH, h, w, 4)
        uv = torch.stack([u, v], dim=-1).contiguous()
        for camera, (ow, oh) in ((stabilize.CAMERA_LENS, (w, h)), (stabilize.CAMERA_PINHOLE, PINHOLE_OUT)):
            if camera == stabilize.CAMERA_PINHOLE and (w, h) != (1920, 1080):
                continue
            kw = dict(sigma=SIGMA, camera=camera, out_size=(ow, oh))
            lens_c, cam_c, dt = color.chroma_config(lens, w, h, ow, oh)
            ckw = dict(camera=camera, out_size=(ow // 2, oh // 2), out_camera=cam_c, fill=128)
            targets = p.stabilize_path(times, lens[0], delay, SIGMA)            # (the three calls share the luma's path)
            oy_, ou, ov = empty(BATCH, oh, ow), empty(BATCH, oh // 2, ow // 2), empty(BATCH, oh // 2, ow // 2)
            ouv, orgba = empty(BATCH, oh // 2, ow // 2, 2), empty(BATCH, oh, ow, 4)

            def three_gray():
                p.stabilize_frames(y, times, lens, delay, out=oy_, **kw)
                p.stabilize_frames(u, times + dt, lens_c, delay, targets=targets, out=ou, **ckw)
                p.stabilize_frames(v, times + dt, lens_c, delay, targets=targets, out=ov, **ckw)

            runs = {
                "gray_y": lambda: p.stabilize_frames(y, times, lens, delay, out=oy_, **kw),
                "three_gray": three_gray,
                "i420": lambda: p.stabilize_color(color.I420, (y, u, v), times, lens, delay, out=(oy_, ou, ov), **kw),
                "nv12": lambda: p.stabilize_color(color.NV12, (y, uv), times, lens, delay, out=(oy_, ouv), **kw),
                "rgba32": lambda: p.stabilize_color(color.RGBA32, rgba, times, lens, delay, out=orgba, **kw),
            }
            # the fused call computes what the three calls compute: checked once, before anything is timed
            three_gray()
            want = [t.clone() for t in (oy_, ou, ov)]
            runs["i420"]()
            # (the three calls' targets pass through the library's normalisation once more: a target may move by an ulp)
            worst = max(int((a_.int() - b_.int()).abs().max()) for a_, b_ in zip(want, (oy_, ou, ov)))
            assert worst <= 1, "fused I420 differs from the three gray calls by %d grey levels" % worst
            # two alternating rounds, the mean of each kind's two medians; the rounds' spread is the noise the ratios are read against
            secs = {k: [] for k in runs}
            for _ in range(2):
                for k, fn in runs.items():
                    secs[k].append(median_time(fn, a.reps))
            row = {"width": w, "height": h, "out_width": ow, "out_height": oh, "camera": "lens" if camera == stabilize.CAMERA_LENS else "pinhole",
                   "i420_against_three_gray_grey_levels": worst}
            for k in runs:
                s = float(np.mean(secs[k]))
                row[k + "_s"] = s
                row[k + "_fps"] = BATCH / s
                row[k + "_round_spread"] = abs(secs[k][0] - secs[k][1]) / s
            row["i420_over_three_gray"] = row["i420_fps"] / row["three_gray_fps"]
            row["nv12_over_i420"] = row["nv12_fps"] / row["i420_fps"]
            row["i420_over_gray_y"] = row["i420_fps"] / row["gray_y_fps"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del y, u, v, uv, rgba
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
