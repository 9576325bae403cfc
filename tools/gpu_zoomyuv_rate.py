"""What the dynamic zoom costs for 4:2:2 and 4:4:4 video on the GPU (include/rssync_zoomyuv.h, csrc/kernels/zoomyuv.hpp), at
1920 x 1080 and 3840 x 2160, in tools/gpu_colorzoom_rate.py's method:

  render  frames per second of rssync_zoomyuv_stabilize beside rssync_yuv_stabilize at one zoom, on the same
          device-resident batches of 8 frames: NV16, P210 and I444, both cameras, both filters.  The pinhole does the same
          arithmetic plus one load per frame; the lens's camera pays fp64 rays in place of 16-byte loads of the cached maps
          -- in a 4:2:2 format three rays per chroma sample, one for the chroma plane and two for the luma pixels under it
          (three rays per four output samples, against 4:2:0's five per six); in a 4:4:4 format one ray per pixel (one per
          three samples).
  fit     frames per second of rssync_zoomyuv_fit (NV16) beside rssync_zoom_fit on 2048 frame times (12 steps, zooms
          1.0 .. 1.5, the path at sigma 0.2 s), both cameras: the fit is the gray fit plus a path download and a second fit
          of a border of the same height and half the width.

    python tools/gpu_zoomyuv_rate.py [--out profiles/zoomyuv_rate.json] [--reps 5]

No ratio is a target.  Every time is a host clock around a call that ends in a device synchronise, after one warm-up call
of the same shape; two alternating rounds of each kind, the mean of each kind's two medians, and the rounds' spread, which
is the noise the ratios are read against.  The frames are noise, the gyro is synth.make_gyro's (up to 2 rad/s), the readout
11.11 ms, the lens synth.LENS scaled to the frame.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_zoom_rate import BATCH, HI, LO, SIGMA, SIZES, STEPS, lens_of, problem, side_by_side  # noqa: E402

FIT_FRAMES = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zoomyuv_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import stabilize, yuv
    cameras = (("lens", stabilize.CAMERA_LENS), ("pinhole", stabilize.CAMERA_PINHOLE))
    filters = (("bilinear", stabilize.FILTER_BILINEAR), ("bicubic", stabilize.FILTER_BICUBIC))
    p, all_times, delay = problem(FIT_FRAMES)
    res = {"sigma_s": SIGMA, "iterations": 3, "render": {"batch_frames": BATCH, "rows": []},
           "fit": {"zoom_lo": LO, "zoom_hi": HI, "steps": STEPS, "frame_times": FIT_FRAMES, "rows": []}}
    rng = np.random.default_rng(0)
    times = all_times[:BATCH]
    zooms = 1.0 + 0.01 * np.arange(BATCH)            # one zoom per frame, 1.00 .. 1.07; the constant one is 1.04

    def on_device(shape, top, shift=0):
        a_ = rng.integers(0, top + 1, size=shape, dtype=np.uint8 if top == 255 else np.uint16)
        return torch.from_numpy(a_ << shift if shift else a_).to("cuda:0")

    for w, h in SIZES:
        lens = lens_of(w, h)
        batches = {
            "nv16": (yuv.NV16, (on_device((BATCH, h, w), 255), on_device((BATCH, h, w // 2, 2), 255))),
            "p210": (yuv.P210, (on_device((BATCH, h, w), 1023, 6), on_device((BATCH, h, w // 2, 2), 1023, 6))),
            "i444": (yuv.I444, tuple(on_device((BATCH, h, w), 255) for _ in range(3))),
        }
        for fmt_name, (fmt, frames) in batches.items():
            out = tuple(torch.empty_like(t) for t in frames)
            row = {"width": w, "height": h, "format": fmt_name}
            for cam_name, cam in cameras:
                for flt_name, flt in filters:
                    kw = dict(out=out, sigma=SIGMA, camera=cam, filter=flt)
                    # equal zooms give rssync_yuv_stabilize's bytes: the two calls timed below do the same work but for the rays
                    want, _ = p.stabilize_yuv(fmt, frames, times, lens, delay, zoom=1.04, **kw)
                    want = [t.clone() for t in want]
                    got, _ = p.stabilize_yuv_zoomed(fmt, frames, times, lens, delay, [1.04] * BATCH, **kw)
                    assert all(bool((g == x).all()) for g, x in zip(got, want)), (w, h, fmt_name, cam_name, flt_name)
                    del want
                    t = side_by_side({"zoomed": lambda: p.stabilize_yuv_zoomed(fmt, frames, times, lens, delay, zooms, **kw),
                                      "constant": lambda: p.stabilize_yuv(fmt, frames, times, lens, delay, zoom=1.04, **kw)}, a.reps)
                    key = "%s_%s" % (cam_name, flt_name)
                    for kind, (s, spread) in t.items():
                        row["%s_%s_s" % (key, kind)] = s
                        row["%s_%s_fps" % (key, kind)] = BATCH / s
                        row["%s_%s_round_spread" % (key, kind)] = spread
                    row[key + "_zoomed_over_constant"] = row[key + "_zoomed_fps"] / row[key + "_constant_fps"]
            res["render"]["rows"].append(row)
            print(json.dumps(row), flush=True)
            del out
        del batches
    for w, h in SIZES:
        lens = lens_of(w, h)
        row = {"width": w, "height": h}
        for cam_name, cam in cameras:
            kw = dict(sigma=SIGMA, camera=cam)
            zc, status = p.fit_zoom_yuv(yuv.NV16, w, h, lens, all_times, delay, LO, HI, steps=STEPS, **kw)
            zl, _ = p.fit_zoom(w, h, lens, all_times, delay, LO, HI, steps=STEPS, **kw)
            row[cam_name + "_not_clear"] = int(status.sum())
            row[cam_name + "_frames_the_chroma_plane_raised"] = int((zc > zl).sum())
            got = side_by_side({"yuv": lambda: p.fit_zoom_yuv(yuv.NV16, w, h, lens, all_times, delay, LO, HI, steps=STEPS, **kw),
                                "gray": lambda: p.fit_zoom(w, h, lens, all_times, delay, LO, HI, steps=STEPS, **kw)}, a.reps)
            for kind, (s, spread) in got.items():
                row["%s_%s_s" % (cam_name, kind)] = s
                row["%s_%s_fps" % (cam_name, kind)] = FIT_FRAMES / s
                row["%s_%s_round_spread" % (cam_name, kind)] = spread
            row[cam_name + "_yuv_over_gray"] = row[cam_name + "_yuv_fps"] / row[cam_name + "_gray_fps"]
        res["fit"]["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
