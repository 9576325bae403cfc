"""4:2:2 and 4:4:4 stabiliser throughput on the GPU (include/rssync_yuv.h): device-resident frames per second for NV16, P210
and I444 at 1920 x 1080 and 3840 x 2160 -- batches of 8 frames along the path at sigma 0.1 s, the lens's camera at the
input's size and a pinhole camera at 1920 x 1080, both samplers -- and, in the same process on the same geometry, NV12
and P010 (include/rssync_color.h, rssync_color16.h) and what the gray stabiliser alone can do for the 8-bit formats: three
``stabilize_frames`` calls over Y, U and V with their cameras.  Before anything is timed the tool asserts that the fused
call's planes lie within 1 grey level of the three calls' (their targets pass through the library's normalisation once
more, so a target may move by an ulp; the tests compare byte for byte on identical targets) and records the largest
difference it saw.

    python tools/gpu_yuv_rate.py [--out profiles/yuv_rate.json] [--reps 5]

The method is tools/gpu_color_rate.py's: host clocks around calls that end in a device synchronise, one warm-up call, two
alternating rounds of each kind whose spread is the noise the ratios are read against.  Every ratio is recorded and none
is gated.  The gyro is synth.make_gyro's (up to 2 rad/s), the readout 11.11 ms, the lens synth.LENS scaled to the frame.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_color_rate import BATCH, PINHOLE_OUT, SIGMA, SIZES, lens_of, median_time, problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import color, stabilize, yuv
    p, times, delay = problem()
    res = {"batch_frames": BATCH, "sigma_s": SIGMA, "iterations": 3, "chroma_site": "center", "pinhole_out": list(PINHOLE_OUT), "rows": []}
    rng = np.random.default_rng(0)

    def dev(*shape, top=256, dtype=np.uint8, shift=0):
        return torch.from_numpy(rng.integers(0, top, size=shape).astype(dtype) << shift).to("cuda:0")

    def empty(*shape, dtype=torch.uint8):
        return torch.empty(shape, dtype=dtype, device="cuda:0")

    for w, h in SIZES:
        lens = lens_of(w, h)
        y, u2, v2, u4, v4 = dev(BATCH, h, w), dev(BATCH, h, w // 2), dev(BATCH, h, w // 2), dev(BATCH, h, w), dev(BATCH, h, w)
        uv2 = torch.stack([u2, v2], dim=-1).contiguous()
        uv0 = dev(BATCH, h // 2, w // 2, 2)
        y10 = dev(BATCH, h, w, top=1024, dtype=np.uint16, shift=6)
        uv10_2 = dev(BATCH, h, w // 2, 2, top=1024, dtype=np.uint16, shift=6)
        uv10_0 = dev(BATCH, h // 2, w // 2, 2, top=1024, dtype=np.uint16, shift=6)
        for camera, (ow, oh) in ((stabilize.CAMERA_LENS, (w, h)), (stabilize.CAMERA_PINHOLE, PINHOLE_OUT)):
            if camera == stabilize.CAMERA_PINHOLE and (w, h) != (1920, 1080):
                continue
            lens_c, cam_c = yuv.chroma_config(lens, w, h, ow, oh)
            targets = p.stabilize_path(times, lens[0], delay, SIGMA)            # (the three calls share the luma's path)
            oy_, ou2, ov2, ou4, ov4 = empty(BATCH, oh, ow), empty(BATCH, oh, ow // 2), empty(BATCH, oh, ow // 2), empty(BATCH, oh, ow), empty(BATCH, oh, ow)
            ouv2, ouv0 = empty(BATCH, oh, ow // 2, 2), empty(BATCH, oh // 2, ow // 2, 2)
            oy10 = empty(BATCH, oh, ow, dtype=torch.uint16)
            ouv10_2, ouv10_0 = empty(BATCH, oh, ow // 2, 2, dtype=torch.uint16), empty(BATCH, oh // 2, ow // 2, 2, dtype=torch.uint16)
            for filt in (stabilize.FILTER_BILINEAR, stabilize.FILTER_BICUBIC):
                kw = dict(sigma=SIGMA, camera=camera, out_size=(ow, oh), filter=filt)
                ckw = dict(camera=camera, out_size=(ow // 2, oh), out_camera=cam_c, fill=128, filter=filt)

                def three_gray_422():
                    p.stabilize_frames(y, times, lens, delay, out=oy_, **kw)
                    p.stabilize_frames(u2, times, lens_c, delay, targets=targets, out=ou2, **ckw)
                    p.stabilize_frames(v2, times, lens_c, delay, targets=targets, out=ov2, **ckw)

                def three_gray_444():
                    p.stabilize_frames(y, times, lens, delay, out=oy_, **kw)
                    p.stabilize_frames(u4, times, lens, delay, targets=targets, out=ou4, fill=128, **kw)
                    p.stabilize_frames(v4, times, lens, delay, targets=targets, out=ov4, fill=128, **kw)

                runs = {
                    "three_gray_422": three_gray_422,
                    "three_gray_444": three_gray_444,
                    "nv16": lambda: p.stabilize_yuv(yuv.NV16, (y, uv2), times, lens, delay, out=(oy_, ouv2), **kw),
                    "p210": lambda: p.stabilize_yuv(yuv.P210, (y10, uv10_2), times, lens, delay, out=(oy10, ouv10_2), **kw),
                    "i444": lambda: p.stabilize_yuv(yuv.I444, (y, u4, v4), times, lens, delay, out=(oy_, ou4, ov4), **kw),
                    "nv12": lambda: p.stabilize_color(color.NV12, (y, uv0), times, lens, delay, out=(oy_, ouv0), **kw),
                    "p010": lambda: p.stabilize_color(color.P010, (y10, uv10_0), times, lens, delay, out=(oy10, ouv10_0), **kw),
                }
                # the fused calls compute what the three calls compute: checked once, before anything is timed
                three_gray_422()
                want = [t.clone() for t in (oy_, ou2, ov2)]
                runs["nv16"]()
                # (the three calls' targets pass through the library's normalisation once more: a target may move by an ulp)
                worst = max(int((a_.int() - b_.int()).abs().max()) for a_, b_ in zip(want, (oy_, ouv2[..., 0], ouv2[..., 1])))
                assert worst <= 1, "fused NV16 differs from the three gray calls by %d grey levels" % worst
                three_gray_444()
                want = [t.clone() for t in (oy_, ou4, ov4)]
                runs["i444"]()
                worst4 = max(int((a_.int() - b_.int()).abs().max()) for a_, b_ in zip(want, (oy_, ou4, ov4)))
                assert worst4 <= 1, "fused I444 differs from the three gray calls by %d grey levels" % worst4
                secs = {k: [] for k in runs}
                for _ in range(2):
                    for k, fn in runs.items():
                        secs[k].append(median_time(fn, a.reps))
                row = {"width": w, "height": h, "out_width": ow, "out_height": oh, "camera": "lens" if camera == stabilize.CAMERA_LENS else "pinhole",
                       "filter": "bicubic" if filt else "bilinear", "nv16_against_three_gray_grey_levels": worst,
                       "i444_against_three_gray_grey_levels": worst4}
                for k in runs:
                    s = float(np.mean(secs[k]))
                    row[k + "_s"] = s
                    row[k + "_fps"] = BATCH / s
                    row[k + "_round_spread"] = abs(secs[k][0] - secs[k][1]) / s
                row["nv16_over_three_gray_422"] = row["nv16_fps"] / row["three_gray_422_fps"]
                row["i444_over_three_gray_444"] = row["i444_fps"] / row["three_gray_444_fps"]
                row["nv16_over_nv12"] = row["nv16_fps"] / row["nv12_fps"]
                row["i444_over_nv12"] = row["i444_fps"] / row["nv12_fps"]
                row["p210_over_p010"] = row["p210_fps"] / row["p010_fps"]
                row["p210_over_nv16"] = row["p210_fps"] / row["nv16_fps"]
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        del y, u2, v2, u4, v4, uv2, uv0, y10, uv10_2, uv10_0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
