"""What the infill costs on the GPU (include/rssync_infill.h, csrc/kernels/infill.hpp), at 1920 x 1080 and 3840 x 2160, on
device-resident batches of 8 frames, both cameras, both filters, radius 1, 2 and 4.  Frames per second of

  infill       rssync_infill_stabilize;
  plain        rssync_stabilize_frames on the same frames: what the borders cost when they are filled with a constant;
  composition  what a caller did before: per output frame one rssync_stabilize_frames call per candidate (2 radius + 1 of
               them, fewer at the ends of the batch) on that candidate alone with the frame's target, results left on the
               device, WITHOUT the merge of the renders -- a lower bound on what the composition costs.

    python tools/gpu_infill_rate.py [--out profiles/infill_rate.json] [--reps 5]

The one gate: the infill must be faster than the composition in every row (the tool exits non-zero where it is not, after
writing the file).  infill / plain is recorded, not gated.  Every time is a host clock around calls that end in a device
synchronise, after one warm-up of the same shape; two alternating rounds of each kind, the mean of each kind's two medians,
and the rounds' spread, which is the noise the ratios are read against.  The frames are noise, the gyro is
synth.make_gyro's (up to 2 rad/s), the targets the path at sigma 0.2 s passed explicitly to all three, zoom 1, the readout
11.11 ms, the lens synth.LENS scaled to the frame; the share of pixels outside their own frame is recorded per row.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_zoom_rate import BATCH, SIGMA, SIZES, lens_of, problem, side_by_side  # noqa: E402

RADII = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infill_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import infill, stabilize
    p, times, delay = problem(64)
    times = times[:BATCH]
    res = {"sigma_s": SIGMA, "iterations": 3, "zoom": 1.0, "batch_frames": BATCH, "rows": []}
    rng = np.random.default_rng(0)
    slower = []
    for w, h in SIZES:
        lens = lens_of(w, h)
        targets = p.stabilize_path(times, lens[0], delay, SIGMA)
        frames = torch.from_numpy(rng.integers(0, 256, size=(BATCH, h, w), dtype=np.uint8)).to("cuda:0")
        out = torch.empty_like(frames)
        one = torch.empty_like(frames[:1])
        for cam_name, cam in (("lens", stabilize.CAMERA_LENS), ("pinhole", stabilize.CAMERA_PINHOLE)):
            for flt_name, flt in (("bilinear", stabilize.FILTER_BILINEAR), ("bicubic", stabilize.FILTER_BICUBIC)):
                kw = dict(camera=cam, filter=flt)
                for radius in RADII:
                    cand = [infill.candidates(f, BATCH, radius) for f in range(BATCH)]

                    def composition():
                        for f in range(BATCH):
                            for g in cand[f]:
                                p.stabilize_frames(frames[g:g + 1], times[g:g + 1], lens, delay, targets=targets[f:f + 1], out=one, **kw)

                    _, n_out, n_lent = p.stabilize_frames_infilled(frames, times, lens, delay, radius, targets=targets, out=out, **kw)
                    _, n_plain = p.stabilize_frames(frames, times, lens, delay, targets=targets, out=out, **kw)
                    assert ((n_out + n_lent) == n_plain).all()
                    t = side_by_side({"infill": lambda: p.stabilize_frames_infilled(frames, times, lens, delay, radius, targets=targets,
                                                                                   out=out, **kw),
                                      "plain": lambda: p.stabilize_frames(frames, times, lens, delay, targets=targets, out=out, **kw),
                                      "composition": composition}, a.reps)
                    row = {"width": w, "height": h, "camera": cam_name, "filter": flt_name, "radius": radius,
                           "calls_of_the_composition": sum(len(c) for c in cand),
                           "outside_share": float(n_plain.sum()) / (BATCH * w * h), "borrowed_share": float(n_lent.sum()) / (BATCH * w * h)}
                    for kind, (s, spread) in t.items():
                        row[kind + "_s"] = s
                        row[kind + "_fps"] = BATCH / s
                        row[kind + "_round_spread"] = spread
                    row["infill_over_plain"] = row["infill_fps"] / row["plain_fps"]
                    row["infill_over_composition"] = row["infill_fps"] / row["composition_fps"]
                    if not row["infill_fps"] > row["composition_fps"]:
                        slower.append(row)
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
        del frames, out, one
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    if slower:
        raise SystemExit("the infill is not faster than the composition in %d rows" % len(slower))


if __name__ == "__main__":
    main()
