"""What the path limiter's fit costs on the GPU (include/rssync_limit.h, csrc/kernels/limit.hpp), at 1920 x 1080 and
3840 x 2160:

  fit       frames per second of rssync_limit_fit (12 steps, the path at sigma 0.2 s) on 2048 frame times, with the lens's
            camera and with a pinhole, beside rssync_zoom_fit on the same times and steps in the same process.  The zoom fit
            is the yardstick: its kernel maps the same border once per candidate against a row table that a kernel in front
            of it built once; the limiter's kernel rebuilds the table for every candidate.  The limiter's zoom is, per size
            and camera, the one of LIMIT_ZOOMS at which most frames take the full bisection; each branch's share (goal
            clear, bisected, not clear) is recorded, as are the zoom fit's own.
  variants  not measured here: the section "variants" of the output file is carried over as it stands.  It records the fit
            through the internal launcher for the product's kernel -- which keeps the border's rays between the candidates
            of a frame and computes the rows' orientations again for each -- and for the three builds that chose otherwise
            (orientations kept as well; rays computed again as well; orientations kept and rays computed again), each in
            a process of its own, when the two choices were made.  The kernel code of the other three was removed after
            the measurement (csrc/kernels/limit.hpp says what they were).

    python tools/gpu_limit_rate.py [--out profiles/limit_rate.json] [--reps 5]

No ratio is a target.  Every time is a host clock around a call that ends in a device synchronise, after one warm-up call
of the same shape; two alternating rounds of each kind, the mean of each kind's two medians, and the rounds' spread, which
is the noise the ratios are read against.  The gyro is synth.make_gyro's (up to 2 rad/s), the readout 11.11 ms, the lens
synth.LENS scaled to the frame.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_zoom_rate import lens_of, problem, side_by_side  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]
N_FRAMES = 2048
SIGMA = 0.2
STEPS = 12
ZOOM_LO, ZOOM_HI = 1.0, 1.5                      # the zoom fit's bounds (tools/gpu_zoom_rate.py)
LIMIT_ZOOMS = {"lens": (1.02, 1.05, 1.1, 1.2), "pinhole": (0.9, 1.0, 1.1, 1.2)}  # the limiter's zoom: of these the one at which most frames bisect


def shares(strengths, status):
    n = float(len(strengths))
    return {"goal_clear": float((strengths == 1).sum()) / n, "bisected": float(((status == 0) & (strengths < 1)).sum()) / n,
            "not_clear": float((status == 1).sum()) / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limit_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import stabilize
    p, times, delay = problem(N_FRAMES)
    res = {"sigma_s": SIGMA, "iterations": 3, "steps": STEPS, "frame_times": N_FRAMES, "zoom_fit": {"zoom_lo": ZOOM_LO, "zoom_hi": ZOOM_HI},
           "fit": []}
    for w, h in SIZES:
        lens = lens_of(w, h)
        for cam_name, cam in (("lens", stabilize.CAMERA_LENS), ("pinhole", stabilize.CAMERA_PINHOLE)):
            kw = dict(sigma=SIGMA, camera=cam)
            tried = {z: shares(*p.fit_strength(w, h, lens, times, delay, zoom=z, steps=STEPS, **kw)) for z in LIMIT_ZOOMS[cam_name]}
            z = max(tried, key=lambda v: tried[v]["bisected"])
            zooms, zstatus = p.fit_zoom(w, h, lens, times, delay, ZOOM_LO, ZOOM_HI, steps=STEPS, **kw)
            row = {"width": w, "height": h, "camera": cam_name, "limit_zoom": z, "limit_shares": tried[z],
                   "zoom_fit_shares": {"at_lo": float((zooms == ZOOM_LO).mean()), "bisected": float(((zstatus == 0) & (zooms > ZOOM_LO)).mean()),
                                       "not_clear": float((zstatus == 1).mean())}}
            got = side_by_side({"limit_fit": lambda: p.fit_strength(w, h, lens, times, delay, zoom=z, steps=STEPS, **kw),
                                "zoom_fit": lambda: p.fit_zoom(w, h, lens, times, delay, ZOOM_LO, ZOOM_HI, steps=STEPS, **kw)}, a.reps)
            for kind, (s, spread) in got.items():
                row[kind + "_s"] = s
                row[kind + "_fps"] = N_FRAMES / s
                row[kind + "_round_spread"] = spread
            row["limit_over_zoom_fps"] = row["limit_fit_fps"] / row["zoom_fit_fps"]
            res["fit"].append(row)
            print(json.dumps(row), flush=True)
    if os.path.exists(a.out):                        # the recorded choice between the kernel's variants (see above)
        with open(a.out) as fh:
            old = json.load(fh)
        for key in ("variants", "variants_note"):
            if key in old:
                res[key] = old[key]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
