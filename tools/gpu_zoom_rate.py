"""What the dynamic zoom costs on the GPU (include/rssync_zoom.h, csrc/kernels/zoom.hpp), at 1920 x 1080 and 3840 x 2160:

  fit     frames per second of rssync_zoom_fit (12 steps, zooms 1.0 .. 1.5, the path at sigma 0.2 s) on 256 and on 2048 frame
          times, with the lens's camera and with a pinhole, beside rssync_stabilize_coverage on the same times at 14 zooms:
          the same number of map evaluations per border pixel (hi, lo and twelve middles), all of them in parallel instead
          of one after the other.  The coverage sweep is what the library had before for fitting zooms -- at the fit's
          resolution it would need a grid of 4096 zooms.  The ratio fit / sweep says what the serial in-kernel bisection
          costs per evaluation -- with the lens's camera, where every frame takes all the steps (zooms 1.01 .. 1.23).  A
          pinhole of the lens's focal length sees less than the fisheye: nearly every frame is clear at 1.0 and is done after
          two evaluations (the recorded zooms say so), so its ratio is that of two evaluations against fourteen.
  render  frames per second of rssync_zoom_stabilize beside rssync_stabilize_frames at one zoom, on the same
          device-resident batches of 8 frames, both cameras, both filters.  The pinhole does the same arithmetic plus one
          load per frame; the lens's camera pays an fp64 ray per pixel per frame instead of a 16-byte load of the cached map.

    python tools/gpu_zoom_rate.py [--out profiles/zoom_rate.json] [--reps 5]

No ratio is a target.  Every time is a host clock around a call that ends in a device synchronise, after one warm-up call
of the same shape; two alternating rounds of each kind, the mean of each kind's two medians, and the rounds' spread, which
is the noise the ratios are read against.  The frames are noise, the gyro is synth.make_gyro's (up to 2 rad/s), the readout
11.11 ms, the lens synth.LENS scaled to the frame.
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
FIT_FRAMES = (256, 2048)
BATCH = 8
SIGMA = 0.2
LO, HI, STEPS = 1.0, 1.5, 12
SWEEP_ZOOMS = STEPS + 2


def lens_of(w, h):
    from rssync_amd import synth
    ro, fx, fy, cx, cy = synth.LENS[:5]
    return (ro, fx * w / synth.IMAGE_COLS, fy * h / synth.IMAGE_ROWS, cx * w / synth.IMAGE_COLS, cy * h / synth.IMAGE_ROWS) + \
        tuple(synth.LENS[5:])


def problem(n_times):
    import rssync_amd
    from rssync_amd import synth
    gyro = synth.make_gyro(1.0, 1.0 + (n_times + 2) / synth.FPS, seed=77)
    p = rssync_amd.SyncProblem(seed=1)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p, 1.0 + np.arange(n_times) / synth.FPS, synth.D_TRUE


def median_time(fn, reps):
    fn()                                                             # warm-up (buffers, code object, the ray maps)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                         # returns after the device synchronise
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def side_by_side(kinds, reps):
    """kinds: {name: callable} -> {name: (seconds, spread of the two rounds)}"""
    secs = {k: [] for k in kinds}
    for _ in range(2):
        for k, fn in kinds.items():
            secs[k].append(median_time(fn, reps))
    return {k: (float(np.mean(v)), abs(v[0] - v[1]) / float(np.mean(v))) for k, v in secs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zoom_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device")
    from rssync_amd import stabilize
    cameras = (("lens", stabilize.CAMERA_LENS), ("pinhole", stabilize.CAMERA_PINHOLE))
    p, all_times, delay = problem(max(FIT_FRAMES))
    res = {"sigma_s": SIGMA, "iterations": 3, "fit": {"zoom_lo": LO, "zoom_hi": HI, "steps": STEPS, "sweep_zooms": SWEEP_ZOOMS, "rows": []},
           "render": {"batch_frames": BATCH, "rows": []}}
    sweep = np.linspace(LO, HI, SWEEP_ZOOMS)
    for w, h in SIZES:
        lens = lens_of(w, h)
        for n in FIT_FRAMES:
            times = all_times[:n]
            row = {"width": w, "height": h, "frame_times": n}
            for cam_name, cam in cameras:
                kw = dict(sigma=SIGMA, camera=cam)
                zooms, status = p.fit_zoom(w, h, lens, times, delay, LO, HI, steps=STEPS, **kw)
                row[cam_name + "_not_clear"] = int(status.sum())
                row[cam_name + "_zoom_min_max"] = [float(zooms.min()), float(zooms.max())]
                got = side_by_side({"fit": lambda: p.fit_zoom(w, h, lens, times, delay, LO, HI, steps=STEPS, **kw),
                                    "sweep": lambda: p.stabilize_coverage(w, h, lens, times, delay, sweep, **kw)}, a.reps)
                for kind, (s, spread) in got.items():
                    row["%s_%s_s" % (cam_name, kind)] = s
                    row["%s_%s_fps" % (cam_name, kind)] = n / s
                    row["%s_%s_round_spread" % (cam_name, kind)] = spread
                row[cam_name + "_fit_over_sweep"] = row[cam_name + "_fit_fps"] / row[cam_name + "_sweep_fps"]
            res["fit"]["rows"].append(row)
            print(json.dumps(row), flush=True)
    rng = np.random.default_rng(0)
    times = all_times[:BATCH]
    zooms = 1.0 + 0.01 * np.arange(BATCH)            # one zoom per frame, 1.00 .. 1.07; the constant one is 1.04
    for w, h in SIZES:
        lens = lens_of(w, h)
        frames = torch.from_numpy(rng.integers(0, 256, size=(BATCH, h, w), dtype=np.uint8)).to("cuda:0")
        out = torch.empty_like(frames)
        row = {"width": w, "height": h}
        for cam_name, cam in cameras:
            for flt_name, flt in (("bilinear", stabilize.FILTER_BILINEAR), ("bicubic", stabilize.FILTER_BICUBIC)):
                kw = dict(out=out, sigma=SIGMA, camera=cam, filter=flt)
                # equal zooms give the stabiliser's bytes: the two calls timed below do the same work but for the ray
                want, _ = p.stabilize_frames(frames, times, lens, delay, zoom=1.04, **kw)
                want = want.clone()
                got, _ = p.stabilize_frames_zoomed(frames, times, lens, delay, [1.04] * BATCH, **kw)
                assert bool((got == want).all()), (w, h, cam_name, flt_name)
                del want
                t = side_by_side({"zoomed": lambda: p.stabilize_frames_zoomed(frames, times, lens, delay, zooms, **kw),
                                  "constant": lambda: p.stabilize_frames(frames, times, lens, delay, zoom=1.04, **kw)}, a.reps)
                key = "%s_%s" % (cam_name, flt_name)
                for kind, (s, spread) in t.items():
                    row["%s_%s_s" % (key, kind)] = s
                    row["%s_%s_fps" % (key, kind)] = BATCH / s
                    row["%s_%s_round_spread" % (key, kind)] = spread
                row[key + "_zoomed_over_constant"] = row[key + "_zoomed_fps"] / row[key + "_constant_fps"]
        res["render"]["rows"].append(row)
        print(json.dumps(row), flush=True)
        del frames, out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
