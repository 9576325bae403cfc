"""The feature pipeline on the CPU, for the constant tests/test_gpu_features.py compares the device with: the flat-region
clip of that test, the numpy detector and tracker (tests/feature_reference.py), then the oracle's PreSync + Sync fed the
reference driver's way (pixels_to_tracks + SetTrackResult, gyro integrated as core_testcode.cpp:36-52).

    python tools/feature_cpu_delay.py [--frames 41]

Prints one JSON line: the delay, its error against D_TRUE, the kept tracks and their error against the renderer's truth.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F0, SEED, ROWS, COLS = 30, 77, 760, 1352
FLAT = ((-7.0, 2.0, -7.0), (7.0, 7.0, 7.0))   # the +y part of the box: a third of the view, constant gray


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    a = ap.parse_args()
    import feature_reference as fr
    from oracle import oracle
    from rssync_amd import synth, synth_video as sv
    n = a.frames
    gyro = synth.make_gyro(1.0, 1.0 + (n + 2) / synth.FPS, seed=SEED)
    lens = sv.half_lens()
    frames, times, _ = sv.render(gyro, F0, F0 + n, lens=lens, rows=ROWS, cols=COLS, seed=SEED, flat=FLAT)
    tracks = fr.track(frames)
    p = oracle.OracleProblem(seed=321, threads=os.cpu_count() or 1, faithful=False)
    q, us = oracle.integrate_gyro(gyro.times, gyro.rates)
    p.SetGyroQuaternionsTimestamped(us, q)
    kept, errs = [], []
    for k, (pa, pb, st, _) in enumerate(tracks):
        ok = st == 0
        kept.append(int(ok.sum()))
        truth = sv.true_points(gyro, F0 + k, F0 + k + 2, pa[ok], lens=lens, rows=ROWS, seed=SEED)[0]
        errs.append(np.linalg.norm(pb[ok] - truth, axis=-1))
        p.SetTrackResult(F0 + k, *oracle.pixels_to_tracks(lens, times[k], times[k + 1], ROWS, pa[ok], pb[ok]))
    _, d = p.PreSync(0.0, F0, F0 + n - 1, 0.002, 0.1)
    _, d = p.Sync(d, F0, F0 + n - 2, 0.0, 0.2)
    e = np.concatenate(errs)
    print(json.dumps({"frames": n, "delay": d, "delay_error": abs(d - synth.D_TRUE), "kept_per_pair": [min(kept), max(kept)],
                      "track_error_median_px": float(np.median(e)), "track_error_p99_px": float(np.percentile(e, 99))}))


if __name__ == "__main__":
    main()
