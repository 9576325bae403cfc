"""The lens sweep (rssync_ext_lens_sweep) on an MI355X -> one JSON object (profiles/lens_sweep.json): a 9-lens sweep
on the pipelined route, on the one-by-one route (RSSYNC_SWEEP_PIPELINE=0: re-lens, wait for the count, PreSync, per
candidate) and as the loop through the calls that existed before it (set_track_pixels for every frame, then PreSync, per
candidate); the re-lens kernel against the packing kernel; and a whole estimate_lens (3 passes over "f" and "k1", 9
candidates each, plus the final lens: 55 sweeps' worth in 7 calls).
  (a) the recovery scene of tests/test_gpu_lens_sweep.py: 120 frames x 256 tracks, PreSync step 0.5 ms, radius 0.1 s
  (b) BASELINE config 5's size: 4096 frames x 2048 tracks, step 0.5 ms, radius 0.2 s
Pixel frames from synth.make_pixel_frames, installed with the focal lengths 15 % low and no distortion terms; at size (b)
64 generated frames are repeated over the frame range (timing only).  GPU box."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rssync_amd  # noqa: E402
from rssync_amd import synth  # noqa: E402
from rssync_amd.lens import estimate_lens, shifted  # noqa: E402

KERNELS = ("lmeds", "reduce", "relens", "pixels")


def start_lens():
    ro, fx, fy, cx, cy = synth.LENS[:5]
    return np.array((ro, 0.85 * fx, 0.85 * fy, cx, cy, 0.0, 0.0, 0.0, 0.0))


def scene(F, N, distinct, seed=1):
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=seed)
    base = list(synth.make_pixel_frames(gyro, 0, min(F, distinct), N, seed=seed))
    frames = [(fr, fr / synth.FPS, (fr + 1) / synth.FPS) + tuple(base[fr % len(base)][3:]) for fr in range(F)]
    return gyro, frames


def set_frames(p, frames, lens):
    for fr, ta, tb, pa, pb in frames:
        p.set_track_pixels(fr, ta, tb, pa, pb, lens, synth.IMAGE_ROWS)


def kernels(p):
    k = p.profile_get()
    return {nm: {"launches": k[nm][0], "ms": round(k[nm][1], 4)} for nm in KERNELS}


def measure(name, F, N, distinct, step, radius, reps):
    gyro, frames = scene(F, N, distinct)
    start = start_lens()
    lenses = np.stack([shifted(start, "f", g) for g in np.linspace(-0.25, 0.25, 9)])
    p = rssync_amd.SyncProblem(seed=321)            # (the tests' seed: the recovery scene's numbers are theirs)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    set_frames(p, frames, start)
    p.profile(True)
    p.profile_reset()
    p.upload()                                      # the packing kernel (every frame, from the raw records)
    pack = kernels(p)["pixels"]
    args = (0.0, 0, F, step, radius)
    p.lens_sweep(lenses[:2], *args)                 # warm-up
    out = {"frames": F, "tracks": N, "lenses": len(lenses), "candidate_delays": int(round(2 * radius / step)),
           "pack_kernel_ms": pack["ms"]}
    res = {}
    for route, env in (("pipelined", None), ("one_by_one", "0")):
        walls = []
        for _ in range(reps):
            if env:
                os.environ["RSSYNC_SWEEP_PIPELINE"] = env
            p.profile_reset()
            t = time.perf_counter()
            c, d = p.lens_sweep(lenses, *args)
            walls.append(time.perf_counter() - t)
            os.environ.pop("RSSYNC_SWEEP_PIPELINE", None)
        k = kernels(p)
        res[route] = (c, d)
        out[route] = {"wall_ms": round(1e3 * min(walls), 3), "kernel_ms": round(sum(k[nm]["ms"] for nm in ("lmeds", "reduce", "relens")), 3),
                      "walls_s": [round(w, 4) for w in walls], "kernels_last_run": k}
    walls = []
    for _ in range(reps):                           # the loop through the calls that existed before the sweep
        p.profile_reset()
        t = time.perf_counter()
        r = []
        for lens in lenses:
            set_frames(p, frames, lens)
            r.append(p.PreSync(*args))
        walls.append(time.perf_counter() - t)
    k = kernels(p)
    res["loop"] = (np.array([x[0] for x in r]), np.array([x[1] for x in r]))
    out["loop"] = {"wall_ms": round(1e3 * min(walls), 3), "kernel_ms": round(sum(k[nm]["ms"] for nm in ("lmeds", "reduce", "pixels")), 3),
                   "walls_s": [round(w, 4) for w in walls], "kernels_last_run": k}
    set_frames(p, frames, start)
    out["routes_identical"] = bool(all(np.array_equal(res["pipelined"][i], res[o][i]) for o in ("one_by_one", "loop") for i in (0, 1)))
    out["loop_over_pipelined"] = round(out["loop"]["wall_ms"] / out["pipelined"]["wall_ms"], 2)
    out["one_by_one_over_pipelined"] = round(out["one_by_one"]["wall_ms"] / out["pipelined"]["wall_ms"], 2)
    k = out["pipelined"]["kernels_last_run"]["relens"]
    out["relens_kernel_ms_per_launch"] = round(k["ms"] / max(1, k["launches"]), 5)
    out["pack_kernel_ms_per_launch"] = round(pack["ms"] / max(1, pack["launches"]), 5)
    out["relens_bytes_per_launch"] = F * N * 128       # 32 B read (the pixel record) + 96 B written (all packed streams)
    out["relens_effective_GBps"] = round(out["relens_bytes_per_launch"] / (out["relens_kernel_ms_per_launch"] * 1e-3) / 1e9, 1) \
        if out["relens_kernel_ms_per_launch"] > 0 else None
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        est = estimate_lens(p, start, *args)
        walls.append(time.perf_counter() - t)
    out["estimate_lens"] = {"wall_ms": round(1e3 * min(walls), 3), "walls_s": [round(w, 4) for w in walls]}
    if distinct >= F:    # (repeated frames do not belong to the gyro track: there only the time means something)
        out["estimate_lens"].update({"fx": est.lens[1], "k1": est.lens[5], "fx_error_percent": round(100 * (est.lens[1] / synth.LENS[1] - 1), 4),
                                     "cost": est.cost, "presync_delay_s": est.delay, "unresolved": list(est.unresolved)})
    else:
        out["estimate_lens"]["note"] = "timing only: the repeated frames do not belong to the gyro track, the search finds no minimum"
    print(name, json.dumps(out), flush=True)
    return out


def main():
    which = sys.argv[1:] or ["recovery", "c5"]
    result = {"what": __doc__.strip().splitlines()[0]}
    if "recovery" in which:
        result["recovery_120x256"] = measure("recovery", 120, 256, 120, 0.0005, 0.1, reps=5)
    if "c5" in which:
        result["c5_4096x2048"] = measure("c5", 4096, 2048, 64, 0.0005, 0.2, reps=2)
    path = os.environ.get("OUT")
    if path:
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
