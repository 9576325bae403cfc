"""The readout sweep (rssync_ext_readout_sweep) on an MI355X -> one JSON object (profiles/readout_sweep.json):
wall time against kernel time per candidate readout, the pipelined route against the one-by-one route
(RSSYNC_SWEEP_PIPELINE=0: set the readout, PreSync, per candidate), and the re-timing kernel against the packing kernel.
  (a) the reference driver's window: 61 frames x 130 tracks, PreSync step 1 ms, radius 0.1 s, 41 readouts 0 .. 20 ms
  (b) BASELINE config 5's size: 4096 frames x 2048 tracks, step 0.5 ms, radius 0.2 s, 48 readouts 0 .. 23.5 ms
Pixel frames from synth.make_pixel_frames; at size (b) 64 generated frames are repeated over the frame range (timing only).
GPU box."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rssync_amd  # noqa: E402
from rssync_amd import synth  # noqa: E402

KERNELS = ("lmeds", "reduce", "retime", "pixels")


def problem(F, N, distinct, seed=5):
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=seed)
    base = list(synth.make_pixel_frames(gyro, 0, min(F, distinct), N, seed=seed))
    p = rssync_amd.SyncProblem(seed=seed)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    lens = (0.0,) + tuple(synth.LENS[1:])
    for fr in range(F):
        _, _, _, pa, pb = base[fr % len(base)]
        p.set_track_pixels(fr, fr / synth.FPS, (fr + 1) / synth.FPS, pa, pb, lens, synth.IMAGE_ROWS)
    return p


def kernels(p):
    k = p.profile_get()
    return {nm: {"launches": k[nm][0], "ms": round(k[nm][1], 4)} for nm in KERNELS}


def measure(name, F, N, distinct, readouts, step, radius, reps):
    p = problem(F, N, distinct)
    p.profile(True)
    p.profile_reset()
    t = time.perf_counter()
    p.upload()                                      # the packing kernel (every frame, from the raw records)
    t_pack = time.perf_counter() - t
    pack = kernels(p)["pixels"]
    args = (0.0, 0, F, step, radius)
    p.readout_sweep(readouts[:2], *args)            # warm-up
    out = {"frames": F, "tracks": N, "readouts": len(readouts), "candidate_delays": int(round(2 * radius / step)),
           "pack_wall_ms": round(1e3 * t_pack, 3), "pack_kernel_ms": pack["ms"]}
    res = {}
    for route, env in (("pipelined", None), ("one_by_one", "0")):
        walls = []
        for _ in range(reps):
            if env:
                os.environ["RSSYNC_SWEEP_PIPELINE"] = env
            p.profile_reset()
            t = time.perf_counter()
            c, d = p.readout_sweep(readouts, *args)
            walls.append(time.perf_counter() - t)
            os.environ.pop("RSSYNC_SWEEP_PIPELINE", None)
        k = kernels(p)
        kern = sum(k[nm]["ms"] for nm in ("lmeds", "reduce", "retime"))
        res[route] = (c, d)
        out[route] = {"wall_ms_per_readout": round(1e3 * min(walls) / len(readouts), 4),
                      "kernel_ms_per_readout": round(kern / len(readouts), 4),
                      "walls_s": [round(w, 4) for w in walls], "kernels_last_run": k}
    out["routes_identical"] = bool(np.array_equal(res["pipelined"][0], res["one_by_one"][0]) and
                                   np.array_equal(res["pipelined"][1], res["one_by_one"][1]))
    k = out["pipelined"]["kernels_last_run"]["retime"]
    out["retime_kernel_ms_per_launch"] = round(k["ms"] / max(1, k["launches"]), 5)
    pairs = F * N
    out["retime_bytes_per_launch"] = pairs * 40        # 16 B read (y_a, y_b) + 24 B written (fp32 ta/tb + fp64 ta/tb)
    out["retime_effective_GBps"] = round(out["retime_bytes_per_launch"] / (out["retime_kernel_ms_per_launch"] * 1e-3) / 1e9, 1) \
        if out["retime_kernel_ms_per_launch"] > 0 else None
    out["pack_over_retime"] = round(pack["ms"] / max(1e-9, out["retime_kernel_ms_per_launch"]), 1)
    best = min(range(len(readouts)), key=lambda i: (res["pipelined"][0][i], res["pipelined"][1][i]))
    out["arg_min_readout_s"] = float(readouts[best])
    print(name, json.dumps(out), flush=True)
    return out


def main():
    which = sys.argv[1:] or ["driver", "c5"]
    result = {"what": __doc__.strip().splitlines()[0]}
    if "driver" in which:
        result["driver_61x130"] = measure("driver", 61, 130, 61, np.arange(41) * 0.0005, 0.001, 0.1, reps=5)
    if "c5" in which:
        result["c5_4096x2048"] = measure("c5", 4096, 2048, 64, np.arange(48) * 0.0005, 0.0005, 0.2, reps=2)
    path = os.environ.get("OUT")
    if path:
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
