"""Gyro conditioning (rssync_ext_set_gyro_conditioning) on an MI355X -> one JSON object (profiles/gyro_conditioning.json),
the raw route beside the conditioned one:

  conditioning   steps 1-3 (uniform grid, zero-phase low-pass, decimation: rship_gyro_rates_condition, called on the
                 device context) for 10^6 and 10^7 samples of an 8 kHz stream: time, the filter's share of it, and the
                 bytes the kernels move per second against the 6.29 TB/s a copy kernel reaches on this GPU
  large          PreSync (800 candidates) and Sync at F x 2048 tracks with an 8 kHz gyro: raw, conditioned to 1 kHz
                 (divider 32, every 8th) and to 400 Hz (divider 80, every 20th)
  sync_points    98 sync points of 61 x 130, the same three routes, outer iterations capped per Sync call
  sweep          the 48-orientation sweep at 512 x 2048, raw against conditioned to 1 kHz
  quality        five seeds of an 8 kHz scene whose RATES carry vibration (0.3 rad/s narrow-band at 600-1500 Hz per axis
                 plus white noise, vibration() below): Sync's delay error against the truth, raw and conditioned

    OUT=profiles/gyro_conditioning.json python tools/gpu_gyro_conditioning.py [conditioning large sync_points sweep quality]

GPU box."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rssync_amd  # noqa: E402
from rssync_amd import synth  # noqa: E402

F_LARGE = int(os.environ.get("F", 4096))
REPS = int(os.environ.get("REPS", 3))
BOUND = int(os.environ.get("BOUND", 25))
COPY_TBPS = 6.29                                  # what a copy kernel reaches on this GPU
ROUTES = (("raw_8khz", None), ("conditioned_1khz", (32, 8)), ("conditioned_400hz", (80, 20)))


def note(*a):
    print(*a, file=sys.stderr, flush=True)


class GyroResult(C.Structure):                    # include/rssync_hip.h: rship_gyro_result
    _fields_ = [("fs", C.c_double), ("start", C.c_double), ("first_sample", C.c_uint64), ("bad_pos", C.c_uint64),
                ("bad_a", C.c_int64), ("bad_b", C.c_int64), ("n_knots", C.c_uint32), ("status", C.c_int32)]


def conditioning(n):
    rng = np.random.default_rng(n % 1000)
    t = np.sort(np.arange(n) / 8000.0 + rng.uniform(-0.1, 0.1, n) / 8000.0) + 1.0
    tt = np.arange(n) / 8000.0
    r = np.stack([np.sin(2 * np.pi * (0.7 + 0.4 * ax) * tt) for ax in range(3)], axis=1) + rng.normal(0, 0.01, (n, 3))
    p = rssync_amd.SyncProblem(verbose=False)
    lib = rssync_amd.load_library()
    fn = lib.rship_gyro_rates_condition
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(GyroResult)]
    ctx = C.c_void_p(p.device_context())
    p.set_gyro_rates(t, r)                        # (allocations)
    t0 = time.perf_counter()
    p.set_gyro_rates(t, r)                        # the raw route: upload + per-sample integration, resampling, spline
    raw_setter = time.perf_counter() - t0
    p.profile(True)
    out = {"samples": n}
    for name, (div, k) in (("grid_decimate_only", (0, 8)), ("with_filter", (32, 8))):
        res, walls, kern = GyroResult(), [], []
        for _ in range(REPS + 1):
            p.profile_reset()
            t0 = time.perf_counter()
            rc = fn(ctx, div, k, C.byref(res))
            walls.append(time.perf_counter() - t0)
            kern.append(p.profile_get()["gyro"][1])
            assert rc == 0 and res.status == 0, (rc, res.status)
        out[name] = {"wall_ms": round(1e3 * min(walls[1:]), 3), "kernel_ms": round(min(kern[1:]), 3), "grid_samples_left": res.n_knots}
    full, part = out["with_filter"]["kernel_ms"], out["grid_decimate_only"]["kernel_ms"]
    out["filter_share_of_kernel_time"] = round((full - part) / full, 3)
    # bytes: the order check reads ts + rates (32 n), the grid kernel the same and writes 24 m, every pass of the filter reads its
    # input three times (the segment pass, the chunk from zero, the chunk from its state) and writes once (96 m, two passes), the
    # decimation reads and writes 24 m / k
    m = n
    moved = 64 * n + 24 * m + 192 * m + 48 * (m // 8)
    out["bytes_moved_model"] = moved
    out["effective_TBps"] = round(moved / (full * 1e-3) / 1e12, 3)
    out["share_of_copy_rate"] = round(out["effective_TBps"] / COPY_TBPS, 3)
    out["verdict"] = ("far from the copy rate: the filter is a serial recurrence per thread (chunks of 32 samples, three runs over the data "
                      "per pass, strided 24-byte records); it runs once per upload" if out["share_of_copy_rate"] < 0.5 else "near the copy rate")
    p.profile(False)
    p.set_gyro_conditioning(32, 8)
    p.set_gyro_rates(t, r)
    t0 = time.perf_counter()
    p.set_gyro_rates(t, r)
    out["set_gyro_rates_wall_ms"] = {"raw": round(1e3 * raw_setter, 2), "conditioned_1khz": round(1e3 * (time.perf_counter() - t0), 2)}
    p.close()
    note("conditioning", n, out)
    return out


def scene(F, N, seed, fs=8000.0, **kw):
    g = synth.make_gyro(1.0, 1.0 + (F + 2) / synth.FPS, fs=fs, seed=seed)   # t0 = 0: the raw route takes no negative times
    return g, list(synth.make_frames(g, 30, 30 + F, N, seed=seed, **kw))


def problem(g, frames, cond, rates=None, **kw):
    p = rssync_amd.SyncProblem(verbose=False, **kw)
    if cond:
        p.set_gyro_conditioning(*cond)
    for fr in frames:
        p.SetTrackResult(*fr)
    p.set_gyro_rates(g.times, g.rates if rates is None else rates)
    return p


def per_launch(prof):
    return {k: round(v[1] / v[0], 4) for k, v in prof.items() if v[0]}


def large(F):
    g, frames = scene(F, 2048, seed=3)
    note("large: scene ready")
    out = {"frames": F, "tracks": 2048, "candidates": 800}
    for name, cond in ROUTES:
        p = problem(g, frames, cond, seed=3, max_outer_iters=10)
        p.upload()
        c, d = p.PreSync(0.0, 30, 30 + F, 0.0005, 0.2)
        p.Sync(d, 30, 30 + F - 1, 0.0, 0.2)
        p.profile(True)
        best = None
        for _ in range(REPS):
            p.profile_reset()
            t0 = time.perf_counter()
            c, d = p.PreSync(0.0, 30, 30 + F, 0.0005, 0.2)
            t_pre = time.perf_counter() - t0
            t0 = time.perf_counter()
            c2, d2 = p.Sync(d, 30, 30 + F - 1, 0.0, 0.2)
            t_sync = time.perf_counter() - t0
            cur = per_launch(p.profile_get())
            cur["_presync_ms"], cur["_sync_ms"] = 1e3 * t_pre, 1e3 * t_sync
            best = cur if best is None else {k: min(best[k], cur[k]) for k in cur}
        out[name] = {"presync_ms": round(best.pop("_presync_ms"), 3), "sync_ms": round(best.pop("_sync_ms"), 3), "presync_delay": d,
                     "sync_delay": d2, "outer_iterations": len(p.sync_trace()), "kernel_ms_per_launch": best, "gyro_hz": p.gyro_info()[0],
                     "windows": p.window_info()}
        p.close()
        note("large", name, out[name])
    k2 = {name: out[name]["kernel_ms_per_launch"]["lmeds"] for name, _ in ROUTES}
    out["presync_kernel_ms"] = k2
    # "the 400 Hz numbers come back": the conditioned stream's sweep within 2 % of the same frames at 400 Hz
    out["the_400_hz_numbers_come_back"] = bool(k2["conditioned_1khz"] <= 1.02 * k2["conditioned_400hz"])
    return out


def sync_points():
    Fs, Ns, W, D = 3000, 130, 60, 30
    g, frames = scene(Fs, Ns, seed=6)
    pos = [30 + x for x in range(0, Fs - W - 1, D)]
    out = {"positions": len(pos), "window_frames": W + 1, "tracks": Ns, "outer_iterations_cap_per_call": BOUND}
    for name, cond in ROUTES:
        p = problem(g, frames, cond, seed=6, max_outer_iters=BOUND)
        p.upload()
        p.sync_points(pos, W, 0.0, 0.001, 0.1)
        best = None
        for _ in range(REPS):
            t0 = time.perf_counter()
            c, d = p.sync_points(pos, W, 0.0, 0.001, 0.1)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[name] = {"sync_points_s": round(best, 4), "median_abs_err_ms": float(np.median(np.abs(d - synth.D_TRUE)) * 1e3),
                     "gyro_hz": p.gyro_info()[0], "windows": p.window_info()}
        p.close()
        note("sync_points", name, out[name])
    return out


def sweep():
    F = 512
    g, frames = scene(F, 2048, seed=4)
    names = list(synth.ORIENTATIONS)
    out = {"frames": F, "tracks": 2048, "orientations": len(names), "candidates": 800}
    for name, cond in ROUTES[:2]:
        p = problem(g, frames, cond, seed=4)
        p.upload()
        p.orientation_sweep(g.times, g.rates, names[:2], 0.0, 30, 30 + F, 0.0005, 0.2)
        p.profile(True)
        walls = []
        for _ in range(REPS):
            p.profile_reset()
            t0 = time.perf_counter()
            costs, delays = p.orientation_sweep(g.times, g.rates, names, 0.0, 30, 30 + F, 0.0005, 0.2)
            walls.append(time.perf_counter() - t0)
        k = p.profile_get()
        best = int(np.argmin(costs))
        out[name] = {"wall_ms": round(1e3 * min(walls), 2), "wall_ms_per_orientation": round(1e3 * min(walls) / len(names), 3),
                     "kernel_ms_last_run": {nm: round(v[1], 3) for nm, v in k.items() if v[0]}, "best": names[best], "best_delay": float(delays[best])}
        p.close()
        note("sweep", name, out[name])
    return out


def vibration(g, seed):
    """the rates a flight controller on a vibrating frame logs: per axis a narrow-band 0.3 rad/s component somewhere in
    600-1500 Hz (slowly wandering phase) plus white noise of 0.05 rad/s"""
    rng = np.random.default_rng([seed, 99])
    t = g.times
    out = g.rates.copy()
    for ax in range(3):
        f = rng.uniform(600.0, 1500.0)
        wander = np.cumsum(rng.normal(0, 0.02, t.size))
        out[:, ax] += 0.3 * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi) + wander)
    return out + rng.normal(0, 0.05, out.shape)


def quality():
    F, N = 64, 256
    rows = []
    for seed in range(5):
        g, frames = scene(F, N, seed=20 + seed)
        rates = vibration(g, seed)
        row = {"seed": 20 + seed}
        for name, cond in ROUTES[:2]:
            p = problem(g, frames, cond, rates=rates, seed=20 + seed)
            _, d0 = p.PreSync(0.0, 30, 30 + F, 0.001, 0.1)
            _, d = p.Sync(d0, 30, 30 + F, 0.0, 0.1)
            row[name] = {"presync_delay": d0, "sync_delay": d, "error_s": d - synth.D_TRUE}
            p.close()
        rows.append(row)
        note("quality", row)
    med = {name: float(np.median([abs(r[name]["error_s"]) for r in rows])) for name, _ in ROUTES[:2]}
    return {"frames": F, "tracks": N, "true_delay": synth.D_TRUE, "seeds": rows, "median_abs_error_s": med,
            "conditioning_makes_the_median_worse": bool(med["conditioned_1khz"] > med["raw_8khz"])}


def main():
    which = sys.argv[1:] or ["conditioning", "large", "sync_points", "sweep", "quality"]
    result = {"what": __doc__.strip().splitlines()[0]}
    path = os.environ.get("OUT")
    if path and os.path.exists(path):             # parts measured by an earlier call stay
        with open(path) as f:
            result.update(json.load(f))
    if "conditioning" in which:
        result["conditioning"] = {"copy_rate_TBps": COPY_TBPS, "1e6": conditioning(10 ** 6), "1e7": conditioning(10 ** 7)}
    if "quality" in which:
        result["quality"] = quality()
    if "sweep" in which:
        result["sweep_48_orientations"] = sweep()
    if "sync_points" in which:
        result["sync_points"] = sync_points()
    if "large" in which:
        result["large"] = large(F_LARGE)
    if path:
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
