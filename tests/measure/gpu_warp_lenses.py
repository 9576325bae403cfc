"""The rectifier's and the stabiliser's maps on the device against the float64 reference, per lens and motion at 95 x 169
(tests/test_gpu_warp_lenses.py's section a, measured): the device's distance, the case's tolerance, the shares of pixels
in range, compared and out of range, and the distance of a camera at rest from the identity.  GPU box:

    python tests/measure/gpu_warp_lenses.py [out.json] [--before LIB]      (default profiles/warp_lenses.json)

--before names another build of the library (RSSYNC_LIB): the same distances are measured with it in a child process and
written beside the present ones as `before` -- for `wide`, the map with the driver's nine-step ray, before the polish of
rect_pixel_ray."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: torch ships its own HIP runtime)
import rssync_amd  # noqa: E402
import stabilize_reference as sr  # noqa: E402
import warp_cases as wc  # noqa: E402


def problem(motion):
    g = wc.gyro(motion)
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(g.quats, g.fs, g.t0)
    return p


def distance(got, c):
    """largest |device - float64| over the compared pixels (NaN where the device gives no position for one of them)"""
    d = np.abs(got.astype(np.float64) - c["m64"])[c["compared"]]
    return float(d.max()) if np.isfinite(d).all() else float("nan")


def measure():
    problems = {m: problem(m) for m in wc.MOTIONS}
    res = {"rectifier": {}, "stabiliser": {}, "rest_identity": {}, "points_full_size": {}}
    for name, motion, extra, ref_row in wc.rect_cases():
        c = wc.rect_case(name, motion, extra, ref_row)
        got = problems[motion].rectify_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"], ref_row=ref_row)
        n = c["in_range"].size
        res["rectifier"]["%s %s +%.2f ref_row %s" % (name, motion, extra, ref_row)] = dict(
            device_px=distance(got, c), tolerance_px=c["tol"], in_range_share=c["in_range"].sum() / n,
            out_of_range_share=c["out_of_range"].sum() / n, compared_of_in_range=c["compared"].sum() / c["in_range"].sum(),
            out_of_range_nan_share=float(np.isnan(got[c["out_of_range"]]).all(-1).mean()) if c["out_of_range"].any() else None)
        if motion == "rest":
            d = np.abs(got.astype(np.float64) - wc.grid(wc.ROWS, wc.COLS))[c["in_range"]]
            res["rest_identity"][name] = dict(device_px=float(d.max()), tolerance_px=c["tol"])
    for name, motion in wc.stab_cases():
        c = wc.stab_case(name, motion)
        got = problems[motion].stabilize_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"], sigma=wc.STAB_SIGMA, zoom=wc.STAB_ZOOM,
                                             camera=sr.LENS)
        res["stabiliser"]["%s %s" % (name, motion)] = dict(device_px=distance(got, c), tolerance_px=c["tol"],
                                                          compared_of_in_range=c["compared"].sum() / c["in_range"].sum())
    import rectify_reference as rr
    for name in wc.LENSES:
        L, pts = wc.full_size_points(name)
        got = problems["x1"].rectify_points(pts, wc.FULL_COLS, wc.FULL_ROWS, L, wc.frame_time(), wc.delays()[0])
        want = rr.forward_points(wc.gyro("x1"), L, wc.FULL_ROWS, wc.frame_time(), wc.delays()[0], pts)
        res["points_full_size"][name] = dict(device_px=float(np.abs(got - want).max()), bound_px=1e-9, points=len(pts))
    return res


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print("RESULT " + json.dumps(measure()))
        return
    before = None
    if "--before" in args:
        i = args.index("--before")
        before = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "warp_lenses.json")
    res = {"what": "rectify_map and stabilize_map (lens camera, sigma %.1f, zoom %.1f) at %d x %d against the float64 reference; "
                   "cases and masks of tests/warp_cases.py; tolerance = 4 x max |map32 - map64| of the case" %
                   (wc.STAB_SIGMA, wc.STAB_ZOOM, wc.ROWS, wc.COLS)}
    res.update(measure())
    if before:
        env = dict(os.environ, RSSYNC_LIB=before)
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, check=True, timeout=300,
                             stdout=subprocess.PIPE, universal_newlines=True).stdout
        old = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res["before"] = {"what": "the same with the library before the polish of rect_pixel_ray (the driver's nine-step ray)",
                         "wide": {sec: {k: v["device_px"] for k, v in old[sec].items() if k.split()[0] == "wide"}
                                  for sec in ("rectifier", "stabiliser")},
                         "rest_identity": {k: v["device_px"] for k, v in old["rest_identity"].items()},
                         "points_full_size": {k: v["device_px"] for k, v in old["points_full_size"].items()}}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
