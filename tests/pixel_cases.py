"""Inputs and comparisons of tests/test_pixel_front_door.py and tests/measure/gpu_pixel_front_door.py: lenses, point
sets, the two feeding routes (pixels into the library; the oracle's undistortion, then SetTrackResult) and the per-frame
comparison of the packed fp32 and fp64 streams.  numpy + the oracle only; every function takes the problems it compares."""
from fractions import Fraction

import numpy as np

SEED = 321
LENSES = ("synth", "pinhole", "aniso", "wide", "strong", "negmild", "half")
COLS, ROWS = 2704, 1520
DELAYS = (0.0371, -0.0123)      # two delays per frame for the fp64 rows
RAY_TOL32 = 1.2e-7              # one fp32 ulp of 1: the project's bound on a ray component (test_upstream_steps.py)
P_TOL64 = 1e-13                 # the bound of tests/test_gpu_mid_sizes.py on fp64 rows of P for ray-fed frames


def lenses():
    """name -> (lens, cols, rows).  'aniso' has nine pairwise distinct fields: a swapped pair cannot cancel."""
    from rssync_amd import synth, synth_video
    ro, k = synth.READOUT, tuple(synth.LENS[5:])
    return {
        "synth": (tuple(synth.LENS), COLS, ROWS),
        "pinhole": (tuple(synth.LENS[:5]) + (0.0, 0.0, 0.0, 0.0), COLS, ROWS),
        "aniso": ((ro, 1180.0, 900.0, 1300.5, 790.25) + k, COLS, ROWS),
        "wide": ((ro, 850.0, 850.0, 1352.0, 760.0, 0.03, 0.06, -0.06, 0.02), COLS, ROWS),
        "strong": ((ro, 850.0, 850.0, 1352.0, 760.0, 0.4, 0.1, 0.05, 0.01), COLS, ROWS),
        "negmild": ((ro, 1180.0, 1180.0, 1352.0, 760.0, -0.1, 0.01, 0.0, 0.0), COLS, ROWS),
        "half": (tuple(synth_video.half_lens()), COLS // 2, ROWS // 2),
    }


def nonmonotonic_lens():
    """k1 = -0.3 alone: the model turns over at theta = 1.05, so most of the image has no inverse"""
    from rssync_amd import synth
    return (synth.READOUT, 850.0, 850.0, 1352.0, 760.0, -0.3, 0.0, 0.0, 0.0)


def with_readout(lens, ro):
    return (float(ro),) + tuple(lens[1:])


def scaled_lens(lens, s):
    """the same lens for an image s times the size"""
    return (lens[0],) + tuple(s * v for v in lens[1:5]) + tuple(lens[5:])


def model(lens, th):
    k1, k2, k3, k4 = lens[5:]
    q = th * th
    return th * (1 + q * (k1 + q * (k2 + q * (k3 + q * k4))))


def in_image(p, cols, rows):
    return (p[:, 0] >= 0) & (p[:, 0] <= cols) & (p[:, 1] >= 0) & (p[:, 1] <= rows)


def _uniform(rng, n, cols, rows, margin=0.0):
    return rng.uniform([-margin * cols, -margin * rows], [(1 + margin) * cols, (1 + margin) * rows], size=(n, 2))


def _straddle(rng, n, lens, cols, rows):
    """points on both sides of the model's range rd = model(pi / 2), alternating from lane to lane: inside by a part in
    1e9 to 5 %, outside by as much, at random angles; every fourth lane is an ordinary in-image point (no trip of the
    halving loop beside neighbours that make several)"""
    _, fx, fy, cx, cy = lens[:5]
    edge = model(lens, np.pi / 2)
    s = 10.0 ** rng.uniform(-9, np.log10(0.05), size=n) * np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    rd, phi = edge * (1 + s), rng.uniform(0, 2 * np.pi, size=n)
    p = np.stack([cx + fx * rd * np.cos(phi), cy + fy * rd * np.sin(phi)], axis=-1)
    p[3::4] = _uniform(rng, len(p[3::4]), cols, rows)
    return p


def point_sets(lens, cols, rows, seed, n=1024):
    """-> list of (name, points_a, points_b); the A and B ends of every set are drawn independently"""
    rng = np.random.default_rng([seed, 41])
    cx, cy = lens[3], lens[4]
    out = [("inside", _uniform(rng, n, cols, rows), _uniform(rng, n, cols, rows))]
    border = np.array([[0, 0], [cols, 0], [0, rows], [cols, rows], [cols / 2, 0], [cols / 2, rows], [0, rows / 2],
                       [cols, rows / 2]], dtype=np.float64)
    # the reference's quirk (core_testcode.cpp:64 tests the pixel, not the centred point): (0, 0) at A only, B only, both;
    # the exact principal point and its neighbours on both sides of the rd < 1e-9 branch
    off = [0.0, 1e-10, 1e-7, 1e-6, 2e-6, 1e-5]
    pp = np.array([[cx + d * ux, cy + d * uy] for d in off for ux, uy in ((1, 0), (0, 1), (1, -1))])
    z = np.zeros((3, 2))
    r = _uniform(rng, 3, cols, rows)
    a = np.concatenate([border, rng.permutation(border), z, r, z, pp, _uniform(rng, len(pp), cols, rows), pp])
    b = np.concatenate([rng.permutation(border), border, r[::-1], z, z, _uniform(rng, len(pp), cols, rows), pp,
                        rng.permutation(pp)])
    out.append(("special", a, b))
    out.append(("margin", _uniform(rng, n, cols, rows, 0.5), _uniform(rng, n, cols, rows, 0.5)))
    out.append(("straddle", _straddle(rng, n // 2, lens, cols, rows), _straddle(rng, n // 2, lens, cols, rows)))
    return out


def halving_trips(lens, p):
    """numpy restatement of lens_math.hpp's schedule, counting per point the largest number of trips the halving loop makes
    in one of the nine Newton steps (0 = the loop never ran)"""
    _, fx, fy, cx, cy, k1, k2, k3, k4 = lens
    xn, yn = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    rd = np.sqrt(xn * xn + yn * yn)
    th = np.full(len(p), np.pi / 4)
    worst = np.zeros(len(p), dtype=np.int64)
    for _ in range(9):
        q = th * th
        mdl = th * (1. + q * (k1 + q * (k2 + q * (k3 + q * k4))))
        slope = 1. + q * (3. * k1 + q * (5. * k2 + q * (7. * k3 + q * (8. * k4))))
        nxt = th - (mdl - rd) / slope
        trips = np.zeros(len(p), dtype=np.int64)
        for _ in range(1200):
            out = (nxt <= 0.) | (nxt >= np.pi / 2.)
            if not out.any():
                break
            nxt = np.where(out, 0.5 * (nxt + th), nxt)
            trips += out
        worst = np.maximum(worst, trips)
        th = nxt
    return worst


# ---- feeding -------------------------------------------------------------------------------------------------------
# a frame of a problem: dict(id, ta, tb, pa, pb, lens, rows, cols, rays=False); rays=True: set with SetTrackResult from
# the oracle's undistortion on BOTH routes (a frame the driver undistorted itself)

def frame(fid, ta, tb, pa, pb, lens, rows, cols, rays=False):
    return dict(id=int(fid), ta=float(ta), tb=float(tb), pa=np.ascontiguousarray(pa, np.float64),
                pb=np.ascontiguousarray(pb, np.float64), lens=tuple(lens), rows=rows, cols=cols, rays=rays)


def oracle_tracks(f):
    from oracle import oracle
    return oracle.pixels_to_tracks(f["lens"], f["ta"], f["tb"], f["rows"], f["pa"], f["pb"])


def set_frame(p, f, route):
    """route 'pixels': the library's front door (ray frames excepted); 'oracle': the reference driver's way"""
    if route == "pixels" and not f["rays"]:
        p.set_track_pixels(f["id"], f["ta"], f["tb"], f["pa"], f["pb"], f["lens"], f["rows"])
    else:
        p.SetTrackResult(f["id"], *oracle_tracks(f))


def feed(p, gyro, frames, route):
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for f in frames:
        set_frame(p, f, route)
    return p


def oracle_problem(gyro, frames, seed):
    import os
    from oracle.oracle import OracleProblem
    return feed(OracleProblem(seed=seed, threads=min(os.cpu_count() or 1, 16), faithful=False), gyro, frames, "oracle")


def both_in_image(f):
    return in_image(f["pa"], f["cols"], f["rows"]) & in_image(f["pb"], f["cols"], f["rows"])


# ---- comparing -----------------------------------------------------------------------------------------------------
class Tally:
    """what one check measured: fp32 components compared / differing over in-image tracks, the largest differences"""

    def __init__(self):
        self.total = self.diff = 0
        self.max32 = self.max32_in = self.max64_oracle = self.max64_rays = self.max64_oracle_all = 0.0

    def share(self):
        return self.diff / self.total if self.total else 0.0

    def as_dict(self):
        return dict(in_image_components=self.total, in_image_components_differing=self.diff, in_image_share=self.share(),
                    max_abs_fp32=self.max32, max_abs_fp32_in_image=self.max32_in, max_abs_p64_vs_oracle=self.max64_oracle,
                    max_abs_p64_vs_ray_fed=self.max64_rays, max_abs_p64_vs_oracle_all_points=self.max64_oracle_all)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def restated_offsets(f, start, fs):
    """The knot offsets of a pixel frame restated in numpy, every operation rounded on its own: row_time
    (frame_time + ro * (y / rows)), the base knot (the floor of the earliest row time's knot, sync_problem.cpp
    frame_record) and knot_offset ((ts - start) * fs - base), rounded once to fp32 -> (n, 2).  The oracle-fed library
    computes its offsets with the same rs::knot_offset as the pixel-fed one, so only this restatement is independent of
    that function (and of how a compiler contracts it)."""
    ro, rows = f["lens"][0], float(f["rows"])
    tsa, tsb = f["ta"] + ro * (f["pa"][:, 1] / rows), f["tb"] + ro * (f["pb"][:, 1] / rows)
    base = np.floor((min(tsa.min(), tsb.min()) - start) * fs)
    return np.stack([(tsa - start) * fs - base, (tsb - start) * fs - base], axis=-1).astype(np.float32)


def compare_streams(hp, hr, f, tally, gyro=None):
    """the fp32 streams of one frame, pixel-fed against oracle-fed: every component within one fp32 ulp of 1, the time
    columns bit-equal, everywhere; the differing components of the in-image tracks are counted.  With the gyro given, the
    time columns of a pixel frame are also bit-equal to restated_offsets."""
    n = len(f["pa"])
    a1, b1 = hp.frame_rays(f["id"], cap=max(n, 1))
    a2, b2 = hr.frame_rays(f["id"], cap=max(n, 1))
    assert a1.shape == a2.shape == (n, 4) and b1.shape == b2.shape == (n, 4)
    assert np.isfinite(a1).all() and np.isfinite(b1).all() and np.isfinite(a2).all() and np.isfinite(b2).all()
    da, db = np.abs(a1 - a2), np.abs(b1[:, :2] - b2[:, :2])
    worst = max(float(da.max()), float(db.max()))
    tally.max32 = max(tally.max32, worst)
    assert worst <= RAY_TOL32, (f["id"], worst)
    np.testing.assert_array_equal(u32(b1[:, 2:]), u32(b2[:, 2:]))
    if gyro is not None and not f["rays"] and n:
        np.testing.assert_array_equal(u32(b1[:, 2:]), u32(restated_offsets(f, gyro.t0, gyro.fs)))
    m = both_in_image(f)
    if m.any():
        tally.total += 8 * int(m.sum())
        tally.diff += int((a1[m] != a2[m]).sum() + (b1[m] != b2[m]).sum())
        tally.max32_in = max(tally.max32_in, float(da[m].max()), float(db[m].max()))
    return a1, b1


def compare_p64(hp, hr, o, f, tally, delays=DELAYS):
    """the fp64 streams of one frame through problem_matrix64 (rship_debug_problem64 reads q0..q3: row64 of
    tests/cpu_device/rship_cpu.cpp, debug_problem64_kernel on the device): against the oracle's P and against the library
    fed the oracle's rays, both at 1e-13, on the in-image tracks"""
    n, m = len(f["pa"]), both_in_image(f)
    if n < 2:   # (the library's fp64 side refuses such a frame: "fewer than 2 tracks")
        return
    for d in delays:
        P = hp.problem_matrix64(f["id"], d, n)
        Po = o.problem_matrix(f["id"], d)
        Pr = hr.problem_matrix64(f["id"], d, n)
        assert P.shape == Po.shape == Pr.shape == (n, 3)
        tally.max64_oracle_all = max(tally.max64_oracle_all, float(np.abs(P - Po).max()))
        if m.any():
            e1, e2 = float(np.abs(P - Po)[m].max()), float(np.abs(P - Pr)[m].max())
            tally.max64_oracle = max(tally.max64_oracle, e1)
            tally.max64_rays = max(tally.max64_rays, e2)
            assert e1 < P_TOL64 and e2 < P_TOL64, (f["id"], d, e1, e2)


def same_streams(p, q, frames):
    """two library problems hold the same bits in the fp32 streams of every frame"""
    for f in frames:
        n = max(len(f["pa"]), 1)
        (a1, b1), (a2, b2) = p.frame_rays(f["id"], cap=n), q.frame_rays(f["id"], cap=n)
        np.testing.assert_array_equal(u32(a1), u32(a2))
        np.testing.assert_array_equal(u32(b1), u32(b2))


# ---- the lens check (sections 1-3): one problem per lens, one frame per point set -------------------------------------
def lens_frames(lens, cols, rows, seed, n=1024):
    from rssync_amd import synth
    return [frame(i, i / synth.FPS, (i + 1) / synth.FPS, pa, pb, lens, rows, cols)
            for i, (_, pa, pb) in enumerate(point_sets(lens, cols, rows, seed, n))]


def check_lens(make, name, seed):
    """-> Tally of one lens: streams everywhere, fp64 rows on the in-image tracks"""
    from rssync_amd import synth
    lens, cols, rows = lenses()[name]
    frames = lens_frames(lens, cols, rows, seed)
    gyro = synth.make_gyro(0.0, (len(frames) + 2) / synth.FPS, seed=seed)
    hp, hr = feed(make(), gyro, frames, "pixels"), feed(make(), gyro, frames, "oracle")
    o = oracle_problem(gyro, frames, seed)
    t = Tally()
    for f in frames:
        compare_streams(hp, hr, f, t, gyro)
        compare_p64(hp, hr, o, f, t)
    return t


# ---- the non-finite counter (section 6) -------------------------------------------------------------------------------
COUNTER_ARGS = (0.0, 0, 130, 0.004, 0.06)
COUNTER_BAD = {3: 5, 70: 0, 100: 48, 5: 7, 90: 1}   # frame -> tracks whose both ends are exactly (0, 0)
COUNTER_K = 48 * 3 + 600 * 2 - sum(COUNTER_BAD.values())   # the other tracks of those frames: 1283


def counter_scene():
    """130 frames (two shards when the object has two contexts: the cut is at 64 frames), 48 tracks each but six of 600"""
    from rssync_amd import synth
    sizes = [48] * 130
    for fr in (5, 40, 66, 90, 110, 129):
        sizes[fr] = 600
    gyro = synth.make_gyro(0.0, 132 / synth.FPS, seed=8)
    frames = []
    for fr, n in enumerate(sizes):
        _, ta, tb, pa, pb = next(iter(synth.make_pixel_frames(gyro, fr, fr + 1, n, seed=8)))
        frames.append(frame(fr, ta, tb, pa, pb, synth.LENS, ROWS, COLS))
    return gyro, frames


def check_counter(make, contexts=1):
    """Frames of two size classes set with fx = 0 (every centred x is infinite), a known number of their tracks with both
    ends at exactly (0, 0) -- finite by the reference's quirk: PreSync names exactly the other tracks, summed over the
    kernel's blocks, the classes and the object's contexts (contexts = 2: set_devices([0, 0]), checked with
    device_count); the same frames set again with the good lens give the bits of a fresh problem.  Input validation: the
    kernel writes its rows and counts them, nothing aborts.  -> the K the message named"""
    import re
    import rssync_amd
    from rssync_amd import synth
    gyro, frames = counter_scene()
    fresh = feed(make(), gyro, frames, "pixels")
    want = fresh.PreSync(*COUNTER_ARGS)
    p = make()
    if contexts > 1:
        p.set_devices([0] * contexts)
    assert p.device_count() == contexts
    feed(p, gyro, frames, "pixels")
    assert p.PreSync(*COUNTER_ARGS) == want
    bad_lens = list(synth.LENS)
    bad_lens[1] = 0.0
    K = 0
    for fr, zeros in COUNTER_BAD.items():
        f = frames[fr]
        pa, pb = f["pa"].copy(), f["pb"].copy()
        where = np.linspace(0, len(pa) - 1, zeros).astype(int)
        pa[where], pb[where] = 0.0, 0.0
        if len(pa) > zeros + 2:        # (0, 0) at one end only does not save a track
            rest = np.setdiff1d(np.arange(len(pa)), where)
            pa[rest[0]], pb[rest[1]] = 0.0, 0.0
        p.set_track_pixels(fr, f["ta"], f["tb"], pa, pb, bad_lens, ROWS)
        K += len(pa) - zeros
    named = None
    for _ in range(2):   # the count does not accumulate from call to call
        try:
            p.PreSync(*COUNTER_ARGS)
        except rssync_amd.RsSyncError as e:
            msg = str(e)
        else:
            raise AssertionError("PreSync accepted non-finite rays")
        assert "non-finite numbers in rays (%d tracks; lens parameters?)" % K in msg, (K, msg)
        named = int(re.search(r"rays \((\d+) tracks", msg).group(1))
    assert p.device_count() == contexts
    for fr in COUNTER_BAD:
        set_frame(p, frames[fr], "pixels")
    same_streams(p, fresh, frames)
    assert p.PreSync(*COUNTER_ARGS) == want
    return named


# ---- row times (section 5) ----------------------------------------------------------------------------------------------
ROWTIME_T0 = 3600.0
ROWTIME_EPS = 1e-9   # knots above an integer knot: the fp32 ulp there (9e-17) is far below the product's rounding error


def rowtime_frames(lens, cols, rows, fs, gyro_t0, seed, t_begin=ROWTIME_T0, n=256):
    """frame 0: y from a quarter image above the first row to a quarter below the last.  Frames 1..6: the frame time lies
    ROWTIME_EPS knots above a gyro knot and no row is negative, so the A ends with y = 0 or y tiny have knot offsets of
    1e-9 .. 1e-4 -- where (ts - start) * fs is inexact, its rounding (~1e-14 at knot 100) is then worth many fp32 ulps,
    and a fused multiply-subtract shows in the fp32 stream"""
    from rssync_amd import synth
    rng = np.random.default_rng([seed, 43])
    ro = lens[0]
    out = []
    pa, pb = _uniform(rng, n, cols, rows), _uniform(rng, n, cols, rows)
    pa[:, 1], pb[:, 1] = rng.uniform(-0.25 * rows, 1.25 * rows, size=n), rng.uniform(-0.25 * rows, 1.25 * rows, size=n)
    out.append(frame(0, t_begin + 0.01, t_begin + 0.01 + 1 / synth.FPS, pa, pb, lens, rows, cols))
    for i in range(1, 7):
        knot = np.round((t_begin + 0.01 + i / synth.FPS - gyro_t0) * fs)
        ta = gyro_t0 + (knot + ROWTIME_EPS) / fs
        pa, pb = _uniform(rng, n, cols, rows), _uniform(rng, n, cols, rows)
        pa[:16, 1] = 0.0
        if ro > 0:   # row times 1e-9 .. 1e-4 knots after the frame's
            pa[16:n // 2, 1] = rows * 10.0 ** rng.uniform(-9, -4, size=n // 2 - 16) / (ro * fs)
        out.append(frame(i, ta, ta + 1 / synth.FPS, pa, pb, lens, rows, cols))
    for i in range(7, 13 if ro > 0 else 7):
        # frames 7..12: the earliest rows lie deep in the image, so the readout's share ro * (y / rows) is a tenth of the
        # row time and not 1e-9 of it, and it is THEIR row time that lies just above a knot: A ends a few 1e-10 knots
        # apart (128 per frame), each with its own rounding of the product -- where fusing row_time moves the sum, the fp32 stream shows it
        y0 = rows * (0.3 + 0.1 * (i - 7))
        knot = np.round((t_begin + 0.02 + (i - 6) / synth.FPS - gyro_t0) * fs)
        ta = gyro_t0 + (knot + ROWTIME_EPS) / fs - ro * (y0 / rows)
        pa, pb = _uniform(rng, n, cols, rows), _uniform(rng, n, cols, rows)
        pa[:, 1] = rng.uniform(y0, rows, size=n)
        pa[:128, 1] = y0 + np.arange(128) * (rows * 1e-10 / (ro * fs))
        out.append(frame(i, ta, ta + 1 / synth.FPS, pa, pb, lens, rows, cols))
    return out


def _fl(x):
    return float(x)   # Fraction -> the nearest double


def fused_screen(frames, start, fs):
    """Do these inputs make the two products inexact?  Restates the A ends' knot offsets of the library
    (row_time, then knot_offset, every operation rounded) and two deliberately contracted variants in exact rational
    arithmetic -> (fp32 offsets that differ with knot_offset fused, with row_time fused, fp64 row times that differ with
    row_time fused, points)"""
    n_knot = n_row32 = n_row64 = total = 0
    for f in frames:
        ro, rows, ta = f["lens"][0], float(f["rows"]), f["ta"]
        y = f["pa"][:, 1]
        yb = f["pb"][:, 1]
        ts = ta + ro * (y / rows)
        ts_min = min(ts.min(), (f["tb"] + ro * (yb / rows)).min())
        base = np.floor((ts_min - start) * fs)
        plain = ((ts - start) * fs - base).astype(np.float32)
        for i in range(len(y)):
            fused = np.float32(_fl(Fraction(float(ts[i] - start)) * Fraction(fs) - Fraction(float(base))))
            n_knot += int(fused != plain[i])
            ts_f = _fl(Fraction(ta) + Fraction(ro) * Fraction(float(y[i] / rows)))
            n_row64 += int(ts_f != ts[i])
            n_row32 += int(np.float32((ts_f - start) * fs - base) != plain[i])
        total += len(y)
    return n_knot, n_row32, n_row64, total
