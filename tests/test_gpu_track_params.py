"""LK on the device (csrc/kernels/track.hpp, csrc/kernels/features.hpp) against the fp64 numpy reference
(tests/track_reference.py, tests/feature_reference.py) over the parameter range the public headers accept -- windows
3 .. 21, levels 1 .. 8, any max_iters / epsilon / min_eig -- and at the frame edges: points on the last column and row,
frames only a little wider than the window, the smallest frames a pyramid allows, coordinates near x = 4000.

The frames are synthetic (tests/track_scenes.py): band-limited texture moved by a known shift and quantised to uint8.
fp32 and fp64 may split where a point sits on a decision's threshold; the reference reports how close each point came to
every decision it took (track_pair(..., diag=True)), such points are excused from the status and flow comparison, and
each comparison bounds how many it excused, so that a sweep cannot pass by excusing itself."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import feature_reference as fr
import track_reference as tr
import track_scenes as ts

pytestmark = pytest.mark.gpu

FLOW_TOL = 1e-3        # px: tests/test_gpu_track.py's bound for the flow of a status-0 point
RES_TOL = 1e-2         # mean |I_b - T|, pixel values
NEAR_FRACTION = 0.02   # at most this share of a comparison's points may be excused as near a decision
OK, ILL, LEFT, CAP = tr.STATUS_OK, tr.STATUS_ILL, tr.STATUS_LEFT, tr.STATUS_CAP


def _problem():
    import rssync_amd
    return rssync_amd.SyncProblem(seed=321)


def _lk(**kw):
    """the tracker's parameters with the defaults filled in (what track_pair needs)"""
    out = dict(window=21, levels=4, max_iters=30, epsilon=0.01, min_eig=1e-4)
    out.update(kw)
    return out


def _ref_kw(lk):
    return {k: lk[k] for k in ("window", "max_iters", "epsilon", "min_eig")}


def _compare(what, flow, st, res, ref, epsilon, flow_status=(OK,), stats=None):
    """flow (P, 2), st, res of the device against track_pair(..., diag=True)'s ref: statuses equal and flows within
    FLOW_TOL for the points of a status in flow_status, residuals within RES_TOL at status 0 -- for every point that is not
    near a decision.  -> (near points, largest flow difference)"""
    rf, rst, rres, m = ref
    near = tr.near_decision(m, epsilon)
    far = ~near
    bad = far & (st != rst)
    assert not bad.any(), "%s: statuses %s, reference %s at %s" % (what, st[bad], rst[bad], np.nonzero(bad)[0])
    sel = far & np.isin(rst, flow_status)
    d = float(np.abs(flow - rf)[sel].max()) if sel.any() else 0.0
    assert d <= FLOW_TOL, (what, d)
    ok = far & (rst == OK)
    if ok.any():
        assert np.abs(res - rres)[ok].max() <= RES_TOL, (what, np.abs(res - rres)[ok].max())
    if stats is not None:
        stats.append((what, int(near.sum()), len(st), d))
    return int(near.sum()), d


def _report(name, stats):
    print("\n%s: %d comparisons, %d of %d points near a decision" % (name, len(stats), sum(s[1] for s in stats),
                                                                    sum(s[2] for s in stats)))
    for what, n, P, d in stats:
        print("  %-40s near %3d / %4d   max |flow - ref| %.2e" % (what, n, P, d))


def _bound_near(stats):
    """the points a test excused, over all its comparisons, stay under NEAR_FRACTION"""
    near, total = sum(s[1] for s in stats), sum(s[2] for s in stats)
    assert near <= NEAR_FRACTION * total, (near, total)


def _grid_run(p, frames, step, lk):
    """track_points and the reference (with margins) of the pair frames[0] -> frames[1]"""
    pa, pb, st, res = p.track_points(frames, grid_step=step, **lk)
    pyrs = [tr.pyramid(f, lk["levels"]) for f in frames[:2]]
    ref = tr.track_pair(pyrs[0], pyrs[1], pa, diag=True, **_ref_kw(lk))
    return pa, pb[0] - pa, st[0], res[0], ref


# ---------------------------------------------------------------------------------------------------------------------
# window x levels

SWEEP_SHIFT = {1: (0.35, -0.6), 2: (1.3, -2.2), 4: (5.3, -7.6), 8: (14.7, 19.4)}   # within reach of each pyramid


def test_window_by_levels_sweep(built):
    """windows 3 .. 21 put the window's area on both sides of 64 and 128 (1 .. 7 samples per lane); levels 1 .. 8"""
    p = _problem()
    stats, per_window, tracked = [], {}, 0
    for levels, (sx, sy) in SWEEP_SHIFT.items():
        w, h = (300, 260) if levels == 8 else (260, 200)     # every level at least 3 x 3
        frames = ts.multiscale_frames(w, h, [(0.0, 0.0), (sx, sy)])
        for window in (3, 5, 7, 9, 11, 15, 21):
            lk = _lk(window=window, levels=levels)
            pa, flow, st, res, ref = _grid_run(p, frames, 20, lk)
            what = "window %d levels %d" % (window, levels)
            _, d = _compare(what, flow, st, res, ref, lk["epsilon"], stats=stats)
            assert (ref[1] == OK).mean() >= 0.25, (what, np.bincount(ref[1]))   # (a 3 x 3 window on 8 levels: 1 / 3)
            tracked += int((ref[1] == OK).sum())
            per_window[window] = max(per_window.get(window, 0.0), d)
    _report("window x levels", stats)
    _bound_near(stats)
    assert tracked >= 0.7 * sum(s[2] for s in stats), tracked
    print("  largest flow difference per window: %s" % {k: "%.1e" % v for k, v in per_window.items()})


# ---------------------------------------------------------------------------------------------------------------------
# stopping rules

def test_stopping_rules(built):
    """max_iters 1 .. 3, epsilon 1e-4 .. 1, min_eig up to the grid's median: each run produces the statuses it targets"""
    p = _problem()
    frames = ts.multiscale_frames(260, 200, [(0.0, 0.0), (2.6, -1.7)])
    me = tr.min_eigenvalue(frames[0], tr.grid(260, 200, 20), 9)
    big = float(np.quantile(me, 0.4))                       # ~40 % of the grid ill-conditioned at window 9
    cases = [
        (dict(max_iters=1, epsilon=1e-4), {CAP}),
        (dict(max_iters=2, epsilon=1e-4), {CAP}),
        (dict(max_iters=3, epsilon=0.05), {OK, CAP}),
        (dict(max_iters=3, epsilon=1.0), {OK}),
        (dict(max_iters=30, epsilon=1e-4), {OK}),
        (dict(max_iters=2, epsilon=0.3), {OK, CAP}),
        (dict(min_eig=big), {OK, ILL}),
        (dict(min_eig=big, max_iters=1, epsilon=1e-4), {ILL, CAP}),
    ]
    stats = []
    for kw, want in cases:
        lk = _lk(window=9, levels=3, **kw)
        pa, flow, st, res, ref = _grid_run(p, frames, 20, lk)
        what = " ".join("%s=%g" % kv for kv in sorted(kw.items()))
        _compare(what, flow, st, res, ref, lk["epsilon"], flow_status=(OK, CAP), stats=stats)
        got = set(np.unique(st).tolist())
        assert want <= got, (what, want, np.bincount(st))
    _report("stopping rules", stats)
    _bound_near(stats)


# ---------------------------------------------------------------------------------------------------------------------
# frame edges

def test_border_points(built):
    """points on column width-1 and row height-1 (width = 2 step + 1), a 21 x 21 window on frames hardly wider than it
    (clamped template and gradient samples), and content moved far enough that points leave at a coarse level (the
    LEFT_IMAGE break and its rescale), and one level with epsilon = 0.5, where the first update converges and carries
    the last column's points just outside: only the final level-0 test can find them.  Statuses and final flows are
    compared for status 2 as well as 0"""
    p = _problem()
    stats = []
    left_coarse = 0
    cases = [  # (w, h, step, levels, epsilon, shifts of the frames)
        (25, 25, 12, 4, 0.01, [(0, 0), (0.4, -0.3), (1.6, 0.9), (-2.5, 3.2), (4.0, -4.5), (9.0, 1.0)]),
        (21, 31, 10, 3, 0.01, [(0, 0), (0.6, 0.2), (-1.2, 2.1), (3.3, -0.7), (-7.0, 5.0)]),
        (41, 33, 20, 3, 0.01, [(0, 0), (0.3, 0.3), (2.2, -1.4), (-6.5, -3.5)]),
        (161, 97, 16, 4, 0.01, [(0, 0), (40.0, 0.0), (-28.0, 17.0), (0.0, -35.0)]),
        (25, 25, 12, 1, 0.5, [(0, 0), (0.3, 0.2), (0.5, 0.4), (0.8, 0.6)]),
    ]
    final_out = 0
    for w, h, step, levels, eps, shifts in cases:
        frames = ts.multiscale_frames(w, h, shifts)
        lk = _lk(window=21, levels=levels, epsilon=eps)
        pa, pb, st, res = p.track_points(frames, grid_step=step, **lk)
        assert (pa[:, 0] == w - 1).any() or (pa[:, 1] == h - 1).any() or w == 161
        pyrs = [tr.pyramid(f, levels) for f in frames]
        for k in range(len(frames) - 1):
            ref = tr.track_pair(pyrs[k], pyrs[k + 1], pa, diag=True, **_ref_kw(lk))
            what = "%dx%d step %d pair %d" % (w, h, step, k)
            _compare(what, pb[k] - pa, st[k], res[k], ref, lk["epsilon"], flow_status=(OK, LEFT), stats=stats)
            left_coarse += int((ref[3]["left_level"] > 0).sum())
            final_out += int(((ref[1] == LEFT) & (ref[3]["left_level"] < 0)).sum())
    assert left_coarse >= 5, left_coarse                     # the coarse-level break was taken
    assert final_out >= 2, final_out                         # and the final level-0 test decided some
    _report("border points (%d left at a coarse level)" % left_coarse, stats)
    _bound_near(stats)


@pytest.mark.parametrize("levels", range(1, 9))
def test_smallest_frames(built, levels):
    """2^L + 1 on each side is the smallest frame for L levels (top level 3 x 3); 2^L on either side is refused.  LK with
    the 21 x 21 window at every size, and the 3 x 3 window up to L = 2: from L = 3 on, a 3 x 3 window wanders on the
    blurred 3 x 3 .. 9 x 9 top levels, and such an iteration amplifies rounding from step to step -- the fp64 reference
    itself moves some of those points by tens of px when its pyramid is scaled by 1 + 1e-6 N(0, 1)."""
    import rssync_amd
    from rssync_amd import track
    p = _problem()
    s = 2 ** levels + 1
    frames = ts.multiscale_frames(s, s, [(0.0, 0.0), (0.4, -0.3), (-0.7, 0.2)])
    if levels > 1:
        got = track.pyramid(p, frames, levels)
        assert got[-1].shape[1:] == (3, 3)
        for k in range(len(frames)):
            for lv, (g, want) in enumerate(zip(got, tr.pyramid(frames[k], levels)[1:])):
                np.testing.assert_array_equal(g[k], want, err_msg="%dx%d level %d" % (s, s, lv + 1))
    step = max(1, s // 10)
    stats = []
    for window in ((3, 21) if levels <= 2 else (21,)):
        lk = _lk(window=window, levels=levels)
        pa, pb, st, res = p.track_points(frames, grid_step=step, **lk)
        pyrs = [tr.pyramid(f, levels) for f in frames]
        for k in range(2):
            ref = tr.track_pair(pyrs[k], pyrs[k + 1], pa, diag=True, **_ref_kw(lk))
            _compare("%dx%d window %d pair %d" % (s, s, window, k), pb[k] - pa, st[k], res[k], ref, lk["epsilon"],
                     flow_status=(OK, CAP, LEFT), stats=stats)
    assert sum(x[1] for x in stats) <= max(1, NEAR_FRACTION * sum(x[2] for x in stats)), stats
    for w, h in ((s - 1, s), (s, s - 1)):
        with pytest.raises(rssync_amd.RsSyncError, match="too small for"):
            p.track_points(np.zeros((2, h, w), np.uint8), grid_step=1, levels=levels)


def test_pyramid_shapes(built):
    """levels 2 .. 8, widths a multiple of the 32-wide output tile at level 1 and one either side of it, heights whose
    levels fall below the 8-row tile, pitch > width: bit for bit"""
    from rssync_amd import track
    p = _problem()
    rng = np.random.default_rng(17)
    for levels in range(2, 9):
        t = max(2, 2 ** levels // 64 + 1)
        for w in (64 * t - 2, 64 * t - 1, 64 * t, 64 * t + 1, 64 * t + 2):   # level 1: 32 t - 1, 32 t, 32 t + 1
            for h in (2 ** levels + 1, 2 ** levels + 6, 3 * 2 ** (levels - 1) + 3):
                wide = rng.integers(0, 256, size=(2, h, w + 19), dtype=np.uint8)
                frames = wide[:, :, 5:5 + w]
                got = track.pyramid(p, frames, levels)
                for k in range(2):
                    want = tr.pyramid(frames[k], levels)[1:]
                    assert len(got) == len(want) == levels - 1
                    for lv, (g, wv) in enumerate(zip(got, want)):
                        assert g[k].shape == wv.shape
                        np.testing.assert_array_equal(g[k], wv, err_msg="%dx%d levels %d level %d" % (w, h, levels, lv + 1))


# ---------------------------------------------------------------------------------------------------------------------
# large coordinates

def test_large_coordinates_keep_subpixel_resolution(built):
    """A 4096 px wide pair whose content repeats every 1024 px, moved by (0.37, -0.21) px: points near x = 3900 get the
    reference's flow to 1e-3 px, the true shift to the window's bilinear bias, and bit for bit the flow of the same
    content 3072 px to the left (the integer base plus an fp32 offset: no precision is lost to the coordinate)"""
    from rssync_amd import features
    W, H, SX, SY, PERIOD = 4096, 80, 0.37, -0.21, 1024
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    xm = np.mod(xs, PERIOD)
    frames = np.stack([ts.multiscale(xm, ys, 8, 256), ts.multiscale(xm - SX, ys - SY, 8, 256)])
    far = np.array([(x, y) for x in range(3880, 3921, 4) for y in range(30, 51, 10)], np.int32)   # 33 points
    near = far - (3 * PERIOD, 0)                             # x = 808 .. 848: the same content
    pts = np.concatenate([far, near])
    lk = _lk(window=21, levels=4)
    p = _problem()
    flow, st, _ = features.track_list(p, frames, pts[None], np.array([len(pts)], np.uint32))
    flow, st = flow[0].astype(np.float64), st[0]
    pyrs = [tr.pyramid(f, 4) for f in frames]
    rf, rst, _ = tr.track_pair(pyrs[0], pyrs[1], pts.astype(np.float64), **_ref_kw(lk))
    assert (st == OK).all() and (rst == OK).all(), (st, rst)
    d = np.abs(flow - rf).max()
    assert d <= FLOW_TOL, d
    np.testing.assert_array_equal(flow[:len(far)], flow[len(far):])
    err = np.linalg.norm(flow - (SX, SY), axis=-1)
    rerr = np.linalg.norm(rf - (SX, SY), axis=-1)
    # the reference's own bias against the true shift is the window's (tests/test_track_cpu.py: up to ~0.04 px)
    assert rerr.max() <= 0.05 and err.max() <= rerr.max() + FLOW_TOL, (err.max(), rerr.max())
    print("\nlarge coordinates: max |flow - ref| %.2e, max error against the shift %.3f px" % (d, err.max()))


# ---------------------------------------------------------------------------------------------------------------------
# forward-backward

# fb errors of the device against the reference, away from any LK decision: at most 3.4e-5 px measured (8 levels; 8e-7 px
# at 1 level).  FB_TOL is three times that: the fb errors must agree to it, so a status can split at the fb bound only
# for a track whose reference fb error is within FB_TOL of it -- those are excused and counted with the near ones.
FB_TOL = 1e-4


def _fb_compare(what, cnt, pts, ff, fbk, st, fb, pyrs, frame0, max_fb, lk, stats):
    a = fr.detect(frame0, 32)
    n = cnt
    np.testing.assert_array_equal(pts[:n], a)
    st, ff, fbk, fb = st[:n], ff[:n], fbk[:n], fb[:n]
    rf, rb, rst, rfb, m = fr.track_fb(pyrs[0], pyrs[1], a, max_fb, diag=True, **_ref_kw(lk))
    excused = tr.near_decision(m, lk["epsilon"]) | fr.fb_edge(rfb, max_fb, FB_TOL)
    bad = ~excused & (st != rst)
    assert not bad.any(), (what, st[bad], rst[bad])
    fwd = (rst % 4 == 0) & ~excused                        # forward status 0: a full forward pass and a backward pass
    d = float(np.abs(ff - rf)[fwd].max()) if fwd.any() else 0.0
    assert d <= FLOW_TOL, (what, d)
    if fwd.any():
        assert np.abs(fbk - rb)[fwd].max() <= FLOW_TOL, what
        assert np.abs(fb - rfb)[fwd].max() <= FB_TOL, (what, np.abs(fb - rfb)[fwd].max())
    assert np.isnan(fb[st % 4 != 0]).all()
    stats.append((what, int(excused.sum()), int(n), d))
    return rst


def test_forward_backward_across_the_range(built):
    """windows 3, 9, 21 at levels 1 and windows 9, 21 at levels 8, with a max_fb_error small enough that some tracks fail
    the check (status 4).  Forward flows are compared for status 0 and 4 alike, backward flows and fb errors wherever the
    backward pass ran.  (The 3 x 3 window on 8 levels wanders on the 3 x 3 .. 10 x 9 top levels of a 320 x 272 frame,
    see test_smallest_frames; test_window_by_levels_sweep compares it on the grid.)"""
    from rssync_amd import features
    p = _problem()
    stats = []
    for levels, shift, max_fb in ((1, (0.45, -0.3), 0.004), (8, (6.2, -3.9), 0.004)):
        frames = ts.multiscale_frames(320, 272, [(0.0, 0.0), shift])
        pyrs = [tr.pyramid(f, levels) for f in frames]
        for window in ((3, 9, 21) if levels == 1 else (9, 21)):
            lk = _lk(window=window, levels=levels)
            cnt, pts, ff, fbk, st, fb = features.raw_features(p, frames, cell=32, max_fb_error=max_fb, **lk)
            what = "window %d levels %d" % (window, levels)
            rst = _fb_compare(what, cnt[0], pts[0], ff[0], fbk[0], st[0], fb[0], pyrs, frames[0], max_fb, lk, stats)
            assert (rst == fr.STATUS_FB_MISMATCH).any() and (rst == OK).any(), (what, np.bincount(rst))
    _report("forward-backward", stats)
    _bound_near(stats)


def test_backward_pass_from_a_tiny_negative_flow(built):
    """Frame b is frame a except beyond a few columns, so that the coarse levels move a feature and level 0, whose content
    is unchanged, brings it back towards 0.  Binary content (0 / 200) keeps fp32 iterating until the bilinear weight
    itself rounds: a flow in (-2^-25, 0) leaves fx = flow - floor(flow) = 1 in fp32 (the lkfb kernel's roll-over to the
    next integer base).  Such tracks' backward passes match the reference started from a + flow.

    This checks that the path runs and agrees with the reference; it does not guard the roll-over line itself: base
    bx - 1 with fraction 1.0 is the same start as base bx with fraction 0 -- the same levels, border tests and floors,
    samples within an ulp -- so the results without the roll-over differ far inside FLOW_TOL."""
    from rssync_amd import features
    rng = np.random.default_rng(23)
    blocks = rng.integers(0, 2, size=(34, 40)).astype(np.uint8) * 200
    a = np.kron(blocks, np.ones((8, 8), np.uint8))           # 272 x 320
    b = a.copy()
    b[:, 200:] = np.roll(a, -3, axis=1)[:, 200:]            # beyond x = 200 the content moves 3 px to the left
    frames = np.stack([a, b])
    lk = _lk(window=9, levels=4, max_iters=100, epsilon=1e-9)
    p = _problem()
    cnt, pts, ff, fbk, st, fb = features.raw_features(p, frames, cell=16, quality=0.01, max_fb_error=0.5, **lk)
    n = cnt[0]
    fx = ff[0, :n].astype(np.float32)
    frac = fx - np.floor(fx)
    roll = ((frac == np.float32(1.0)) & (fx < 0)).any(axis=1) & (st[0, :n] % 4 == 0)
    assert roll.sum() >= 1, (n, np.sort(np.abs(fx[fx < 0]))[:8])
    pyrs = [tr.pyramid(f, 4) for f in frames]
    i = np.nonzero(roll)[0]
    start = pts[0, i].astype(np.float64) + ff[0, i].astype(np.float64)       # the kernel's b = a + flow
    rb, rst, _ = tr.track_pair(pyrs[1], pyrs[0], start, **_ref_kw(lk))
    # (no margins here: epsilon = 1e-9 is below fp32's resolution on purpose, so every convergence test is "near"; the
    # backward pass converges to the start in both, which is what is compared)
    assert (rst == OK).all(), rst
    assert np.abs(fbk[0, i] - rb).max() <= FLOW_TOL, np.abs(fbk[0, i] - rb).max()
    print("\ntiny negative flow: %d tracks roll over, backward flow within %.1e of the reference" %
          (roll.sum(), np.abs(fbk[0, i] - rb).max()))


# ---------------------------------------------------------------------------------------------------------------------
# repeatability

def test_repeatable_at_a_non_default_configuration(built):
    from rssync_amd import features
    p = _problem()
    frames = ts.multiscale_frames(300, 260, [(0.0, 0.0), (3.1, -2.4), (5.5, 1.2)])
    lk = _lk(window=7, levels=6, max_iters=5, epsilon=0.02, min_eig=0.5)
    one = p.track_points(frames, grid_step=13, **lk)
    two = p.track_points(frames, grid_step=13, **lk)
    for x, y in zip(one, two):
        np.testing.assert_array_equal(x, y)
    f1 = features.raw_features(p, frames, cell=24, max_fb_error=0.05, **lk)
    f2 = features.raw_features(p, frames, cell=24, max_fb_error=0.05, **lk)
    for x, y in zip(f1, f2):
        np.testing.assert_array_equal(x, y)
