"""The path limiter on the device (include/rssync_limit.h, csrc/kernels/limit.hpp): the fit against the header's procedure
run on the host through rssync_stabilize_path and rssync_stabilize_coverage, bit for bit, and against the numpy restatement
(tests/limit_reference.py); every frame alone against the batch; the anchors; fit, envelope and targets end to end through
the grayscale and the NV12 renderer; the errors."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import limit_reference as lr
import rectify_reference as rr
import stabilize_reference as sr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

W, H = rr.COLS, rr.ROWS
TINY_W, TINY_H = 96, 64        # fewer than 255 rows: threads without a table entry
MIXED_ZOOMS = (1.0, 1.03, 1.059, 1.08, 1.1, 1.03, 1.0, 1.06, 1.2)


@pytest.fixture(scope="module")
def scene(built):
    import rssync_amd
    s = dict(rr.scene())
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(s["gyro"].quats, s["gyro"].fs, s["gyro"].t0)
    s["problem"] = p
    np.testing.assert_array_equal(s["times"], lr.TIMES[zr.SCENE])
    return s


def _kw(case, **more):
    """the keywords the device calls share with the reference's case"""
    c = lr.CASES[case]
    kw = dict(sigma=lr.SIGMA, camera=c["camera"])
    if c["out_size"] is not None:
        kw["out_size"] = c["out_size"]
    kw.update(more)
    return kw


def _tiny_lens(lens):
    sx, sy = TINY_W / W, TINY_H / H
    return (lens[0], lens[1] * sx, lens[2] * sy, lens[3] * sx, lens[4] * sy) + tuple(lens[5:])


def _host_fit(p, width, height, lens, times, zooms, steps, targets=None, sigma=lr.SIGMA, **kw):
    """the header's procedure for all frames at once: r and g from rssync_stabilize_path (or the caller's targets as given),
    the candidates blended in numpy in the header's order, clear(f, a) read from the existing coverage call with the
    candidates as explicit targets -- all frames' zooms go in as the sweep's zooms and the diagonal is read"""
    from rssync_amd import synth
    n = len(times)
    own = p.stabilize_path(times, lens[0], synth.D_TRUE, 0.0)
    goal = p.stabilize_path(times, lens[0], synth.D_TRUE, sigma) if targets is None else np.asarray(targets, np.float64)

    def clear(a):
        cand = np.stack([lr.blend(own[f], goal[f], a[f]) for f in range(n)])
        counts = p.stabilize_coverage(width, height, lens, times, synth.D_TRUE, zooms, targets=cand, **kw)
        return np.diagonal(counts) == 0

    clear_1, clear_0 = clear(np.ones(n)), clear(np.zeros(n))
    lo, hi = np.zeros(n), np.ones(n)
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        ok = clear(mid)
        lo = np.where(ok, mid, lo)
        hi = np.where(ok, hi, mid)
    strengths = np.where(clear_1, 1.0, np.where(clear_0, lo, 0.0))
    return strengths, (~clear_1 & ~clear_0).astype(np.uint32)


def _targets():
    """goals that are not unit quaternions: half the path at another sigma"""
    s = rr.scene()
    from rssync_amd import synth
    return 0.5 * sr.path64(s["gyro"], lr.TIMES, s["lens"][0], synth.D_TRUE, 0.3)


@pytest.fixture(scope="module")
def fitted(scene):
    """the device's fit of both cases (read-only)"""
    from rssync_amd import synth
    out = {}
    for name, c in lr.CASES.items():
        a, st = scene["problem"].fit_strength(W, H, scene["lens"], lr.TIMES, synth.D_TRUE, zoom=c["zoom"], steps=lr.STEPS, **_kw(name))
        a.setflags(write=False)
        st.setflags(write=False)
        out[name] = (a, st)
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------
FIT_CASES = {
    # id: (size, case, steps, zoom, more)
    "A": ("scene", "A", 10, None, {}),
    "B": ("scene", "B", 10, None, {}),                      # height != out_height
    "A-at-1.06-five-steps": ("scene", "A", 5, 1.06, {}),
    "A-targets": ("scene", "A", 10, None, {"targets": True}),
    "B-targets": ("scene", "B", 10, None, {"targets": True}),
    "A-one-step": ("scene", "A", 1, None, {}),
    "A-default-steps": ("scene", "A", 0, None, {}),
    "A-zooms": ("scene", "A", 10, MIXED_ZOOMS, {}),
    "B-zooms": ("scene", "B", 5, tuple(0.84 + 0.015 * k for k in range(9)), {}),
    "A-40x30": ("scene", "A", 10, 1.02, {"out_size": (40, 30)}),          # 136 border pixels: threads without one
    "A-two-iterations": ("scene", "A", 10, None, {"iterations": 2}),
    "tiny-lens": ("tiny", "A", 10, 1.05, {}),
    "tiny-pinhole": ("tiny", "B", 10, 0.9, {"out_size": (50, 40)}),
}


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fit_is_the_headers_procedure_on_the_host_bit_for_bit(scene, name):
    from rssync_amd import synth
    size, case, steps, zoom, more = FIT_CASES[name]
    p = scene["problem"]
    w, h, lens = (W, H, scene["lens"]) if size == "scene" else (TINY_W, TINY_H, _tiny_lens(scene["lens"]))
    more = dict(more)
    targets = _targets() if more.pop("targets", False) else None
    kw = _kw(case, **more)
    zoom = lr.CASES[case]["zoom"] if zoom is None else zoom
    n = len(lr.TIMES)
    if isinstance(zoom, tuple):
        zooms = np.array(zoom)
        got, status = p.fit_strength(w, h, lens, lr.TIMES, synth.D_TRUE, zooms=zooms, zoom=-3.0, steps=steps, targets=targets, **kw)
    else:
        zooms = np.full(n, zoom)
        got, status = p.fit_strength(w, h, lens, lr.TIMES, synth.D_TRUE, zoom=zoom, steps=steps, targets=targets, **kw)
    cover = {k: v for k, v in kw.items() if k != "sigma"}
    want, want_status = _host_fit(p, w, h, lens, lr.TIMES, zooms, steps if steps else 12, targets=targets, **cover)
    print(name, got.tolist(), status.tolist())
    assert got.dtype == np.float64 and status.dtype == np.uint32
    assert [float(v).hex() for v in got] == [float(v).hex() for v in want]
    np.testing.assert_array_equal(status, want_status)
    assert ((got >= 0) & (got <= 1)).all() and (got[status == 1] == 0).all()
    if name in ("A-zooms", "B-zooms"):          # all three branches of the procedure among the nine frames
        assert (status == 1).any() and (got == 1).any() and ((got > 0) & (got < 1)).any()
    if name in ("A", "B"):                      # (tests/limit_reference.py: FITTED)
        assert ((got > 0) & (got < 1)).sum() >= 3, got


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(lr.CASES))
def test_fit_lies_between_the_references_brackets(scene, fitted, case):
    """a device map within the map tolerance of the float64 one can count a border pixel differently only within that
    tolerance of a frame edge: conservative <= device <= liberal.  On these inputs the brackets coincide."""
    c = lr.CASES[case]
    frames = lr.frames(case)
    tol = sr.device_tolerance(c["camera"])
    liberal, _ = lr.fit64(frames, mode=lr.LIBERAL, tol=tol)
    conservative, _ = lr.fit64(frames, mode=lr.CONSERVATIVE, tol=tol)
    got, status = fitted[case]
    print(case, got.tolist())
    assert (conservative <= got).all() and (got <= liberal).all() and not status.any()
    np.testing.assert_array_equal(got, np.array(lr.FITTED[case]))


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_a_frames_result_does_not_depend_on_its_neighbours(scene, fitted):
    from rssync_amd import synth
    p, lens = scene["problem"], scene["lens"]
    for case in sorted(lr.CASES):
        z = lr.CASES[case]["zoom"]
        for f in range(len(lr.TIMES)):
            a, st = p.fit_strength(W, H, lens, lr.TIMES[f:f + 1], synth.D_TRUE, zoom=z, steps=lr.STEPS, **_kw(case))
            assert float(a[0]).hex() == float(fitted[case][0][f]).hex() and st[0] == fitted[case][1][f], (case, f)
        rev, st = p.fit_strength(W, H, lens, lr.TIMES[::-1], synth.D_TRUE, zoom=z, steps=lr.STEPS, **_kw(case))
        np.testing.assert_array_equal(rev[::-1], fitted[case][0])


def test_fit_of_more_frames_than_one_chunk_holds_tables_for(scene, fitted):
    """the nine times over and over, past the number of row tables the pipeline's buffer keeps (64 MiB of them, the zoom
    fit's constant): every frame's result is its own, whichever chunk and workgroup it fell into; without the status array"""
    from rssync_amd import limit, stabilize, synth
    p, lens, c = scene["problem"], scene["lens"], lr.CASES["B"]
    n = (64 << 20) // ((H + 1) * 36) + 10
    times = np.ascontiguousarray(np.resize(lr.TIMES, n))
    got, status = p.fit_strength(W, H, lens, times, synth.D_TRUE, zoom=c["zoom"], steps=lr.STEPS, **_kw("B"))
    np.testing.assert_array_equal(got, np.resize(fitted["B"][0], n))
    assert not status.any()
    lib = limit.library()
    L = np.ascontiguousarray(lens, np.float64)
    prm = stabilize.params(zoom=c["zoom"], **{k: v for k, v in _kw("B").items() if k != "out_size"})
    ow, oh = c["out_size"]
    alone = np.zeros(9)
    assert lib.rssync_limit_fit(p._h, W, H, L.ctypes.data, ow, oh, lr.TIMES.ctypes.data_as(C.POINTER(C.c_double)), 9, synth.D_TRUE, None,
                                C.byref(prm), None, lr.STEPS, alone.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    np.testing.assert_array_equal(alone, fitted["B"][0])


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_anchors(scene):
    from rssync_amd import limit, synth
    p, lens = scene["problem"], scene["lens"]
    ro = lens[0]
    own = p.stabilize_path(lr.TIMES, ro, synth.D_TRUE, 0.0)
    path = p.stabilize_path(lr.TIMES, ro, synth.D_TRUE, lr.SIGMA)
    goals = _targets()
    ones, zeros = np.ones(9), np.zeros(9)
    # strengths all 1: the goal's bits, whether it is the path or the caller's (not normalised)
    np.testing.assert_array_equal(p.strength_targets(lr.TIMES, ro, synth.D_TRUE, ones, sigma=lr.SIGMA).view(np.uint64), path.view(np.uint64))
    np.testing.assert_array_equal(p.strength_targets(lr.TIMES, ro, synth.D_TRUE, ones, targets=goals).view(np.uint64), goals.view(np.uint64))
    # strengths all 0: the path at sigma 0
    np.testing.assert_array_equal(p.strength_targets(lr.TIMES, ro, synth.D_TRUE, zeros, sigma=lr.SIGMA).view(np.uint64), own.view(np.uint64))
    np.testing.assert_array_equal(p.strength_targets(lr.TIMES, ro, synth.D_TRUE, zeros, targets=goals).view(np.uint64), own.view(np.uint64))
    # between: the header's blend of the two, bit for bit
    a = np.array(lr.FITTED["A"])
    got = p.strength_targets(lr.TIMES, ro, synth.D_TRUE, a, sigma=lr.SIGMA)
    want = np.stack([lr.blend(own[f], path[f], a[f]) for f in range(9)])
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    # a render with strengths 1 is the render with the goal as explicit targets, byte for byte
    frames, times = scene["frames"], scene["times"]
    t1 = p.strength_targets(times, ro, synth.D_TRUE, np.ones(3), targets=goals[zr.SCENE])
    got, n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, targets=t1, zoom=1.06)
    want, want_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, targets=goals[zr.SCENE], zoom=1.06)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(n, want_n)
    # frames that show a border even without smoothing: case A at zoom 1.0
    a, st = p.fit_strength(W, H, lens, lr.TIMES, synth.D_TRUE, zoom=lr.NOT_CLEAR_ZOOM["A"], steps=lr.STEPS, **_kw("A"))
    assert (a == 0).all() and (st == limit.LIMIT_NOT_CLEAR).all()
    # ... and frames whose goal is clear
    a, st = p.fit_strength(W, H, lens, lr.TIMES, synth.D_TRUE, zoom=1.3, steps=lr.STEPS, **_kw("A"))
    assert (a == 1).all() and (st == limit.LIMIT_CLEAR).all()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end(scene, fitted):
    """fit, envelope, targets; then the grayscale renderer"""
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    zoom = lr.CASES["A"]["zoom"]
    targets, strengths, status = p.limited_targets(W, H, lens, lr.TIMES, synth.D_TRUE, lr.WINDOW, zoom=zoom, steps=lr.STEPS, verify=True,
                                                   **_kw("A"))
    a = fitted["A"][0]
    print("fitted", a.tolist(), "smoothed", strengths.tolist())
    assert not status.any() and (strengths <= a).all() and (strengths < a).any() and (strengths >= a.min()).all()
    want = lr.smooth(lr.TIMES, a, lr.WINDOW)
    assert np.abs(strengths / want - 1).max() <= 1e-12                 # (tests/test_limit_cpu.py: an ulp per weight)
    np.testing.assert_array_equal(p.smooth_strengths(lr.TIMES, a, 0.0), a)
    np.testing.assert_array_equal(targets.view(np.uint64),
                                  p.strength_targets(lr.TIMES, lens[0], synth.D_TRUE, strengths, sigma=lr.SIGMA).view(np.uint64))
    counts = p.stabilize_coverage(W, H, lens, lr.TIMES, synth.D_TRUE, [zoom], targets=targets)
    assert (counts == 0).all(), counts.ravel()
    # the scene's three frames: all limited (strength below 1), so the unlimited goal shows fill and the limited path none
    assert (strengths[zr.SCENE] < 1).all()
    out, n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, targets=targets[zr.SCENE], zoom=zoom)
    assert (n == 0).all() and out.shape == (rr.N_FRAMES, H, W), n
    _, n_goal = p.stabilize_frames(frames, times, lens, synth.D_TRUE, sigma=lr.SIGMA, zoom=zoom)
    print("outside along the unlimited path", n_goal.tolist())
    assert (n_goal > 0).all(), n_goal


def test_end_to_end_nv12_with_the_chroma_plane_limited_too(scene, fitted):
    """INTEGRATION.md's recipe for 4:2:0 video: rssync_limit_fit tests the luma plane's border; the chroma plane is the
    image of a camera of its own (rssync_color.h: half the sizes, the chroma lens and output camera, a frame time
    ro * (oy / height) later), so the fit is run on it as well, against the same goals, and every frame takes the smaller
    of its two strengths.  Then neither plane of the NV12 render has a filled sample, where the unlimited goal fills both."""
    from rssync_amd import color, synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    zoom = lr.CASES["A"]["zoom"]
    goal = p.stabilize_path(lr.TIMES, lens[0], synth.D_TRUE, lr.SIGMA)
    luma = fitted["A"][0]
    lens_c, cam_c, dt = color.chroma_config(lens, W, H, W, H)
    chroma_kw = dict(out_camera=cam_c, camera=lr.CASES["A"]["camera"])
    chroma, status = p.fit_strength(W // 2, H // 2, lens_c, lr.TIMES + dt, synth.D_TRUE, zoom=zoom, steps=lr.STEPS, targets=goal, **chroma_kw)
    print("luma", luma.tolist(), "chroma", chroma.tolist())
    assert not status.any()
    assert (chroma < luma).any()                     # (the chroma border is another contour: here it is the tighter one somewhere)
    strengths = p.smooth_strengths(lr.TIMES, np.minimum(luma, chroma), lr.WINDOW)
    targets = p.strength_targets(lr.TIMES, lens[0], synth.D_TRUE, strengths, sigma=lr.SIGMA)
    # both planes' borders, by the coverage call
    assert (p.stabilize_coverage(W, H, lens, lr.TIMES, synth.D_TRUE, [zoom], targets=targets) == 0).all()
    assert (p.stabilize_coverage(W // 2, H // 2, lens_c, lr.TIMES + dt, synth.D_TRUE, [zoom], targets=targets, **chroma_kw) == 0).all()
    rng = np.random.default_rng(5)
    nv12 = (np.ascontiguousarray(frames), rng.integers(0, 256, size=(rr.N_FRAMES, H // 2, W // 2, 2), dtype=np.uint8))
    assert (strengths[zr.SCENE] < 1).all()
    _, n = p.stabilize_color(color.NV12, nv12, times, lens, synth.D_TRUE, targets=targets[zr.SCENE], zoom=zoom)
    _, n_goal = p.stabilize_color(color.NV12, nv12, times, lens, synth.D_TRUE, sigma=lr.SIGMA, zoom=zoom)
    print("NV12 outside (luma, chroma): limited", n.tolist(), "unlimited", n_goal.tolist())
    assert n.shape == (rr.N_FRAMES, 2) and (n == 0).all(), n
    assert (n_goal > 0).all(), n_goal


def test_verify_names_the_frames_that_are_not_clear(scene):
    from rssync_amd import limit, synth
    p, lens = scene["problem"], scene["lens"]
    with pytest.raises(limit.RsSyncError, match=r"frames \[0, 1, 2, 3, 4, 5, 6, 7, 8\] are not clear"):
        p.limited_targets(W, H, lens, lr.TIMES, synth.D_TRUE, lr.WINDOW, zoom=lr.NOT_CLEAR_ZOOM["A"], steps=lr.STEPS, verify=True, **_kw("A"))
    # one zoom per frame: the frames at zoom 1.0 are named, the others are clear
    with pytest.raises(limit.RsSyncError, match=r"frames \[0, 6\] are not clear"):
        p.limited_targets(W, H, lens, lr.TIMES, synth.D_TRUE, 0.0, zooms=MIXED_ZOOMS, steps=lr.STEPS, verify=True, **_kw("A"))


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene, fitted):
    from rssync_amd import limit, stabilize, synth
    p, lens = scene["problem"], scene["lens"]
    lib = limit.library()
    lib.rssync_set_panic_mode(1)
    PD = C.POINTER(C.c_double)
    L = np.ascontiguousarray(lens, np.float64)
    T9 = np.ascontiguousarray(lr.TIMES)
    zoom = lr.CASES["A"]["zoom"]
    prm = stabilize.params(sigma=lr.SIGMA, zoom=zoom)
    nan, inf = float("nan"), float("inf")

    def err():
        return lib.rssync_last_error().decode()

    def pd(a):
        return None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(PD)

    def with_value(a, i, v):
        b = np.array(a, np.float64)
        b[i] = v
        return b

    # the fit
    res, st = np.zeros(9), np.zeros(9, np.uint32)

    def fit(h=p._h, t=T9, lens_=L, delay=synth.D_TRUE, zooms=None, steps=10, a=res, prm_=prm, ow=W, targets=None):
        return lib.rssync_limit_fit(h, W, H, None if lens_ is None else lens_.ctypes.data, ow, H, pd(t), 9, delay, pd(targets), C.byref(prm_),
                                    pd(zooms), steps, None if a is None else a.ctypes.data_as(PD), st.ctypes.data_as(C.POINTER(C.c_uint32)))

    ones = np.ones(9)
    for match, kw in (("steps", dict(steps=-1)), ("steps", dict(steps=41)), ("zoom", dict(zooms=with_value(ones, 3, 0.0))),
                      ("zoom", dict(zooms=with_value(ones, 0, nan))), ("zoom", dict(zooms=with_value(ones, 8, -1.0))),
                      ("zoom", dict(zooms=with_value(ones, 8, inf))), ("zoom", dict(prm_=stabilize.params(sigma=lr.SIGMA, zoom=-1.0))),
                      ("no frame times", dict(t=None)), ("null output", dict(a=None)), ("no lens", dict(lens_=None)),
                      ("no problem", dict(h=None)), ("leaves the gyro data", dict(delay=9.0)), ("too small", dict(ow=1)),
                      ("sigma", dict(prm_=stabilize.params(sigma=-1.0))), ("camera", dict(prm_=stabilize.params(camera=5))),
                      ("zero or not finite", dict(targets=np.zeros((9, 4)))), ("zero or not finite", dict(targets=np.full((9, 4), nan)))):
        assert fit(**kw) != 0, kw
        assert match in err(), (match, err())
    assert fit(steps=40) == 0, err()
    assert fit(zooms=np.full(9, zoom), prm_=stabilize.params(sigma=lr.SIGMA, zoom=-7.0)) == 0, err()   # (params->zoom is not read then)
    np.testing.assert_array_equal(res, fitted["A"][0])
    # the envelope
    out = np.zeros(9)
    a9 = np.array(fitted["A"][0])

    def smooth(h=p._h, t=T9, a=a9, window=0.1, o=out):
        return lib.rssync_limit_smooth(h, pd(t), pd(a), 9, window, None if o is None else o.ctypes.data_as(PD))

    for match, kw in (("window", dict(window=-0.1)), ("window", dict(window=nan)), ("window", dict(window=inf)),
                      ("must not decrease", dict(t=with_value(T9, 4, T9[2]))), ("non-finite frame time", dict(t=with_value(T9, 4, nan))),
                      ("strength", dict(a=with_value(a9, 3, -0.01))), ("strength", dict(a=with_value(a9, 3, 1.01))),
                      ("strength", dict(a=with_value(a9, 0, nan))), ("strength", dict(a=with_value(a9, 0, inf))),
                      ("no frame times", dict(t=None)), ("no strengths", dict(a=None)), ("null output", dict(o=None)),
                      ("no problem", dict(h=None))):
        assert smooth(**kw) != 0, kw
        assert match in err(), (match, err())
    assert smooth() == 0, err()
    np.testing.assert_array_equal(out, p.smooth_strengths(lr.TIMES, a9, 0.1))
    same = np.array(a9)
    assert lib.rssync_limit_smooth(p._h, pd(T9), same.ctypes.data_as(PD), 9, 0.1, same.ctypes.data_as(PD)) == 0      # (in place)
    np.testing.assert_array_equal(same, out)
    # the targets
    q = np.zeros((9, 4))

    def targets(h=p._h, t=T9, a=a9, o=q, sigma=lr.SIGMA, delay=synth.D_TRUE, ro=float(L[0]), goals=None):
        return lib.rssync_limit_targets(h, pd(t), 9, ro, delay, pd(goals), sigma, pd(a), None if o is None else o.ctypes.data_as(PD))

    for match, kw in (("strength", dict(a=with_value(a9, 5, 1.5))), ("strength", dict(a=with_value(a9, 5, -1e-9))),
                      ("strength", dict(a=with_value(a9, 5, nan))), ("no frame times", dict(t=None)), ("no strengths", dict(a=None)),
                      ("null output", dict(o=None)), ("sigma", dict(sigma=-1.0)), ("sigma", dict(sigma=nan)), ("no problem", dict(h=None)),
                      ("leaves the gyro data", dict(delay=-2.0)), ("readout", dict(ro=-0.01)),
                      ("zero or not finite", dict(goals=np.zeros((9, 4))))):
        assert targets(**kw) != 0, kw
        assert match in err(), (match, err())
    assert targets() == 0, err()
    np.testing.assert_array_equal(q, p.strength_targets(lr.TIMES, L[0], synth.D_TRUE, a9, sigma=lr.SIGMA))
    with pytest.raises(ValueError):
        p.fit_strength(W, H, lens, lr.TIMES, synth.D_TRUE, zooms=[1.0, 1.0])
    with pytest.raises(limit.RsSyncError, match="steps"):
        p.fit_strength(W, H, lens, lr.TIMES, synth.D_TRUE, steps=99)
