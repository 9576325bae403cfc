"""The dynamic zoom on the device (include/rssync_zoom.h, csrc/kernels/zoom.hpp): the fit against the same bisection run
on the host through rssync_stabilize_coverage, bit for bit, and against the numpy restatement (tests/zoom_reference.py);
the render against rssync_stabilize_frames of every frame alone, byte for byte; the envelope end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import rectify_reference as rr
import stabilize_reference as sr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

W, H = rr.COLS, rr.ROWS
SMALL = (37, 29)       # rows, cols: smaller than one 64 x 4 tile
ODD = (331, 197)       # no multiple of the tile
RENDER_ZOOMS = (1.04, 1.0, 1.09)


@pytest.fixture(scope="module")
def scene(built):
    import rssync_amd
    s = dict(rr.scene())
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(s["gyro"].quats, s["gyro"].fs, s["gyro"].t0)
    s["problem"] = p
    np.testing.assert_array_equal(s["times"], zr.TIMES[zr.SCENE])
    return s


def _kw(case, **more):
    """the keywords the device calls share with the reference's case"""
    c = zr.CASES[case]
    kw = dict(sigma=zr.SIGMA, camera=c["camera"])
    if c["out_size"] is not None:
        kw["out_size"] = c["out_size"]
    kw.update(more)
    return kw


def _host_fit(p, lens, lo, hi, steps, **kw):
    """the header's procedure for the nine frames at once, clear(f, z) read from the existing coverage call: at each step
    the nine current candidates go in as the sweep's zooms and the diagonal is read"""
    from rssync_amd import synth
    n = len(zr.TIMES)

    def clear(z):
        counts = p.stabilize_coverage(W, H, lens, zr.TIMES, synth.D_TRUE, z, **kw)
        return np.diagonal(counts) == 0

    clear_hi, clear_lo = clear(np.full(n, hi)), clear(np.full(n, lo))
    a, b = np.full(n, lo), np.full(n, hi)
    for _ in range(steps):
        mid = 0.5 * (a + b)
        ok = clear(mid)
        b = np.where(ok, mid, b)
        a = np.where(ok, a, mid)
    zooms = np.where(~clear_hi, hi, np.where(clear_lo, lo, b))
    return zooms, (~clear_hi).astype(np.uint32)


@pytest.fixture(scope="module")
def fitted(scene):
    """the device's fit of both cases (read-only)"""
    from rssync_amd import synth
    out = {}
    for name, c in zr.CASES.items():
        z, st = scene["problem"].fit_zoom(W, H, scene["lens"], zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, **_kw(name))
        z.setflags(write=False)
        st.setflags(write=False)
        out[name] = (z, st)
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------
def _targets():
    s = rr.scene()
    from rssync_amd import synth
    return 0.5 * sr.path64(s["gyro"], zr.TIMES, s["lens"][0], synth.D_TRUE, 0.3)


@pytest.mark.parametrize("case,steps,more", [("A", 10, {}), ("B", 10, {}), ("A", 10, {"targets": True}), ("A", 1, {}), ("A", 0, {}),
                                             ("A", 10, {"iterations": 2})],
                         ids=["A", "B", "A-targets", "A-one-step", "A-default-steps", "A-two-iterations"])
def test_fit_is_the_hosts_bisection_through_the_coverage_call_bit_for_bit(scene, case, steps, more):
    from rssync_amd import synth
    p, lens, c = scene["problem"], scene["lens"], zr.CASES[case]
    more = dict(more)
    if more.pop("targets", False):
        more["targets"] = _targets()
    kw = _kw(case, **more)
    got, status = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=steps, **kw)
    want, want_status = _host_fit(p, lens, c["lo"], c["hi"], steps if steps else 12, **kw)
    print(case, steps, more.keys(), got.tolist(), status.tolist())
    assert got.dtype == np.float64 and status.dtype == np.uint32
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    np.testing.assert_array_equal(status, want_status)
    assert not status.any() and (got > c["lo"]).all() and (got < c["hi"]).all()      # (these inputs make every frame bisect)
    if steps == 0:
        assert (np.abs(got - np.array(zr.FITTED[case])) < (c["hi"] - c["lo"]) / 1024).all()      # (two steps finer than the ten's)


def test_fit_of_more_frames_than_one_step_holds_tables_for(scene, fitted):
    """the nine times over and over, past the number of row tables one step of the pipeline keeps: every frame's result
    is its own, whichever step and workgroup it fell into; without the status array"""
    from rssync_amd import stabilize, synth, zoom
    p, lens, c = scene["problem"], scene["lens"], zr.CASES["B"]
    n = (64 << 20) // ((H + 1) * 36) + 10
    times = np.ascontiguousarray(np.resize(zr.TIMES, n))
    got, status = p.fit_zoom(W, H, lens, times, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, **_kw("B"))
    np.testing.assert_array_equal(got, np.resize(fitted["B"][0], n))
    assert not status.any()
    lib = zoom.library()
    L = np.ascontiguousarray(lens, np.float64)
    prm = stabilize.params(**{k: v for k, v in _kw("B").items() if k != "out_size"})
    ow, oh = c["out_size"]
    alone = np.zeros(9)
    assert lib.rssync_zoom_fit(p._h, W, H, L.ctypes.data, ow, oh, zr.TIMES.ctypes.data_as(C.POINTER(C.c_double)), 9, synth.D_TRUE, None,
                               C.byref(prm), c["lo"], c["hi"], zr.STEPS, alone.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    np.testing.assert_array_equal(alone, fitted["B"][0])


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(zr.CASES))
def test_fit_lies_between_the_references_brackets(scene, fitted, case):
    """a device map within the map tolerance of the float64 one can count a border pixel differently only within that
    tolerance of a frame edge: liberal <= device <= conservative.  On these inputs the brackets coincide."""
    c = zr.CASES[case]
    frames = zr.borders(case)
    tol = sr.device_tolerance(c["camera"])
    liberal, _ = zr.fit64(frames, c["lo"], c["hi"], mode=zr.LIBERAL, tol=tol)
    conservative, _ = zr.fit64(frames, c["lo"], c["hi"], mode=zr.CONSERVATIVE, tol=tol)
    got, status = fitted[case]
    print(case, got.tolist())
    assert (liberal <= got).all() and (got <= conservative).all() and not status.any()
    np.testing.assert_array_equal(got, np.array(zr.FITTED[case]))


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(scene):
    from rssync_amd import synth, zoom
    p, lens = scene["problem"], scene["lens"]
    z, st = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.02, steps=zr.STEPS, **_kw("A"))
    assert (z == 1.02).all() and (st == zoom.ZOOM_NOT_CLEAR).all()
    z, st = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, 1.2, 1.5, steps=zr.STEPS, **_kw("A"))
    assert (z == 1.2).all() and (st == zoom.ZOOM_CLEAR).all()
    z, st = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.06, steps=zr.STEPS, **_kw("A"))
    want_z, want_st = zr.fit64(zr.borders("A"), 1.0, 1.06)
    assert st.tolist() == want_st.tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 1]       # clear: k = 31, 35, 36, 37
    np.testing.assert_array_equal(z, want_z)
    with pytest.raises(zoom.RsSyncError, match="not clear"):
        p.dynamic_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.06, zr.WINDOW, steps=zr.STEPS, **_kw("A"))


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_the_fitted_zoom_is_the_edge(scene, fitted):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    z = fitted["A"][0][zr.SCENE]
    _, n_at = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, z, sigma=zr.SIGMA)
    assert (n_at == 0).all(), n_at
    below = z - 0.5 / 1024          # the bisection's last lo: exactly representable, and not clear
    assert ((below + 0.5 / 1024) == z).all()
    _, n_below = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, below, sigma=zr.SIGMA)
    print("outside at the fitted zoom", n_at.tolist(), "one step below", n_below.tolist())
    assert (n_below > 0).all(), n_below


# 5 ---------------------------------------------------------------------------------------------------------------------
def _alone(p, scene, zooms, **kw):
    """every frame through rssync_stabilize_frames on its own, at its own zoom"""
    from rssync_amd import synth
    outs, counts = [], []
    for k, z in enumerate(zooms):
        o, n = p.stabilize_frames(scene["frames"][k:k + 1], scene["times"][k:k + 1], scene["lens"], synth.D_TRUE, zoom=z, **kw)
        outs.append(o[0])
        counts.append(n[0])
    return np.stack(outs), np.array(counts, np.uint64)


@pytest.mark.parametrize("out", [(H, W), SMALL, ODD], ids=["same", "small", "odd"])
@pytest.mark.parametrize("filter", [0, 1], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("camera", [sr.LENS, sr.PINHOLE], ids=["lens", "pinhole"])
def test_render_is_every_frame_alone_at_its_zoom_byte_for_byte(scene, camera, filter, out):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    orows, ocols = out
    kw = dict(sigma=zr.SIGMA, camera=camera, filter=filter, fill=77, out_size=(ocols, orows))
    want, want_n = _alone(p, scene, RENDER_ZOOMS, **kw)
    assert want_n.sum() > 0 or camera == sr.PINHOLE         # (the lens's camera at zoom 1.0 sees past the frame)
    # numpy frames
    got, n = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, RENDER_ZOOMS, **kw)
    assert isinstance(got, np.ndarray) and got.shape == (rr.N_FRAMES, orows, ocols)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(n, want_n)
    # device-resident tensors
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")
    got, n = p.stabilize_frames_zoomed(dev, times, lens, synth.D_TRUE, RENDER_ZOOMS, **kw)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(n, want_n)
    # pitched device buffers, a guard pattern between the rows of the result
    wide = np.zeros((rr.N_FRAMES, H + 2, W + 61), np.uint8)
    wide[:, 1:1 + H, 13:13 + W] = frames
    dwide = torch.from_numpy(wide).to("cuda:0")
    dout = torch.full((rr.N_FRAMES, orows + 3, ocols + 19), 201, dtype=torch.uint8, device="cuda:0")
    view = dout[:, 2:2 + orows, 3:3 + ocols]
    res, n = p.stabilize_frames_zoomed(dwide[:, 1:1 + H, 13:13 + W], times, lens, synth.D_TRUE, RENDER_ZOOMS, out=view, **kw)
    assert res is view
    back = dout.cpu().numpy()
    np.testing.assert_array_equal(back[:, 2:2 + orows, 3:3 + ocols], want)
    np.testing.assert_array_equal(n, want_n)
    guard = np.ones(back.shape, bool)
    guard[:, 2:2 + orows, 3:3 + ocols] = False
    assert (back[guard] == 201).all()
    # pitched host buffers, the same way
    hout = np.full((rr.N_FRAMES, orows + 1, ocols + 5), 9, np.uint8)
    p.stabilize_frames_zoomed(wide[:, 1:1 + H, 13:13 + W], times, lens, synth.D_TRUE, RENDER_ZOOMS, out=hout[:, :orows, 2:2 + ocols], **kw)
    np.testing.assert_array_equal(hout[:, :orows, 2:2 + ocols], want)
    assert (hout[:, orows:] == 9).all() and (hout[:, :, :2] == 9).all() and (hout[:, :, 2 + ocols:] == 9).all()
    # a budget of one and a half frames per slot: three chunks through both slots
    per_frame = (H + 1) * 36 + H * W + orows * ocols
    got, n = p.stabilize_frames_zoomed_budget(frames, times, lens, synth.D_TRUE, RENDER_ZOOMS, 2 * 1.5 * per_frame, out_size=(ocols, orows),
                                              sigma=zr.SIGMA, camera=camera, filter=filter, fill=77)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(n, want_n)


def test_render_with_the_callers_targets_and_camera(scene):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    kw = dict(targets=_targets()[zr.SCENE], out_size=(320, 200), out_camera=(300.0, 310.0, 150.5, 99.0), iterations=2)
    for camera in (sr.LENS, sr.PINHOLE):
        got, n = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, RENDER_ZOOMS, camera=camera, **kw)
        for k, z in enumerate(RENDER_ZOOMS):
            one = dict(kw, targets=kw["targets"][k:k + 1])
            want, want_n = p.stabilize_frames(frames[k:k + 1], times[k:k + 1], lens, synth.D_TRUE, zoom=z, camera=camera, **one)
            np.testing.assert_array_equal(got[k], want[0])
            assert n[k] == want_n[0]


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", [sr.LENS, sr.PINHOLE], ids=["lens", "pinhole"])
def test_a_frames_bytes_do_not_depend_on_its_neighbours(scene, camera):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    kw = dict(sigma=zr.SIGMA, camera=camera, filter=1)
    fwd, n_fwd = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, RENDER_ZOOMS, **kw)
    rev, n_rev = p.stabilize_frames_zoomed(np.ascontiguousarray(frames[::-1]), times[::-1], lens, synth.D_TRUE, RENDER_ZOOMS[::-1], **kw)
    np.testing.assert_array_equal(rev[::-1], fwd)
    np.testing.assert_array_equal(n_rev[::-1], n_fwd)
    assert (fwd[0] != fwd[1]).any()


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", [0, 1], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("camera", [sr.LENS, sr.PINHOLE], ids=["lens", "pinhole"])
def test_equal_zooms_are_the_stabiliser_with_that_zoom(scene, camera, filter):
    """the case in which the cached ray map and the ray computed in place must agree"""
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    for z, out_size in ((1.07, None), (0.93, (ODD[1], ODD[0]))):
        kw = dict(sigma=zr.SIGMA, camera=camera, filter=filter, out_size=out_size)
        want, want_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, zoom=z, **kw)
        got, n = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, [z] * rr.N_FRAMES, **kw)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(n, want_n)


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end(scene, fitted):
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    c = zr.CASES["A"]
    smoothed = p.dynamic_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], zr.WINDOW, steps=zr.STEPS, **_kw("A"))
    z = fitted["A"][0]
    print("fitted", z.tolist(), "smoothed", smoothed.tolist())
    assert (smoothed >= z).all() and (smoothed > z).any() and (smoothed <= z.max()).all()
    want = zr.smooth(zr.TIMES, z, zr.WINDOW)
    assert np.abs(smoothed / want - 1).max() <= 1e-12                  # (tests/test_zoom_cpu.py: an ulp per weight)
    np.testing.assert_array_equal(p.smooth_zooms(zr.TIMES, z, 0.0), z)
    # a zoom at or above a frame's fitted one stays clear: clear is monotone over the range (tests/test_zoom_cpu.py)
    out, n = p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, smoothed[zr.SCENE], sigma=zr.SIGMA)
    assert (n == 0).all() and out.shape == (rr.N_FRAMES, H, W)


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene, fitted):
    from rssync_amd import stabilize, synth, zoom
    p, frames, times, lens = scene["problem"], np.ascontiguousarray(scene["frames"]), scene["times"], scene["lens"]
    lib = zoom.library()
    lib.rssync_set_panic_mode(1)
    PD = C.POINTER(C.c_double)
    L = np.ascontiguousarray(lens, np.float64)
    T9 = np.ascontiguousarray(zr.TIMES)
    T3 = np.ascontiguousarray(times, np.float64)
    N = rr.N_FRAMES
    prm = stabilize.params(sigma=zr.SIGMA)
    nan, inf = float("nan"), float("inf")

    def err():
        return lib.rssync_last_error().decode()

    def pd(a):
        return None if a is None else a.ctypes.data_as(PD)

    # the fit
    zs, st = np.zeros(9), np.zeros(9, np.uint32)

    def fit(h=p._h, t=T9, lens_=L, delay=synth.D_TRUE, lo=1.0, hi=1.5, steps=10, z=zs, prm_=prm, ow=W):
        return lib.rssync_zoom_fit(h, W, H, None if lens_ is None else lens_.ctypes.data, ow, H, pd(t), 9, delay, None, C.byref(prm_), lo, hi,
                                   steps, pd(z), st.ctypes.data_as(C.POINTER(C.c_uint32)))

    for match, kw in (("below zoom_hi", dict(lo=1.5, hi=1.5)), ("below zoom_hi", dict(lo=1.5, hi=1.2)), ("zoom_lo", dict(lo=0.0)),
                      ("zoom_lo", dict(lo=-1.0)), ("zoom_lo", dict(lo=nan)), ("zoom_lo", dict(lo=-inf)), ("zoom_hi", dict(hi=inf)),
                      ("zoom_hi", dict(hi=nan)), ("zoom_hi", dict(hi=-2.0)), ("steps", dict(steps=-1)), ("steps", dict(steps=41)),
                      ("no frame times", dict(t=None)), ("null output", dict(z=None)), ("no lens", dict(lens_=None)),
                      ("no problem", dict(h=None)), ("leaves the gyro data", dict(delay=9.0)), ("too small", dict(ow=1)),
                      ("sigma", dict(prm_=stabilize.params(sigma=-1.0))), ("camera", dict(prm_=stabilize.params(camera=5)))):
        assert fit(**kw) != 0, kw
        assert match in err(), (match, err())
    assert fit(steps=40) == 0, err()
    assert fit(prm_=stabilize.params(sigma=zr.SIGMA, zoom=-7.0)) == 0, err()        # (params->zoom is not read)
    np.testing.assert_array_equal(zs, fitted["A"][0])
    # the envelope
    out = np.zeros(9)

    def smooth(h=p._h, t=T9, z=fitted["A"][0], window=0.1, o=out):
        return lib.rssync_zoom_smooth(h, pd(t), pd(np.ascontiguousarray(z) if z is not None else None), 9, window, pd(o))

    def with_value(a, i, v):
        b = np.array(a, np.float64)
        b[i] = v
        return b

    for match, kw in (("window", dict(window=-0.1)), ("window", dict(window=nan)), ("window", dict(window=inf)),
                      ("must not decrease", dict(t=with_value(T9, 4, T9[2]))), ("non-finite frame time", dict(t=with_value(T9, 4, nan))),
                      ("zoom", dict(z=with_value(fitted["A"][0], 3, 0.0))), ("zoom", dict(z=with_value(fitted["A"][0], 3, nan))),
                      ("zoom", dict(z=with_value(fitted["A"][0], 0, -1.0))), ("no frame times", dict(t=None)), ("no zooms", dict(z=None)),
                      ("null output", dict(o=None)), ("no problem", dict(h=None))):
        assert smooth(**kw) != 0, kw
        assert match in err(), (match, err())
    assert smooth() == 0, err()
    np.testing.assert_array_equal(out, p.smooth_zooms(zr.TIMES, fitted["A"][0], 0.1))
    same = np.array(fitted["A"][0])
    assert lib.rssync_zoom_smooth(p._h, pd(T9), pd(same), 9, 0.1, pd(same)) == 0       # (in place)
    np.testing.assert_array_equal(same, out)
    # the render: its own errors and the stabiliser's
    res = np.zeros_like(frames)
    Z3 = np.array(RENDER_ZOOMS)

    def render(h=p._h, f=frames.ctypes.data, t=T3, delay=synth.D_TRUE, z=Z3, o=None, pitch=W, opitch=W, prm_=prm, lens_=L):
        o = res.ctypes.data if o is None else o
        return lib.rssync_zoom_stabilize(h, f, N, W, H, pitch, W * H, pd(t), None if lens_ is None else lens_.ctypes.data, delay, None,
                                         C.byref(prm_), o if o else None, W, H, opitch, W * H, None, pd(z))

    for match, kw in (("no zooms", dict(z=None)), ("zoom", dict(z=np.array([1.0, 0.0, 1.0]))), ("zoom", dict(z=np.array([1.0, 1.0, nan]))),
                      ("zoom", dict(z=np.array([inf, 1.0, 1.0]))), ("zoom", dict(z=np.array([1.0, -1.0, 1.0]))), ("no frames", dict(f=None)),
                      ("null output", dict(o=0)), ("no frame times", dict(t=None)), ("no lens", dict(lens_=None)), ("pitch", dict(pitch=W - 1)),
                      ("out_pitch", dict(opitch=W - 1)), ("leaves the gyro data", dict(delay=-2.0)),
                      ("overlaps", dict(o=frames.ctypes.data + W * H)), ("fill", dict(prm_=stabilize.params(fill=256))),
                      ("filter", dict(prm_=stabilize.params(filter=2))), ("iterations", dict(prm_=stabilize.params(iterations=9)))):
        assert render(**kw) != 0, kw
        assert match in err(), (match, err())
    assert render() == 0, err()
    want, _ = _alone(p, scene, RENDER_ZOOMS, sigma=zr.SIGMA)
    np.testing.assert_array_equal(res, want)
    with pytest.raises(ValueError):
        p.stabilize_frames_zoomed(frames, times, lens, synth.D_TRUE, [1.0, 1.0])
    with pytest.raises(zoom.RsSyncError, match="zoom"):
        p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, 1.5, 1.0)
