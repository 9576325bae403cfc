"""The dynamic zoom for colour video on the device (include/rssync_colorzoom.h, csrc/kernels/colorzoom.hpp): the render
against rssync_color_stabilize / rssync_color16_stabilize of every frame alone at its zoom, byte for byte in every plane and
both counts; the fit against the header's procedure run through rssync_zoom_fit and rssync_stabilize_path, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

# luma (rows, cols): the smallest 4:2:0 frame, one under a 64 x 4 tile of chroma samples, an odd chroma size that is no
# multiple of the tile (165 x 99), the scene's
SCENE_SIZE = (rr.ROWS, rr.COLS)
MID = (330, 198)
SIZES = [(4, 4), (38, 30), MID, SCENE_SIZE]
OUT = (200, 320)        # rows, cols of the other output size
N = 3
ZOOMS = (1.04, 0.8, 1.09)
CAMERAS = [sr.LENS, sr.PINHOLE]
FILTERS = [0, 1]
W, H = rr.COLS, rr.ROWS

GRAY8, NV12, I420, RGBA32, GRAY16, P010, P016, I010 = 0, 1, 2, 3, 16, 17, 18, 19
FORMATS = [NV12, I420, RGBA32, GRAY16, P010, P016, I010]
NAMES = {GRAY8: "gray8", NV12: "nv12", I420: "i420", RGBA32: "rgba32", GRAY16: "gray16", P010: "p010", P016: "p016", I010: "i010"}
YUV = (NV12, I420, P010, P016, I010)
# explicit fills, in sample values of the format's depth
FILLS = {NV12: (7, 99, 200, 0), I420: (7, 99, 200, 0), RGBA32: (7, 99, 200, 31), GRAY16: (65000, 0, 0, 0), P010: (1000, 5, 700, 0),
         P016: (65000, 5, 40000, 0), I010: (1000, 5, 700, 0)}


CAM_IDS, FILTER_IDS = ["lens", "pinhole"], ["bilinear", "bicubic"]
SIZE_IDS = ["%dx%d" % s for s in SIZES]


@pytest.fixture(scope="module")
def scene(built):
    import rssync_amd
    s = dict(cr.scene())
    assert rr.N_FRAMES == N
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(s["gyro"].quats, s["gyro"].fs, s["gyro"].t0)
    s["problem"] = p
    np.testing.assert_array_equal(s["times"], zr.TIMES[zr.SCENE])
    return s


@pytest.fixture(scope="module")
def planes():
    """per luma size: the lens and N frames in every format -- the colour scene at its size (widened to 10 and 16 bits with
    the low bits filled in), noise of the full range elsewhere; P010's low six bits are zero, I010 holds values up to 1023
    (read-only)"""
    out = {}
    col = cr.scene()
    for rows, cols in SIZES:
        rng = np.random.default_rng(rows * 1000 + cols)
        if (rows, cols) == SCENE_SIZE:
            y, u, v = (np.array(col[k][:N]) for k in ("y", "u", "v"))
            rgba = np.stack([y, y[:, ::-1], y[:, :, ::-1], y[::-1]], axis=-1)
            y10, u10, v10 = ((a.astype(np.uint16) << 2) | (a & 3) for a in (y, u, v))
            y16, u16, v16 = (a.astype(np.uint16) * 257 for a in (y, u, v))
        else:
            def noise(top, chroma):
                shape = (N, rows // 2, cols // 2) if chroma else (N, rows, cols)
                return rng.integers(0, top + 1, size=shape, dtype=np.uint8 if top == 255 else np.uint16)
            y, u, v = noise(255, False), noise(255, True), noise(255, True)
            rgba = rng.integers(0, 256, size=(N, rows, cols, 4), dtype=np.uint8)
            y10, u10, v10 = noise(1023, False), noise(1023, True), noise(1023, True)
            y16, u16, v16 = noise(65535, False), noise(65535, True), noise(65535, True)
        assert y10.max() <= 1023 and y10.max() > 255 and y16.max() > 1023
        d = {"lens": rr.scaled_lens(rows, cols), GRAY8: y, NV12: (y, np.stack([u, v], axis=-1)), I420: (y, u, v), RGBA32: rgba, GRAY16: y16,
             P010: (y10 << 6, np.stack([u10, v10], axis=-1) << 6), P016: (y16, np.stack([u16, v16], axis=-1)), I010: (y10, u10, v10)}
        for a in d.values():
            for b in (a if isinstance(a, tuple) else (a,)):
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
        out[(rows, cols)] = d
    return out


def _tuple(frames):
    return frames if isinstance(frames, tuple) else (frames,)


def _outs(rows, cols):
    """out_size arguments (cols, rows): the input's size, and OUT for sizes of at least 38 x 30"""
    return [None] + ([(OUT[1], OUT[0])] if rows >= 38 else [])


def _alone(p, fmt, frames, times, lens, zooms, targets=None, **kw):
    """the defining call: every frame through stabilize_color on its own, at its own zoom -> (planes, counts (n, 2))"""
    from rssync_amd import synth
    outs, counts = [], []
    for k, z in enumerate(zooms):
        one = tuple(a[k:k + 1] for a in _tuple(frames))
        res, n = p.stabilize_color(fmt, one if len(one) > 1 else one[0], times[k:k + 1], lens, synth.D_TRUE, zoom=z,
                                   targets=None if targets is None else targets[k:k + 1], **kw)
        outs.append(_tuple(res))
        counts.append(n[0])
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0]))), np.stack(counts)


def _same(got, got_n, want, want_n, what=""):
    got = _tuple(got)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a, b, err_msg="%s plane %d" % (what, k))
    np.testing.assert_array_equal(got_n, want_n, err_msg=what)


def _targets(scene):
    """explicit targets: another smoothing's orientations, not of unit length (the library normalises them)"""
    from rssync_amd import synth
    return 2.5 * sr.path64(scene["gyro"], scene["times"], scene["lens"][0], synth.D_TRUE, 0.3)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_every_frame_alone_at_its_zoom_byte_for_byte(scene, planes, fmt, camera, filter, size):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[size]
    for out_size in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, filter=filter, fills=FILLS[fmt])
        want, want_n = _alone(p, fmt, d[fmt], times, d["lens"], ZOOMS, **kw)
        if size == SCENE_SIZE and out_size is None and fmt in YUV:
            # the guard: at zoom 0.8 both cameras fill samples in both planes, or the counts and fills are not tested
            print(NAMES[fmt], CAM_IDS[camera], "reference counts", want_n.tolist())
            assert (want_n[1] > 0).all(), want_n
        got, got_n = p.stabilize_color_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
        _same(got, got_n, want, want_n, "%s -> %s" % (size, out_size))
        if fmt not in YUV:
            assert (got_n[:, 1] == 0).all()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [MID, SCENE_SIZE], ids=["330x198", "scene"])
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
def test_chroma_left_and_default_fills(scene, planes, fmt, camera, filter, size):
    from rssync_amd import color, synth
    p, times, d = scene["problem"], scene["times"], planes[size]
    for out_size in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, filter=filter, chroma_site=color.CHROMA_LEFT, fill=9)
        want, want_n = _alone(p, fmt, d[fmt], times, d["lens"], ZOOMS, **kw)
        got, got_n = p.stabilize_color_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
        _same(got, got_n, want, want_n, "%s -> %s" % (size, out_size))
        centre, _ = p.stabilize_color_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **dict(kw, chroma_site=color.CHROMA_CENTER))
        assert (centre[1] != got[1]).any() and (centre[0] == got[0]).all()         # (the site moves the chroma plane alone)


# 3 ---------------------------------------------------------------------------------------------------------------------
def _padded(like, value, device):
    """a backing buffer filled with `value` around a view of the shape of `like` -> (backing, view, index of the view)"""
    n, rows, cols = like.shape[:3]
    back = np.full((n, rows + 3, cols + 5) + like.shape[3:], value, like.dtype)
    where = (slice(None), slice(2, 2 + rows), slice(3, 3 + cols))
    if device:
        back = torch.from_numpy(back).to("cuda:0")
    return back, back[where], where


@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
def test_memory_kinds_pitches_and_chunks_do_not_change_the_result(scene, planes, fmt, camera, filter):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[MID]
    rows, cols = MID
    frames = d[fmt]
    kw = dict(sigma=sr.SIGMA, camera=camera, filter=filter)
    want, want_n = _alone(p, fmt, frames, times, d["lens"], ZOOMS, **kw)
    # device tensors in and out
    dev = tuple(torch.from_numpy(np.array(a)).to("cuda:0") for a in frames)
    got, got_n = p.stabilize_color_zoomed(fmt, dev, times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in got)
    _same(got, got_n, want, want_n, "device")
    # pitched buffers with a guard pattern around every output plane, on the device and on the host
    guard = 0xab if fmt == NV12 else 0xabcd
    for device in (True, False):
        src = [_padded(a, 0, False) for a in frames]
        for (back, view, where), a in zip(src, frames):
            view[:] = a
        ins = tuple(torch.from_numpy(back).to("cuda:0")[where] if device else view for back, view, where in src)
        dst = [_padded(a, guard, device) for a in want]
        views = tuple(view for _, view, _ in dst)
        res, n = p.stabilize_color_zoomed(fmt, ins, times, d["lens"], synth.D_TRUE, ZOOMS, out=views, **kw)
        assert res is views
        _same(views, n, want, want_n, "pitched, device %s" % device)
        for back, _, where in dst:
            back = back.cpu().numpy() if device else back
            pad = np.ones(back.shape, bool)
            pad[where] = False
            assert (back[pad] == guard).all()
    # a budget of one and a half frames per slot: three chunks through both slots
    b = 1 if fmt == NV12 else 2
    per_frame = (rows + 1) * 36 + (rows // 2 + 1) * 36 + 2 * b * (rows * cols * 3 // 2)
    got, got_n = p.stabilize_color_zoomed_budget(fmt, frames, times, d["lens"], synth.D_TRUE, ZOOMS, 2 * 1.5 * per_frame, **kw)
    _same(got, got_n, want, want_n, "chunks")


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV12, I010], ids=["nv12", "i010"])
def test_equal_zooms_are_the_colour_front_with_that_zoom(scene, planes, fmt, camera, filter):
    """the case in which the cached ray maps and the rays computed in place must agree"""
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[SCENE_SIZE]
    for z, out_size in ((1.07, None), (0.93, (MID[1], MID[0]))):
        kw = dict(sigma=sr.SIGMA, camera=camera, filter=filter, out_size=out_size)
        want, want_n = p.stabilize_color(fmt, d[fmt], times, d["lens"], synth.D_TRUE, zoom=z, **kw)
        got, got_n = p.stabilize_color_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, [z] * N, **kw)
        _same(got, got_n, want, want_n, "zoom %g" % z)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
def test_a_frames_bytes_do_not_depend_on_its_neighbours(scene, planes, camera):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[SCENE_SIZE]
    kw = dict(sigma=sr.SIGMA, camera=camera, filter=1)
    fwd, n_fwd = p.stabilize_color_zoomed(NV12, d[NV12], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
    back = tuple(np.ascontiguousarray(a[::-1]) for a in d[NV12])
    rev, n_rev = p.stabilize_color_zoomed(NV12, back, times[::-1], d["lens"], synth.D_TRUE, ZOOMS[::-1], **kw)
    _same(tuple(a[::-1] for a in rev), n_rev[::-1], fwd, n_fwd)
    assert (fwd[0][0] != fwd[0][1]).any() and (fwd[1][0] != fwd[1][1]).any()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
def test_gray8_is_the_gray_dynamic_zoom(scene, planes, camera, filter):
    from rssync_amd import synth
    p, times = scene["problem"], scene["times"]
    for size in (MID, SCENE_SIZE):
        d = planes[size]
        for out_size in _outs(*size):
            kw = dict(sigma=sr.SIGMA, camera=camera, filter=filter, out_size=out_size, fill=77)
            want, want_n = p.stabilize_frames_zoomed(d[GRAY8], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
            got, got_n = p.stabilize_color_zoomed(GRAY8, d[GRAY8], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(got_n[:, 0], want_n)
            assert (got_n[:, 1] == 0).all()
            assert want_n[1] > 0 or size != SCENE_SIZE or out_size is not None       # (zoom 0.8 fills pixels with both cameras)


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV12, P016], ids=["nv12", "p016"])
def test_render_with_the_callers_targets_and_camera(scene, planes, fmt, camera):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[SCENE_SIZE]
    kw = dict(out_size=(320, 200), out_camera=(300.0, 310.0, 150.5, 99.0), iterations=2, camera=camera)
    targets = _targets(scene)
    want, want_n = _alone(p, fmt, d[fmt], times, d["lens"], ZOOMS, targets=targets, **kw)
    got, got_n = p.stabilize_color_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, targets=targets, **kw)
    _same(got, got_n, want, want_n)


# 8 ---------------------------------------------------------------------------------------------------------------------
def _fit_kw(case):
    """the keywords of a case of tests/zoom_reference.py for a 4:2:0 format.  Case B's output, 197 x 131, is odd in both
    directions, which no 4:2:0 format takes (test below): its camera, range and steps with the next even size, 198 x 132"""
    c = zr.CASES[case]
    out_size = c["out_size"]
    if out_size is not None:
        out_size = (out_size[0] + (out_size[0] & 1), out_size[1] + (out_size[1] & 1))
    return c, dict(sigma=zr.SIGMA, camera=c["camera"], out_size=out_size)


def _procedure(p, lens, case, site, targets):
    """the header's procedure through the existing calls -> (zL, sL, zC, sC)"""
    from rssync_amd import color, stabilize, synth
    c, kw = _fit_kw(case)
    ow, oh = (W, H) if kw["out_size"] is None else kw["out_size"]
    zl, sl = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, targets=targets, **kw)
    lens_c, cam_c, dt = color.chroma_config(lens, W, H, ow, oh, site)
    if targets is None:
        targets = stabilize.stabilize_path(p, zr.TIMES, lens[0], synth.D_TRUE, zr.SIGMA)        # at the LUMA frame times
    zc, sc = p.fit_zoom(W // 2, H // 2, lens_c, zr.TIMES + dt, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, targets=targets,
                        **dict(kw, out_size=(ow // 2, oh // 2), out_camera=cam_c))
    return zl, sl, zc, sc


@pytest.mark.parametrize("site", [cr.CENTER, cr.LEFT], ids=["center", "left"])
@pytest.mark.parametrize("own_targets", [False, True], ids=["path", "targets"])
@pytest.mark.parametrize("case", sorted(zr.CASES))
def test_fit_is_the_maximum_of_the_luma_and_the_chroma_fit_bit_for_bit(scene, case, own_targets, site):
    from rssync_amd import synth
    p, lens = scene["problem"], scene["lens"]
    targets = 0.5 * sr.path64(scene["gyro"], zr.TIMES, lens[0], synth.D_TRUE, 0.3) if own_targets else None
    c, kw = _fit_kw(case)
    zl, sl, zc, sc = _procedure(p, lens, case, site, targets)
    got, status = p.fit_zoom_color(NV12, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, targets=targets, chroma_site=site,
                                   **kw)
    print(case, "site", site, "targets", own_targets)
    print("  luma  ", zl.tolist(), sl.tolist())
    print("  chroma", zc.tolist(), sc.tolist())
    print("  chroma dominates frames", np.flatnonzero(zc > zl).tolist(), "luma", np.flatnonzero(zl > zc).tolist())
    assert got.dtype == np.float64 and status.dtype == np.uint32
    np.testing.assert_array_equal(got.view(np.uint64), np.maximum(zl, zc).view(np.uint64))
    np.testing.assert_array_equal(status, sl | sc)


def test_fit_refuses_an_odd_output_for_420_and_is_fit_zoom_without_a_sub_sampled_plane(scene):
    import rssync_amd
    from rssync_amd import synth
    p, lens = scene["problem"], scene["lens"]
    for case in sorted(zr.CASES):
        c = zr.CASES[case]
        kw = dict(sigma=zr.SIGMA, camera=c["camera"], out_size=c["out_size"])
        want, want_status = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, **kw)
        for fmt in (RGBA32, GRAY16, GRAY8):
            got, status = p.fit_zoom_color(fmt, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, **kw)
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
            np.testing.assert_array_equal(status, want_status)
        np.testing.assert_array_equal(want, np.array(zr.FITTED[case]))
    c = zr.CASES["B"]
    with pytest.raises(rssync_amd.RsSyncError, match="even"):
        p.fit_zoom_color(NV12, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], sigma=zr.SIGMA, camera=c["camera"], out_size=c["out_size"])


def test_frames_rendered_at_their_fitted_zooms_are_clear_in_every_plane(scene, planes):
    import rssync_amd
    from rssync_amd import synth
    p, times, lens, d = scene["problem"], scene["times"], scene["lens"], planes[SCENE_SIZE]
    c, kw = _fit_kw("A")
    fitted, status = p.fit_zoom_color(NV12, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, **kw)
    assert not status.any()
    _, n_at = p.stabilize_color_zoomed(NV12, d[NV12], times, lens, synth.D_TRUE, fitted[zr.SCENE], sigma=zr.SIGMA)
    print("fitted", fitted.tolist(), "outside at the fitted zooms", n_at.tolist())
    assert (n_at == 0).all(), n_at
    smoothed = p.dynamic_zoom_color(NV12, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], zr.WINDOW, steps=zr.STEPS, **kw)
    np.testing.assert_array_equal(smoothed, p.smooth_zooms(zr.TIMES, fitted, zr.WINDOW))
    assert (smoothed >= fitted).all() and (smoothed > fitted).any()
    _, n_smooth = p.stabilize_color_zoomed(NV12, d[NV12], times, lens, synth.D_TRUE, smoothed[zr.SCENE], sigma=zr.SIGMA)
    assert (n_smooth == 0).all(), n_smooth
    with pytest.raises(rssync_amd.RsSyncError, match="not clear"):
        p.dynamic_zoom_color(NV12, W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.02, zr.WINDOW, steps=zr.STEPS, **kw)


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene, planes):
    from rssync_amd import color, colorzoom, synth
    p, times, lens, d = scene["problem"], scene["times"], scene["lens"], planes[SCENE_SIZE]
    y, uv = (np.ascontiguousarray(a) for a in d[NV12])
    y10, uv10 = (np.ascontiguousarray(a) for a in d[P010])
    want, want_n = _alone(p, NV12, d[NV12], times, lens, ZOOMS, sigma=sr.SIGMA, camera=sr.LENS, filter=0, fills=FILLS[NV12])
    lib = colorzoom.library()
    lib.rssync_set_panic_mode(1)
    PD = C.POINTER(C.c_double)
    L, T, Z = np.ascontiguousarray(lens, np.float64), np.ascontiguousarray(times, np.float64), np.array(ZOOMS)
    out_y, out_uv = np.zeros_like(y), np.zeros_like(uv)
    out_y10, out_uv10 = np.zeros_like(y10), np.zeros_like(uv10)
    nan, inf = float("nan"), float("inf")

    def err():
        return lib.rssync_last_error().decode()

    def image(arrays, w, h, size=1):
        img = color.ColorImage()
        for k, a in enumerate(arrays):
            img.plane[k] = a if isinstance(a, int) or a is None else a.ctypes.data
            img.pitch[k], img.stride[k] = size * w, size * w * (h if k == 0 else h // 2)
        return img

    def prm_with(site=0, fill_set=1, fills=FILLS[NV12], **kw):
        q = color.ColorParams()
        q.stab = color.StabilizeParams(**dict(dict(sigma=sr.SIGMA), **kw))
        q.chroma_site, q.fill_set = site, fill_set
        for k in range(4):
            q.fill[k] = fills[k]
        return q

    def render(fmt=NV12, src=None, dst=None, w=W, h=H, ow=W, oh=H, prm=None, z=Z, edit=None):
        src = image((y, uv), w, h) if src is None else src
        dst = image((out_y, out_uv), ow, oh) if dst is None else dst
        if edit:
            edit(src, dst)
        prm = prm_with() if prm is None else prm
        counts = np.zeros((N, 2), np.uint64)
        rc = lib.rssync_colorzoom_stabilize(p._h, fmt, C.byref(src), N, w, h, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE, None, C.byref(prm),
                                            C.byref(dst), ow, oh, counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            None if z is None else np.ascontiguousarray(z, np.float64).ctypes.data_as(PD))
        return rc, counts

    def set_(which, field, k, value):
        def edit(src, dst):
            getattr(src if which == "in" else dst, field)[k] = value
        return edit

    def p010(**kw):
        return dict(dict(fmt=P010, src=image((y10, uv10), W, H, 2), dst=image((out_y10, out_uv10), W, H, 2), prm=prm_with(fills=FILLS[P010])),
                    **kw)

    for match, kw in (("no zooms", dict(z=None)), ("zoom", dict(z=[1.0, 0.0, 1.0])), ("zoom", dict(z=[1.0, -1.0, 1.0])),
                      ("zoom", dict(z=[1.0, 1.0, nan])), ("zoom", dict(z=[inf, 1.0, 1.0])),
                      ("is NULL", dict(edit=set_("in", "plane", 1, None))), ("is NULL", dict(edit=set_("out", "plane", 0, None))),
                      ("pitch", dict(edit=set_("in", "pitch", 0, W - 1))), ("pitch", dict(edit=set_("out", "pitch", 1, W - 1))),
                      ("even", dict(w=W - 1)), ("even", dict(oh=H - 1)), ("format", dict(fmt=4)), ("format", dict(fmt=20)),
                      ("format", dict(fmt=-1)), ("alignment", p010(edit=set_("in", "pitch", 0, 2 * W + 1))),
                      ("alignment", p010(edit=set_("out", "pitch", 1, 2 * W + 3))),
                      ("overlaps", dict(dst=image((out_y, y.ctypes.data + 8), W, H))), ("fill 1", dict(prm=prm_with(fills=(0, 256, 0, 0)))),
                      ("fill 0", p010(prm=prm_with(fills=(1024, 0, 0, 0)))), ("filter", dict(prm=prm_with(filter=2))),
                      ("chroma_site", dict(prm=prm_with(site=2)))):
        rc, _ = render(**kw)
        assert rc != 0, (match, kw)
        assert match in err(), (match, err())
    rc, _ = render(prm=prm_with(zoom=-7.0))                  # (params->stab.zoom is not read)
    assert rc == 0, err()
    np.testing.assert_array_equal(out_y, want[0])

    # the fit
    zs, st = np.zeros(9), np.zeros(9, np.uint32)
    T9 = np.ascontiguousarray(zr.TIMES)

    def fit(fmt=NV12, lo=1.0, hi=1.5, steps=zr.STEPS, prm=None, ow=W):
        prm = prm_with(fill_set=0, sigma=zr.SIGMA) if prm is None else prm
        return lib.rssync_colorzoom_fit(p._h, fmt, W, H, L.ctypes.data, ow, H, T9.ctypes.data_as(PD), 9, synth.D_TRUE, None, C.byref(prm), lo, hi,
                                        steps, zs.ctypes.data_as(PD), st.ctypes.data_as(C.POINTER(C.c_uint32)))

    for match, kw in (("below zoom_hi", dict(lo=1.5, hi=1.5)), ("below zoom_hi", dict(lo=1.5, hi=1.2)), ("steps", dict(steps=41)),
                      ("format", dict(fmt=4)), ("format", dict(fmt=20)), ("chroma_site", dict(prm=prm_with(site=2, fill_set=0))),
                      ("even", dict(ow=W - 1)), ("zoom_lo", dict(lo=0.0)), ("zoom_hi", dict(hi=inf))):
        assert fit(**kw) != 0, kw
        assert match in err(), (match, err())
    assert fit(prm=prm_with(fill_set=0, sigma=zr.SIGMA, zoom=-7.0)) == 0, err()
    again, _ = p.fit_zoom_color(NV12, W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.5, steps=zr.STEPS, sigma=zr.SIGMA)
    np.testing.assert_array_equal(zs, again)
    with pytest.raises(ValueError):
        p.stabilize_color_zoomed(NV12, d[NV12], times, lens, synth.D_TRUE, [1.0, 1.0])

    # ... and a good call gives case 1's bytes
    out_y[:], out_uv[:] = 0, 0
    rc, counts = render()
    assert rc == 0, err()
    np.testing.assert_array_equal(out_y, want[0])
    np.testing.assert_array_equal(out_uv, want[1])
    np.testing.assert_array_equal(counts, want_n)
    got, got_n = p.stabilize_color_zoomed(NV12, d[NV12], times, lens, synth.D_TRUE, ZOOMS, sigma=sr.SIGMA, fills=FILLS[NV12])
    _same(got, got_n, want, want_n)
