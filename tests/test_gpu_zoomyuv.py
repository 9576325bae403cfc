"""The dynamic zoom for 4:2:2 and 4:4:4 video on the device (include/rssync_zoomyuv.h, csrc/kernels/zoomyuv.hpp): the render
against rssync_yuv_stabilize of every frame alone at its zoom, byte for byte in every plane and both counts; the fit against
the header's procedure run through rssync_zoom_fit and rssync_stabilize_path, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import rectify_reference as rr
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
import yuv_reference as yr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

# luma (rows, cols), tests/test_gpu_yuv.py's: the smallest 4:2:2 frame with an odd height; 65 chroma columns and 5 rows, one
# past a 64 x 4 tile each way; two sizes that are no multiple of the tile; the scene's.  4:4:4 adds a frame odd both ways.
SCENE_SIZE = (rr.ROWS, rr.COLS)
MID = (199, 330)
SIZES = [(3, 4), (5, 130), (31, 38), MID, SCENE_SIZE]
SIZES444 = SIZES + [(3, 5)]
OUT = (131, 198)        # rows, cols of the other output size
N = 3
ZOOMS = (1.04, 0.8, 1.09)
CAMERAS = [sr.LENS, sr.PINHOLE]
FILTERS = [0, 1]
W, H = rr.COLS, rr.ROWS
FIT_STEPS = 16          # at 10 or 12 steps the two planes' fits differ by at most a step: a test of the maximum shows nothing

I422, NV16, I444, I210, P210, P216, I410 = 32, 33, 34, 48, 49, 50, 51
FORMATS = [I422, NV16, I444, I210, P210, P216, I410]
NAMES = {I422: "i422", NV16: "nv16", I444: "i444", I210: "i210", P210: "p210", P216: "p216", I410: "i410"}
F444 = (I444, I410)
DEPTH = {I422: 8, NV16: 8, I444: 8, I210: 10, P210: 10, P216: 16, I410: 10}
# explicit fills, in sample values of the format's depth
FILLS = {8: (7, 99, 200, 0), 10: (1000, 5, 700, 0), 16: (65000, 5, 40000, 0)}

CAM_IDS, FILTER_IDS = ["lens", "pinhole"], ["bilinear", "bicubic"]
# every format at every size it takes: the odd width is 4:4:4's alone
FORMAT_SIZES = [(f, s) for f in FORMATS for s in (SIZES444 if f in F444 else SIZES)]
FORMAT_SIZE_IDS = ["%s-%dx%d" % (NAMES[f], s[0], s[1]) for f, s in FORMAT_SIZES]


def _problem(gyro):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def scene(built):
    s = dict(rr.scene())
    assert rr.N_FRAMES == N
    s["problem"] = _problem(s["gyro"])
    np.testing.assert_array_equal(s["times"], zr.TIMES[zr.SCENE])
    return s


def _layouts(y, u, v, u4, v4, shift):
    """the planes as (I422's, NV16's, I444's) frames; shift: the container's (P210: 6)"""
    return (y, u, v), (y << shift, np.stack([u, v], axis=-1) << shift), (y, u4, v4)


@pytest.fixture(scope="module")
def planes():
    """per luma size: the lens and N frames in every format -- the 4:2:2 scene at its size (widened to 10 and 16 bits with
    the low bits filled in; its 4:4:4 chroma planes are noise), noise of the full range elsewhere; P210's low six bits are
    zero, I210 and I410 hold values up to 1023 (read-only)"""
    out = {}
    col = yr.scene()
    for rows, cols in SIZES444:
        rng = np.random.default_rng(rows * 1000 + cols)

        def noise(top, half):
            return rng.integers(0, top + 1, size=(N, rows, cols // 2 if half else cols), dtype=np.uint8 if top == 255 else np.uint16)
        u4, v4 = noise(255, False), noise(255, False)
        if (rows, cols) == SCENE_SIZE:
            y, u, v = (np.array(col[k][:N]) for k in ("y", "u", "v"))
            y10, u10, v10 = ((a.astype(np.uint16) << 2) | (a & 3) for a in (y, u, v))
            y16, u16, v16 = (a.astype(np.uint16) * 257 for a in (y, u, v))
        else:
            y, u, v = noise(255, False), noise(255, True), noise(255, True)
            y10, u10, v10 = noise(1023, False), noise(1023, True), noise(1023, True)
            y16, u16, v16 = noise(65535, False), noise(65535, True), noise(65535, True)
        u410, v410 = noise(1023, False), noise(1023, False)
        assert y10.max() <= 1023 and y10.max() > 255 and y16.max() > 1023 and u410.max() > 255
        d = {"lens": rr.scaled_lens(rows, cols)}
        d[I422], d[NV16], d[I444] = _layouts(y, u, v, u4, v4, 0)
        d[I210], _, d[I410] = _layouts(y10, u10, v10, u410, v410, 0)
        _, d[P210], _ = _layouts(y10, u10, v10, u410, v410, 6)
        _, d[P216], _ = _layouts(y16, u16, v16, None, None, 0)
        assert (d[P210][0] & 63).max() == 0 and (d[P210][1] & 63).max() == 0 and d[P210][0].max() > 1023
        for a in d.values():
            for b in a:
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
        out[(rows, cols)] = d
    return out


def _outs(rows, cols):
    """out_size arguments (cols, rows): the input's size, and OUT for sizes of at least 31 rows"""
    return [None] + ([(OUT[1], OUT[0])] if rows >= 31 else [])


def _alone(p, fmt, frames, times, lens, zooms, targets=None, **kw):
    """the defining call: every frame through stabilize_yuv on its own, at its own zoom -> (planes, counts (n, 2))"""
    from rssync_amd import synth
    outs, counts = [], []
    for k, z in enumerate(zooms):
        one = tuple(a[k:k + 1] for a in frames)
        res, n = p.stabilize_yuv(fmt, one, times[k:k + 1], lens, synth.D_TRUE, zoom=z, targets=None if targets is None else targets[k:k + 1],
                                 **kw)
        outs.append(res)
        counts.append(n[0])
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0]))), np.stack(counts)


def _same(got, got_n, want, want_n, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        if a.dtype == np.int16:
            a = a.view(np.uint16)
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a, b, err_msg="%s plane %d" % (what, k))
    np.testing.assert_array_equal(got_n, want_n, err_msg=what)


def _targets(scene):
    """explicit targets: another smoothing's orientations, not of unit length (the library normalises them)"""
    from rssync_amd import synth
    return 2.5 * sr.path64(scene["gyro"], scene["times"], scene["lens"][0], synth.D_TRUE, 0.3)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt,size", FORMAT_SIZES, ids=FORMAT_SIZE_IDS)
def test_every_frame_alone_at_its_zoom_byte_for_byte(scene, planes, fmt, size, camera, filter):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[size]
    for out_size in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, filter=filter, fills=FILLS[DEPTH[fmt]])
        want, want_n = _alone(p, fmt, d[fmt], times, d["lens"], ZOOMS, **kw)
        if size == SCENE_SIZE and out_size is None:
            # the guard: at zoom 0.8 both cameras fill samples in both planes, or the counts and fills are not tested
            print(NAMES[fmt], CAM_IDS[camera], "reference counts", want_n.tolist())
            assert (want_n[1] > 0).all(), want_n
        got, got_n = p.stabilize_yuv_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
        _same(got, got_n, want, want_n, "%s -> %s" % (size, out_size))
        if fmt in F444:
            np.testing.assert_array_equal(got_n[:, 1], got_n[:, 0])


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [MID, SCENE_SIZE], ids=["199x330", "scene"])
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
def test_chroma_left_and_default_fills(scene, planes, fmt, camera, filter, size):
    from rssync_amd import synth, yuv
    p, times, d = scene["problem"], scene["times"], planes[size]
    for out_size in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, filter=filter, chroma_site=yuv.CHROMA_LEFT, fill=9)
        want, want_n = _alone(p, fmt, d[fmt], times, d["lens"], ZOOMS, **kw)
        got, got_n = p.stabilize_yuv_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
        _same(got, got_n, want, want_n, "%s -> %s" % (size, out_size))
        centre, _ = p.stabilize_yuv_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **dict(kw, chroma_site=yuv.CHROMA_CENTER))
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
@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
def test_memory_kinds_pitches_and_chunks_do_not_change_the_result(scene, planes, fmt, camera, filter):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[MID]
    rows, cols = MID
    frames = d[fmt]
    kw = dict(sigma=sr.SIGMA, camera=camera, filter=filter)
    want, want_n = _alone(p, fmt, frames, times, d["lens"], ZOOMS, **kw)
    # device tensors in and out
    dev = tuple(torch.from_numpy(np.array(a)).to("cuda:0") for a in frames)
    got, got_n = p.stabilize_yuv_zoomed(fmt, dev, times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in got)
    _same(got, got_n, want, want_n, "device")
    # pitched buffers with a guard pattern around every output plane, on the device and on the host
    guard = 0xab if fmt == NV16 else 0xabcd
    for device in (True, False):
        src = [_padded(a, 0, False) for a in frames]
        for (back, view, where), a in zip(src, frames):
            view[:] = a
        ins = tuple(torch.from_numpy(back).to("cuda:0")[where] if device else view for back, view, where in src)
        dst = [_padded(a, guard, device) for a in want]
        views = tuple(view for _, view, _ in dst)
        res, n = p.stabilize_yuv_zoomed(fmt, ins, times, d["lens"], synth.D_TRUE, ZOOMS, out=views, **kw)
        assert res is views
        _same(views, n, want, want_n, "pitched, device %s" % device)
        for back, _, where in dst:
            back = back.cpu().numpy() if device else back
            pad = np.ones(back.shape, bool)
            pad[where] = False
            assert (back[pad] == guard).all()
    # a budget of one and a half frames per slot: three chunks of one frame through both slots, each with a zoom of its
    # own (a kernel that read the cameras from the call's first frame would render frames 1 and 2 at frame 0's zoom)
    b = 1 if fmt == NV16 else 2
    per_frame = (rows + 1) * 36 + 2 * b * (rows * cols * 2)         # (one row table per frame; Y and UV, in and out)
    got, got_n = p.stabilize_yuv_zoomed_budget(fmt, frames, times, d["lens"], synth.D_TRUE, ZOOMS, 2 * 1.5 * per_frame, **kw)
    assert len(set(ZOOMS)) == 3
    _same(got, got_n, want, want_n, "chunks")


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV16, I410], ids=["nv16", "i410"])
def test_equal_zooms_are_stabilize_yuv_with_that_zoom(scene, planes, fmt, camera, filter):
    """the case in which the cached ray maps and the rays computed in place must agree"""
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[SCENE_SIZE]
    for z, out_size in ((1.07, None), (0.93, (OUT[1], OUT[0]))):
        kw = dict(sigma=sr.SIGMA, camera=camera, filter=filter, out_size=out_size)
        want, want_n = p.stabilize_yuv(fmt, d[fmt], times, d["lens"], synth.D_TRUE, zoom=z, **kw)
        got, got_n = p.stabilize_yuv_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, [z] * N, **kw)
        _same(got, got_n, want, want_n, "zoom %g" % z)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV16, I444], ids=["nv16", "i444"])
def test_a_frames_bytes_do_not_depend_on_its_neighbours(scene, planes, fmt, camera):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[SCENE_SIZE]
    kw = dict(sigma=sr.SIGMA, camera=camera, filter=1)
    fwd, n_fwd = p.stabilize_yuv_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, **kw)
    pick = [2, 0]
    some = tuple(np.ascontiguousarray(a[pick]) for a in d[fmt])
    got, got_n = p.stabilize_yuv_zoomed(fmt, some, times[pick], d["lens"], synth.D_TRUE, [ZOOMS[k] for k in pick], **kw)
    _same(got, got_n, tuple(a[pick] for a in fwd), n_fwd[pick])
    assert (fwd[0][0] != fwd[0][2]).any() and (fwd[1][0] != fwd[1][2]).any()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("fmt", [NV16, P216], ids=["nv16", "p216"])
def test_render_with_the_callers_targets_and_camera(scene, planes, fmt, camera):
    from rssync_amd import synth
    p, times, d = scene["problem"], scene["times"], planes[SCENE_SIZE]
    kw = dict(out_size=(320, 200), out_camera=(300.0, 310.0, 150.5, 99.0), iterations=2, camera=camera)
    targets = _targets(scene)
    want, want_n = _alone(p, fmt, d[fmt], times, d["lens"], ZOOMS, targets=targets, **kw)
    got, got_n = p.stabilize_yuv_zoomed(fmt, d[fmt], times, d["lens"], synth.D_TRUE, ZOOMS, targets=targets, **kw)
    _same(got, got_n, want, want_n)


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problems(built):
    """one problem per motion of tests/render_cases.py's per-frame cases"""
    return {m: _problem(wc.gyro(m)) for m in sorted({motion for _, motion, _ in rc.PERCAM_CASES})}


@pytest.fixture(scope="module")
def small():
    """noise at tests/render_cases.py's size, 94 x 170: NV16's and I444's frames (read-only)"""
    rng = np.random.default_rng([31, rc.ROWS, rc.COLS])
    y, u4, v4 = (rng.integers(0, 256, (rc.N_FRAMES, rc.ROWS, rc.COLS), dtype=np.uint8) for _ in range(3))
    uv = rng.integers(0, 256, (rc.N_FRAMES, rc.ROWS, rc.COLS // 2, 2), dtype=np.uint8)
    for a in (y, u4, v4, uv):
        a.setflags(write=False)
    return {NV16: (y, uv), I444: (y, u4, v4)}


@pytest.mark.parametrize("camera", CAMERAS, ids=CAM_IDS)
@pytest.mark.parametrize("name,motion,zoom", rc.PERCAM_CASES)
def test_lenses_that_leave_pixels_without_a_ray(problems, small, name, motion, zoom, camera):
    """with the LENS camera 'half' and 'nonmono' have output samples no ray belongs to, in both planes: computed in place
    here, read from the cached ray map by the frames alone"""
    from rssync_amd import synth
    assert {"half", "nonmono"} <= {c[0] for c in rc.PERCAM_CASES} and (rc.ROWS, rc.COLS) == (94, 170)
    p, L, times = problems[motion], rc.lens(name), wc.frame_times()
    site = yr.LEFT if name in ("half", "strong") else yr.CENTER
    filled = 0
    for fmt in (NV16, I444):
        for out_size in rc.out_sizes():
            kw = dict(sigma=rc.SIGMA, camera=camera, filter=0, chroma_site=site, fills=FILLS[8], out_size=out_size)
            want, want_n = _alone(p, fmt, small[fmt], times, L, rc.PERCAM_ZOOMS, **kw)
            got, got_n = p.stabilize_yuv_zoomed(fmt, small[fmt], times, L, synth.D_TRUE, rc.PERCAM_ZOOMS, **kw)
            _same(got, got_n, want, want_n, "%s %s camera %d format %d -> %s" % (name, motion, camera, fmt, out_size))
            filled += int(got_n.sum())
            if camera == sr.LENS and out_size is None and name in ("half", "nonmono"):
                # the samples beyond the zoomed camera's model range at zoom 1 (frame 0) are among the filled ones
                z0 = rc.PERCAM_ZOOMS[0]
                for pl in ((0, 1) if fmt == NV16 else (0,)):
                    cam, shape = wc.stab_camera_lens(L, rc.ROWS, rc.COLS, z0), (rc.ROWS, rc.COLS)
                    if pl == 1:
                        cam = (L[0],) + tuple(yr.chroma_camera422(L, rc.ROWS, rc.COLS, rc.ROWS, rc.COLS, site, z0)) + tuple(L[5:])
                        shape = (rc.ROWS, rc.COLS // 2)
                    outr = wc.range_masks(cam, wc.grid(*shape))[1]
                    assert outr.sum() >= 9 and int(want_n[0, pl]) >= outr.sum(), (name, pl, int(outr.sum()), want_n.tolist())
    print("%s %s camera %d: %d samples filled in all" % (name, motion, camera, filled))
    assert filled > 0 or camera == sr.PINHOLE


# 8 ---------------------------------------------------------------------------------------------------------------------
# case A of tests/zoom_reference.py, and its case B with an even output width (no 4:2:2 format takes 197) and a wider range
FIT_CASES = {
    "A": dict(zr.CASES["A"]),
    "B'": dict(camera=sr.PINHOLE, out_size=(198, 131), lo=0.5, hi=1.5),
}


def _fit_kw(case):
    c = FIT_CASES[case]
    return c, dict(sigma=zr.SIGMA, camera=c["camera"], out_size=c["out_size"])


def _procedure(p, lens, case, site, targets):
    """the header's procedure through the existing calls -> (zL, sL, zC, sC)"""
    from rssync_amd import stabilize, synth, yuv
    c, kw = _fit_kw(case)
    ow, oh = (W, H) if kw["out_size"] is None else kw["out_size"]
    zl, sl = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=FIT_STEPS, targets=targets, **kw)
    lens_c, cam_c = yuv.chroma_config(lens, W, H, ow, oh, site)
    if targets is None:
        targets = stabilize.stabilize_path(p, zr.TIMES, lens[0], synth.D_TRUE, zr.SIGMA)
    zc, sc = p.fit_zoom(W // 2, H, lens_c, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=FIT_STEPS, targets=targets,
                        **dict(kw, out_size=(ow // 2, oh), out_camera=cam_c))
    return zl, sl, zc, sc


@pytest.mark.parametrize("site", [yr.CENTER, yr.LEFT], ids=["center", "left"])
@pytest.mark.parametrize("own_targets", [False, True], ids=["path", "targets"])
@pytest.mark.parametrize("case", sorted(FIT_CASES))
def test_fit_is_the_maximum_of_the_luma_and_the_chroma_fit_bit_for_bit(scene, case, own_targets, site):
    from rssync_amd import synth
    p, lens = scene["problem"], scene["lens"]
    assert (zr.CASES["A"]["camera"], zr.CASES["A"]["lo"], zr.CASES["A"]["hi"], len(zr.TIMES)) == (sr.LENS, 1.0, 1.5, 9)
    targets = 0.5 * sr.path64(scene["gyro"], zr.TIMES, lens[0], synth.D_TRUE, 0.3) if own_targets else None
    c, kw = _fit_kw(case)
    zl, sl, zc, sc = _procedure(p, lens, case, site, targets)
    got, status = p.fit_zoom_yuv(NV16, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=FIT_STEPS, targets=targets, chroma_site=site,
                                 **kw)
    step = (c["hi"] - c["lo"]) / 2 ** FIT_STEPS
    print(case, "site", site, "targets", own_targets)
    print("  luma  ", zl.tolist(), sl.tolist())
    print("  chroma", zc.tolist(), sc.tolist())
    print("  chroma - luma in steps", ((zc - zl) / step).tolist())
    if case == "A" and site == yr.CENTER and not own_targets:
        # the guard: each plane sets the zoom of some frame, or the maximum is not tested (tests/test_zoomyuv_cpu.py: the
        # float64 bisection has the chroma plane above in frames 0 .. 4 and the luma plane in frames 5 .. 8)
        assert (zc > zl).any() and (zl > zc).any()
    assert got.dtype == np.float64 and status.dtype == np.uint32
    np.testing.assert_array_equal(got.view(np.uint64), np.maximum(zl, zc).view(np.uint64))
    np.testing.assert_array_equal(status, sl | sc)
    for fmt in (I422, I210, P210, P216):
        again, st = p.fit_zoom_yuv(fmt, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=FIT_STEPS, targets=targets, chroma_site=site,
                                   **kw)
        np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))
        np.testing.assert_array_equal(st, status)


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_fit_is_fit_zoom_without_a_sub_sampled_plane_and_refuses_an_odd_output_width_for_422(scene):
    import rssync_amd
    from rssync_amd import synth
    p, lens = scene["problem"], scene["lens"]
    for case in sorted(zr.CASES):
        c = zr.CASES[case]
        kw = dict(sigma=zr.SIGMA, camera=c["camera"], out_size=c["out_size"])
        for steps in (zr.STEPS, FIT_STEPS):
            want, want_status = p.fit_zoom(W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=steps, **kw)
            for fmt in F444:
                got, status = p.fit_zoom_yuv(fmt, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=steps, **kw)
                np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
                np.testing.assert_array_equal(status, want_status)
    c = zr.CASES["B"]
    assert c["out_size"][0] % 2 == 1
    for fmt in (NV16, I422, P210):
        with pytest.raises(rssync_amd.RsSyncError, match="even"):
            p.fit_zoom_yuv(fmt, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], sigma=zr.SIGMA, camera=c["camera"], out_size=c["out_size"])


# 10 --------------------------------------------------------------------------------------------------------------------
def test_frames_rendered_at_their_fitted_zooms_are_clear_in_every_plane(scene, planes):
    import rssync_amd
    from rssync_amd import synth
    p, times, lens, d = scene["problem"], scene["times"], scene["lens"], planes[SCENE_SIZE]
    c, kw = _fit_kw("A")
    fitted, status = p.fit_zoom_yuv(NV16, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], steps=zr.STEPS, **kw)
    assert not status.any()
    _, n_at = p.stabilize_yuv_zoomed(NV16, d[NV16], times, lens, synth.D_TRUE, fitted[zr.SCENE], sigma=zr.SIGMA)
    print("fitted", fitted.tolist(), "outside at the fitted zooms", n_at.tolist())
    assert n_at.shape == (N, 2) and (n_at == 0).all(), n_at
    smoothed = p.dynamic_zoom_yuv(NV16, W, H, lens, zr.TIMES, synth.D_TRUE, c["lo"], c["hi"], zr.WINDOW, steps=zr.STEPS, **kw)
    np.testing.assert_array_equal(smoothed, p.smooth_zooms(zr.TIMES, fitted, zr.WINDOW))
    assert (smoothed >= fitted).all() and (smoothed > fitted).any()
    _, n_smooth = p.stabilize_yuv_zoomed(NV16, d[NV16], times, lens, synth.D_TRUE, smoothed[zr.SCENE], sigma=zr.SIGMA)
    assert (n_smooth == 0).all(), n_smooth
    with pytest.raises(rssync_amd.RsSyncError, match="not clear"):
        p.dynamic_zoom_yuv(NV16, W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.02, zr.WINDOW, steps=zr.STEPS, **kw)


# 11 --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene, planes):
    from rssync_amd import color, synth, zoomyuv
    p, times, lens, d = scene["problem"], scene["times"], scene["lens"], planes[SCENE_SIZE]
    y, uv = (np.ascontiguousarray(a) for a in d[NV16])
    y10, uv10 = (np.ascontiguousarray(a) for a in d[P210])
    want, want_n = _alone(p, NV16, d[NV16], times, lens, ZOOMS, sigma=sr.SIGMA, camera=sr.LENS, filter=0, fills=FILLS[8])
    lib = zoomyuv.library()
    lib.rssync_set_panic_mode(1)
    PD = C.POINTER(C.c_double)
    L, T, Z = np.ascontiguousarray(lens, np.float64), np.ascontiguousarray(times, np.float64), np.array(ZOOMS)
    out_y, out_uv = np.zeros_like(y), np.zeros_like(uv)
    out_y10, out_uv10 = np.zeros_like(y10), np.zeros_like(uv10)
    nan, inf = float("nan"), float("inf")

    def err():
        return lib.rssync_last_error().decode()

    def image(arrays, w, h, size=1):
        """NV16's planes: Y and the interleaved U V, both w samples by h rows"""
        img = color.ColorImage()
        for k, a in enumerate(arrays):
            img.plane[k] = a if isinstance(a, int) or a is None else a.ctypes.data
            img.pitch[k], img.stride[k] = size * w, size * w * h
        return img

    def prm_with(site=0, fill_set=1, fills=FILLS[8], **kw):
        q = color.ColorParams()
        q.stab = color.StabilizeParams(**dict(dict(sigma=sr.SIGMA), **kw))
        q.chroma_site, q.fill_set = site, fill_set
        for k in range(4):
            q.fill[k] = fills[k]
        return q

    def render(fmt=NV16, src=None, dst=None, w=W, h=H, ow=W, oh=H, prm=None, z=Z, edit=None):
        src = image((y, uv), w, h) if src is None else src
        dst = image((out_y, out_uv), ow, oh) if dst is None else dst
        if edit:
            edit(src, dst)
        prm = prm_with() if prm is None else prm
        counts = np.zeros((N, 2), np.uint64)
        rc_ = lib.rssync_zoomyuv_stabilize(p._h, fmt, C.byref(src), N, w, h, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE, None, C.byref(prm),
                                           C.byref(dst), ow, oh, counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           None if z is None else np.ascontiguousarray(z, np.float64).ctypes.data_as(PD))
        return rc_, counts

    def set_(which, field, k, value):
        def edit(src, dst):
            getattr(src if which == "in" else dst, field)[k] = value
        return edit

    def p210(**kw):
        return dict(dict(fmt=P210, src=image((y10, uv10), W, H, 2), dst=image((out_y10, out_uv10), W, H, 2), prm=prm_with(fills=FILLS[10])),
                    **kw)

    cases = [("no zooms", dict(z=None)), ("zoom", dict(z=[1.0, 0.0, 1.0])), ("zoom", dict(z=[1.0, -1.0, 1.0])),
             ("zoom", dict(z=[1.0, 1.0, nan])), ("zoom", dict(z=[inf, 1.0, 1.0]))]
    cases += [("format", dict(fmt=f)) for f in (0, 1, 2, 3, 16, 17, 18, 19, 35, 47, 52, -1)]
    cases += [("is NULL", dict(edit=set_("in", "plane", 1, None))), ("is NULL", dict(edit=set_("out", "plane", 0, None))),
              ("pitch", dict(edit=set_("in", "pitch", 0, W - 1))), ("pitch", dict(edit=set_("out", "pitch", 1, W - 1))),
              ("even", dict(w=W - 1)), ("even", dict(ow=W - 1)),
              ("alignment", p210(edit=set_("in", "pitch", 0, 2 * W + 1))), ("alignment", p210(edit=set_("out", "pitch", 1, 2 * W + 3))),
              ("overlaps", dict(dst=image((out_y, y.ctypes.data + 8), W, H))), ("fill 1", dict(prm=prm_with(fills=(0, 256, 0, 0)))),
              ("fill 0", p210(prm=prm_with(fills=(1024, 0, 0, 0)))), ("filter", dict(prm=prm_with(filter=2))),
              ("chroma_site", dict(prm=prm_with(site=2)))]
    for match, kw in cases:
        rc_, _ = render(**kw)
        assert rc_ != 0, (match, kw)
        assert match in err(), (match, err())
    rc_, _ = render(prm=prm_with(zoom=-7.0))                 # (params->stab.zoom is not read)
    assert rc_ == 0, err()
    np.testing.assert_array_equal(out_y, want[0])
    rc_, _ = render(h=H - 1, oh=H - 1)                       # (odd heights are allowed)
    assert rc_ == 0, err()

    # the fit
    zs, st = np.zeros(9), np.zeros(9, np.uint32)
    T9 = np.ascontiguousarray(zr.TIMES)

    def fit(fmt=NV16, lo=1.0, hi=1.5, steps=zr.STEPS, prm=None, ow=W):
        prm = prm_with(fill_set=0, sigma=zr.SIGMA) if prm is None else prm
        return lib.rssync_zoomyuv_fit(p._h, fmt, W, H, L.ctypes.data, ow, H, T9.ctypes.data_as(PD), 9, synth.D_TRUE, None, C.byref(prm), lo, hi,
                                      steps, zs.ctypes.data_as(PD), st.ctypes.data_as(C.POINTER(C.c_uint32)))

    for match, kw in (("below zoom_hi", dict(lo=1.5, hi=1.5)), ("below zoom_hi", dict(lo=1.5, hi=1.2)), ("steps", dict(steps=41)),
                      ("format", dict(fmt=1)), ("format", dict(fmt=17)), ("format", dict(fmt=35)), ("format", dict(fmt=52)),
                      ("chroma_site", dict(prm=prm_with(site=2, fill_set=0))), ("even", dict(ow=W - 1)), ("zoom_lo", dict(lo=0.0)),
                      ("zoom_hi", dict(hi=inf))):
        assert fit(**kw) != 0, kw
        assert match in err(), (match, err())
    assert fit(prm=prm_with(fill_set=0, sigma=zr.SIGMA, zoom=-7.0)) == 0, err()
    again, _ = p.fit_zoom_yuv(NV16, W, H, lens, zr.TIMES, synth.D_TRUE, 1.0, 1.5, steps=zr.STEPS, sigma=zr.SIGMA)
    np.testing.assert_array_equal(zs, again)
    with pytest.raises(ValueError):
        p.stabilize_yuv_zoomed(NV16, d[NV16], times, lens, synth.D_TRUE, [1.0, 1.0])

    # ... and a good call gives case 1's bytes
    out_y[:], out_uv[:] = 0, 0
    rc_, counts = render()
    assert rc_ == 0, err()
    np.testing.assert_array_equal(out_y, want[0])
    np.testing.assert_array_equal(out_uv, want[1])
    np.testing.assert_array_equal(counts, want_n)
    got, got_n = p.stabilize_yuv_zoomed(NV16, d[NV16], times, lens, synth.D_TRUE, ZOOMS, sigma=sr.SIGMA, fills=FILLS[8])
    _same(got, got_n, want, want_n)
