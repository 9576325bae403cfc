"""The colour front on the device (include/rssync_color.h, csrc/kernels/color.hpp) against the stabiliser it is defined
by -- every plane is rssync_stabilize_frames of that plane with that plane's camera, byte for byte --, its numpy
restatement (tests/color_reference.py) and global-shutter renders of the colour scene at the smoothed path's orientations."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr

pytestmark = pytest.mark.gpu

# luma (rows, cols): the smallest 4:2:0 frame, one under a 64 x 4 tile of chroma samples, an odd chroma size that is no
# multiple of the tile (165 x 99), the scene's
SIZES = [(4, 4), (38, 30), (330, 198), (rr.ROWS, rr.COLS)]
OUT = (200, 320)        # rows, cols of the other output size
SITES = [cr.CENTER, cr.LEFT]
CAMERAS = [sr.LENS, sr.PINHOLE]
N = 2                   # frames of the byte-for-byte cases


def _problem(gyro=None):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    if gyro is not None:
        p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def scene(built):
    s = dict(cr.scene())
    s["problem"] = _problem(s["gyro"])
    return s


@pytest.fixture(scope="module")
def planes():
    """per luma size: lens and N frames of Y, U, V, UV and RGBA -- the scene's planes at its size, noise elsewhere (read-only)"""
    out = {}
    col = cr.scene()
    for rows, cols in SIZES:
        rng = np.random.default_rng(rows * 1000 + cols)
        if (rows, cols) == (rr.ROWS, rr.COLS):
            y, u, v = (np.array(col[k][:N]) for k in ("y", "u", "v"))
        else:
            y = rng.integers(0, 256, size=(N, rows, cols), dtype=np.uint8)
            u, v = (rng.integers(0, 256, size=(N, rows // 2, cols // 2), dtype=np.uint8) for _ in range(2))
        d = dict(lens=rr.scaled_lens(rows, cols), y=y, u=u, v=v, uv=np.stack([u, v], axis=-1),
                 rgba=rng.integers(0, 256, size=(N, rows, cols, 4), dtype=np.uint8))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(rows, cols)] = d
    return out


def _outs(rows, cols):
    """(out_size argument (cols, rows), out rows, out cols): the input's size and OUT"""
    return [(None, rows, cols), ((OUT[1], OUT[0]), OUT[0], OUT[1])]


def _targets(scene, n=N):
    """explicit targets: another smoothing's orientations, not of unit length (the library normalises them)"""
    from rssync_amd import synth
    return 2.5 * sr.path64(scene["gyro"], scene["times"][:n], scene["lens"][0], synth.D_TRUE, 0.3)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_gray8_is_the_stabiliser_byte_for_byte(scene, planes, size):
    from rssync_amd import color, synth
    p, times, d = scene["problem"], scene["times"][:N], planes[size]
    for out_size, orows, ocols in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, fill=9)
        want, want_n = p.stabilize_frames(d["y"], times, d["lens"], synth.D_TRUE, **kw)
        got, got_n = p.stabilize_color(color.GRAY8, d["y"], times, d["lens"], synth.D_TRUE, **kw)
        assert got.shape == (N, orows, ocols)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_n[:, 0], want_n)
        assert (got_n[:, 1] == 0).all()
    # NULL parameters and a zeroed struct are the defaults too
    rows, cols = size
    lib = color.library()
    want, want_n = p.stabilize_frames(d["y"], times, d["lens"], synth.D_TRUE)
    L, T, f = np.ascontiguousarray(d["lens"], np.float64), np.ascontiguousarray(times, np.float64), np.ascontiguousarray(d["y"])
    for prm in (None, C.byref(color.ColorParams())):
        out, n_out = np.zeros_like(f), np.zeros((N, 2), np.uint64)
        src, dst = color.ColorImage(), color.ColorImage()
        src.plane[0], src.pitch[0], src.stride[0] = f.ctypes.data, cols, rows * cols
        dst.plane[0], dst.pitch[0], dst.stride[0] = out.ctypes.data, cols, rows * cols
        assert lib.rssync_color_stabilize(p._h, color.GRAY8, C.byref(src), N, cols, rows, T.ctypes.data_as(C.POINTER(C.c_double)), L.ctypes.data,
                                          synth.D_TRUE, None, prm, C.byref(dst), cols, rows,
                                          n_out.ctypes.data_as(C.POINTER(C.c_uint64))) == 0, lib.rssync_last_error()
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(n_out[:, 0], want_n)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("size", SIZES)
def test_luma_plane_is_the_stabiliser_byte_for_byte(scene, planes, size, camera):
    from rssync_amd import color, synth
    p, times, d = scene["problem"], scene["times"][:N], planes[size]
    rows, cols = size
    for out_size, orows, ocols in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, zoom=1.1)
        want, want_n = p.stabilize_frames(d["y"], times, d["lens"], synth.D_TRUE, fill=3, **kw)
        (y1, uv), n1 = p.stabilize_color(color.NV12, (d["y"], d["uv"]), times, d["lens"], synth.D_TRUE, fill=3, **kw)
        (y2, u, v), n2 = p.stabilize_color(color.I420, (d["y"], d["u"], d["v"]), times, d["lens"], synth.D_TRUE, fill=3, **kw)
        assert uv.shape == (N, orows // 2, ocols // 2, 2) and u.shape == v.shape == (N, orows // 2, ocols // 2)
        np.testing.assert_array_equal(y1, want)
        np.testing.assert_array_equal(y2, want)
        np.testing.assert_array_equal(n1[:, 0], want_n)
        np.testing.assert_array_equal(n2[:, 0], want_n)
        for fmt in (color.GRAY8, color.NV12, color.I420, color.RGBA32):
            got = p.color_map(fmt, 0, cols, rows, d["lens"], times[1], synth.D_TRUE, **kw)
            np.testing.assert_array_equal(got.view(np.uint32), p.stabilize_map(cols, rows, d["lens"], times[1], synth.D_TRUE, **kw).view(np.uint32))


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("size", SIZES)
def test_rgba_is_the_stabiliser_per_channel(scene, planes, size, camera):
    from rssync_amd import color, synth
    p, times, d = scene["problem"], scene["times"][:N], planes[size]
    fills = (7, 99, 200, 31)
    for out_size, orows, ocols in _outs(*size):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera)
        got, got_n = p.stabilize_color(color.RGBA32, d["rgba"], times, d["lens"], synth.D_TRUE, fills=fills, fill=255, **kw)
        plain, plain_n = p.stabilize_color(color.RGBA32, d["rgba"], times, d["lens"], synth.D_TRUE, fill=17, **kw)
        assert got.shape == (N, orows, ocols, 4)
        for k in range(4):
            want, want_n = p.stabilize_frames(d["rgba"][..., k], times, d["lens"], synth.D_TRUE, fill=fills[k], **kw)
            np.testing.assert_array_equal(got[..., k], want, err_msg="channel %d" % k)
            np.testing.assert_array_equal(got_n[:, 0], want_n)
        np.testing.assert_array_equal(plain_n, got_n)
        filled = np.stack([~sr.inside(p.stabilize_map(size[1], size[0], d["lens"], t, synth.D_TRUE, **kw), *size) for t in times])
        assert filled.sum() == got_n[:, 0].sum()
        assert (plain[filled] == (17, 17, 17, 255)).all() and (plain[~filled] == got[~filled]).all()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoom", [1.0, 1.3])
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_i420_chroma_is_nv12_chroma_deinterleaved(scene, planes, site, camera, zoom):
    from rssync_amd import color, synth
    p, times = scene["problem"], scene["times"][:N]
    some_outside = 0
    for size in SIZES:
        d = planes[size]
        for out_size, _, _ in _outs(*size):
            kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, zoom=zoom, chroma_site=site, fills=(1, 2, 3))
            (y1, uv), n1 = p.stabilize_color(color.NV12, (d["y"], d["uv"]), times, d["lens"], synth.D_TRUE, **kw)
            (y2, u, v), n2 = p.stabilize_color(color.I420, (d["y"], d["u"], d["v"]), times, d["lens"], synth.D_TRUE, **kw)
            np.testing.assert_array_equal(uv[..., 0], u)
            np.testing.assert_array_equal(uv[..., 1], v)
            np.testing.assert_array_equal(y1, y2)
            np.testing.assert_array_equal(n1, n2)
            some_outside += int(n1[:, 1].sum())
    assert some_outside > 0


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_chroma_planes_are_the_stabiliser_with_the_chroma_camera(scene, planes, site, camera):
    """explicit targets: plane 1's map is rssync_stabilize_map of the chroma lens, T_c and the chroma output camera bit for
    bit, and U and V are rssync_stabilize_frames of those planes byte for byte"""
    from rssync_amd import color, synth
    p, times, targets = scene["problem"], scene["times"][:N], _targets(scene)
    for size in SIZES:
        rows, cols = size
        d = planes[size]
        lens_c = cr.chroma_lens(d["lens"], site)
        times_c = np.array([cr.chroma_time(t, d["lens"], rows, site) for t in times])
        for (out_size, orows, ocols), zoom in zip(_outs(*size), (1.3, 1.0)):
            cam_c = cr.chroma_camera(d["lens"], rows, cols, orows, ocols, site, zoom)
            kw = dict(camera=camera, iterations=3)
            ckw = dict(out_size=(ocols // 2, orows // 2), out_camera=cam_c, **kw)
            got = p.color_map(color.NV12, 1, cols, rows, d["lens"], times[1], synth.D_TRUE, target=targets[1], out_size=out_size, zoom=zoom,
                              chroma_site=site, **kw)
            want = p.stabilize_map(cols // 2, rows // 2, lens_c, times_c[1], synth.D_TRUE, target=targets[1], **ckw)
            assert got.shape == (orows // 2, ocols // 2, 2)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
            (_, u, v), n_out = p.stabilize_color(color.I420, (d["y"], d["u"], d["v"]), times, d["lens"], synth.D_TRUE, targets=targets,
                                                 out_size=out_size, zoom=zoom, chroma_site=site, fills=(0, 55, 66), **kw)
            want_u, want_n = p.stabilize_frames(d["u"], times_c, lens_c, synth.D_TRUE, targets=targets, fill=55, **ckw)
            want_v, _ = p.stabilize_frames(d["v"], times_c, lens_c, synth.D_TRUE, targets=targets, fill=66, **ckw)
            np.testing.assert_array_equal(u, want_u, err_msg="U %s -> %s" % (size, out_size))
            np.testing.assert_array_equal(v, want_v, err_msg="V %s -> %s" % (size, out_size))
            np.testing.assert_array_equal(n_out[:, 1], want_n)


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_chroma_along_the_path_against_the_restatement(scene, site, camera):
    """targets = NULL: the chroma bytes are the restated sampler's from the device's own plane-1 map, the count is that
    map's, and the map is within the tolerance of the float64 restatement (which takes the path at the LUMA's centre time).
    Both output sizes at zoom 1, and the input's size at zoom 0.8: at zoom 1 the pinhole camera's view lies wholly inside
    the fisheye frame (the restatement counts no outside sample for it), so only the zoomed-out case makes the count and the
    fills say something with that camera.  The restatement's float32 spread at zoom 0.8 is 6.2e-5 to 7.2e-5 chroma px, so
    the tolerance of zoom 1 (below four times that) asks no less there."""
    from rssync_amd import color, synth
    p, g, lens, times = scene["problem"], scene["gyro"], scene["lens"], scene["times"]
    col = cr.scene(site)
    tol = cr.device_tolerance(camera)
    for (out_size, orows, ocols), zoom in zip(_outs(rr.ROWS, rr.COLS) + _outs(rr.ROWS, rr.COLS)[:1], (1.0, 1.0, 0.8)):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, chroma_site=site, zoom=zoom)
        (_, uv), n_out = p.stabilize_color(color.NV12, (col["y"], col["uv"]), times, lens, synth.D_TRUE, fills=(0, 77, 88), **kw)
        for k in range(rr.N_FRAMES):
            m = p.color_map(color.NV12, 1, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw)
            want, want_n = cr.sample_pairs(col["uv"][k], m, fill=(77, 88))
            np.testing.assert_array_equal(uv[k], want, err_msg="frame %d" % k)
            assert int(n_out[k, 1]) == want_n == int((~sr.inside(m, cr.C_ROWS, cr.C_COLS)).sum())
            ref = cr.chroma_map64(g, lens, rr.ROWS, rr.COLS, times[k], synth.D_TRUE, site, sigma=sr.SIGMA, out_size=out_size, camera=camera,
                                  zoom=zoom)
            diff = np.abs(m.astype(np.float64) - ref).max()
            print("site %d camera %d out %s zoom %.1f frame %d: %.3g chroma px (tolerance %.3g), %d outside" %
                  (site, camera, out_size, zoom, k, diff, tol, n_out[k, 1]))
            assert diff <= tol
            # (the restatement's own count is 0 with the pinhole at zoom 1, thousands otherwise: a sample at the edge may flip)
            assert (n_out[k, 1] > 0) == ((~sr.inside(ref, cr.C_ROWS, cr.C_COLS)).sum() > 0)


# 7 ---------------------------------------------------------------------------------------------------------------------
def _against_truth(name, img, ok, m, ref_img, ref_map, raw, truth, rows, cols, tol):
    err, ref_err = rr.grey_error(img, truth, ok), rr.grey_error(ref_img, truth, sr.inside(ref_map, rows, cols))
    raw_err = rr.grey_error(raw, truth, ok)
    ref_ok = sr.inside(ref_map, rows, cols)
    worst = np.abs(img.astype(int) - ref_img.astype(int))[ok & ref_ok].max()
    flips = ok != ref_ok
    print("%s: device %.4f reference %.4f raw %.1f; %d grey levels from the reference image, %d inside flags differ" %
          (name, err, ref_err, raw_err, worst, flips.sum()))
    assert err <= 1.05 * ref_err, (name, err, ref_err)
    assert err <= rr.RATIO * raw_err, (name, err, raw_err)
    assert worst <= 1, (name, worst)
    assert sr.near_edge(ref_map, rows, cols, tol)[flips].all(), name


@pytest.mark.parametrize("site", SITES)
def test_error_against_the_global_shutter_truth_per_plane(scene, site):
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col, truth_uv = cr.scene(site), cr.truth(site)
    kw = dict(sigma=sr.SIGMA, chroma_site=site)
    (y, uv), _ = p.stabilize_color(color.NV12, (col["y"], col["uv"]), times, lens, synth.D_TRUE, **kw)
    for k in range(rr.N_FRAMES):
        m = p.color_map(color.NV12, 0, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw)
        ref_map = sr.reference_maps()[k]
        _against_truth("Y frame %d" % k, y[k], sr.inside(m, rr.ROWS, rr.COLS), m, rr.sample(col["y"][k], ref_map)[0], ref_map, col["y"][k],
                       sr.truth()[k], rr.ROWS, rr.COLS, sr.device_tolerance(sr.LENS))
        m = p.color_map(color.NV12, 1, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw)
        ref_map = cr.reference_maps(site)[k]
        ok = sr.inside(m, cr.C_ROWS, cr.C_COLS)
        for c, name in enumerate("uv"):
            _against_truth("%s frame %d" % (name.upper(), k), uv[k, ..., c], ok, m, sr.sample(col[name][k], ref_map, fill=128)[0], ref_map,
                           col[name][k], truth_uv[c][k], cr.C_ROWS, cr.C_COLS, cr.device_tolerance(sr.LENS))


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_chunks_pitched_views_and_device_tensors_do_not_change_the_result(scene):
    """a budget of one and a half frames per slot: the three NV12 frames go as three chunks through both slots into a
    200 x 320 output; pitched numpy views and device tensors give the same bytes; the padding of `out` is not written"""
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col = cr.scene()
    y, uv = col["y"], col["uv"]
    orows, ocols = OUT
    kw = dict(sigma=sr.SIGMA, out_size=(ocols, orows))
    (one_y, one_uv), one_n = p.stabilize_color(color.NV12, (y, uv), times, lens, synth.D_TRUE, **kw)
    assert one_y.shape == (rr.N_FRAMES, orows, ocols) and one_uv.shape == (rr.N_FRAMES, orows // 2, ocols // 2, 2)
    per_frame = (rr.ROWS + 1) * 36 + (cr.C_ROWS + 1) * 36 + rr.ROWS * rr.COLS * 3 // 2 + orows * ocols * 3 // 2
    (got_y, got_uv), got_n = color.stabilize_color_budget(p, color.NV12, (y, uv), times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, **kw)
    np.testing.assert_array_equal(got_y, one_y)
    np.testing.assert_array_equal(got_uv, one_uv)
    np.testing.assert_array_equal(got_n, one_n)
    # pitched views in, pitched views out
    wide_y = np.zeros((rr.N_FRAMES, rr.ROWS + 2, rr.COLS + 45), np.uint8)
    wide_y[:, 1:1 + rr.ROWS, 7:7 + rr.COLS] = y
    wide_uv = np.zeros((rr.N_FRAMES, cr.C_ROWS, cr.C_COLS + 9, 2), np.uint8)
    wide_uv[:, :, 4:4 + cr.C_COLS] = uv
    dst_y = np.full((rr.N_FRAMES, orows + 3, ocols + 21), 201, np.uint8)
    dst_uv = np.full((rr.N_FRAMES, orows // 2 + 1, ocols // 2 + 5, 2), 202, np.uint8)
    views = (dst_y[:, 1:1 + orows, 5:5 + ocols], dst_uv[:, 1:, 2:2 + ocols // 2])
    res, n = p.stabilize_color(color.NV12, (wide_y[:, 1:1 + rr.ROWS, 7:7 + rr.COLS], wide_uv[:, :, 4:4 + cr.C_COLS]), times, lens,
                               synth.D_TRUE, out=views, **kw)
    assert res is views
    np.testing.assert_array_equal(views[0], one_y)
    np.testing.assert_array_equal(views[1], one_uv)
    np.testing.assert_array_equal(n, one_n)
    pad_y, pad_uv = np.ones(dst_y.shape, bool), np.ones(dst_uv.shape, bool)
    pad_y[:, 1:1 + orows, 5:5 + ocols] = False
    pad_uv[:, 1:, 2:2 + ocols // 2] = False
    assert (dst_y[pad_y] == 201).all() and (dst_uv[pad_uv] == 202).all()
    # device tensors, contiguous and pitched
    dev = (torch.from_numpy(np.array(y)).to("cuda:0"), torch.from_numpy(np.array(uv)).to("cuda:0"))
    (dy, duv), dn = p.stabilize_color(color.NV12, dev, times, lens, synth.D_TRUE, **kw)
    assert isinstance(dy, torch.Tensor) and isinstance(duv, torch.Tensor)
    np.testing.assert_array_equal(dy.cpu().numpy(), one_y)
    np.testing.assert_array_equal(duv.cpu().numpy(), one_uv)
    np.testing.assert_array_equal(dn, one_n)
    dwide = (torch.from_numpy(wide_y).to("cuda:0")[:, 1:1 + rr.ROWS, 7:7 + rr.COLS], torch.from_numpy(wide_uv).to("cuda:0")[:, :, 4:4 + cr.C_COLS])
    dout_y = torch.full((rr.N_FRAMES, orows, ocols + 19), 9, dtype=torch.uint8, device="cuda:0")
    dout_uv = torch.full((rr.N_FRAMES, orows // 2, ocols // 2 + 3, 2), 8, dtype=torch.uint8, device="cuda:0")
    p.stabilize_color(color.NV12, dwide, times, lens, synth.D_TRUE, out=(dout_y[:, :, 3:3 + ocols], dout_uv[:, :, 1:1 + ocols // 2]), **kw)
    back_y, back_uv = dout_y.cpu().numpy(), dout_uv.cpu().numpy()
    np.testing.assert_array_equal(back_y[:, :, 3:3 + ocols], one_y)
    np.testing.assert_array_equal(back_uv[:, :, 1:1 + ocols // 2], one_uv)
    assert (back_y[:, :, :3] == 9).all() and (back_y[:, :, 3 + ocols:] == 9).all()
    assert (back_uv[:, :, :1] == 8).all() and (back_uv[:, :, 1 + ocols // 2:] == 8).all()
    # host frames into device tensors and the other way, I420 and RGBA through the chunks too
    (hy, huv), _ = p.stabilize_color(color.NV12, dev, times, lens, synth.D_TRUE, out=(np.zeros_like(one_y), np.zeros_like(one_uv)), **kw)
    np.testing.assert_array_equal(hy, one_y)
    np.testing.assert_array_equal(huv, one_uv)
    (iy, iu, iv), i_n = color.stabilize_color_budget(p, color.I420, (y, col["u"], col["v"]), times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, **kw)
    np.testing.assert_array_equal(iy, one_y)
    np.testing.assert_array_equal(np.stack([iu, iv], axis=-1), one_uv)
    np.testing.assert_array_equal(i_n, one_n)
    rgba = np.stack([y, y[:, ::-1], y[:, :, ::-1], y[::-1]], axis=-1)
    want, want_n = p.stabilize_color(color.RGBA32, rgba, times, lens, synth.D_TRUE, **kw)
    got, got_n = color.stabilize_color_budget(p, color.RGBA32, rgba, times, lens, synth.D_TRUE, 2 * 1.5 * (381 * 36 + 4 * rr.ROWS * rr.COLS + 4 * orows * ocols),
                                              **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_n, want_n)


def test_mixed_memory_kinds_across_chunks(scene, monkeypatch):
    """NV12 device tensors into host arrays and host arrays into device tensors, each with a budget of one and a half of
    the frames that then pass through a slot: three chunks through both slots.  Where the output planes lie in a slot
    depends on whether the input planes pass through it too; the result is the unchunked all-host call's."""
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col = cr.scene()
    y, uv = col["y"], col["uv"]
    orows, ocols = OUT
    kw = dict(sigma=sr.SIGMA, out_size=(ocols, orows))
    (one_y, one_uv), one_n = p.stabilize_color(color.NV12, (y, uv), times, lens, synth.D_TRUE, **kw)
    tabs, px_in, px_out = (rr.ROWS + 1) * 36 + (cr.C_ROWS + 1) * 36, rr.ROWS * rr.COLS * 3 // 2, orows * ocols * 3 // 2
    dev = (torch.from_numpy(np.array(y)).to("cuda:0"), torch.from_numpy(np.array(uv)).to("cuda:0"))
    (got_y, got_uv), got_n = color.stabilize_color_budget(p, color.NV12, dev, times, lens, synth.D_TRUE, 2 * 1.5 * (tabs + px_out), **kw)
    np.testing.assert_array_equal(got_y, one_y)
    np.testing.assert_array_equal(got_uv, one_uv)
    np.testing.assert_array_equal(got_n, one_n)
    # the budget wrapper writes host arrays: hand the launcher device tensors in their place
    lib = color.library()
    launcher = lib.rship_color_frames
    dout = (torch.zeros(one_y.shape, dtype=torch.uint8, device="cuda:0"), torch.zeros(one_uv.shape, dtype=torch.uint8, device="cuda:0"))
    dst, _keep = color._image(color.NV12, dout, rr.N_FRAMES, orows, ocols, True)
    monkeypatch.setattr(lib, "rship_color_frames", lambda *a: launcher(*a[:6], C.byref(dst), *a[7:]))
    _, got_n = color.stabilize_color_budget(p, color.NV12, (y, uv), times, lens, synth.D_TRUE, 2 * 1.5 * (tabs + px_in), **kw)
    np.testing.assert_array_equal(dout[0].cpu().numpy(), one_y)
    np.testing.assert_array_equal(dout[1].cpu().numpy(), one_uv)
    np.testing.assert_array_equal(got_n, one_n)


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene):
    import rssync_amd
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col = cr.scene()
    y, uv, u, v = (np.ascontiguousarray(col[k]) for k in ("y", "uv", "u", "v"))
    W, H, NF = rr.COLS, rr.ROWS, rr.N_FRAMES
    (want_y, want_uv), want_n = p.stabilize_color(color.NV12, (y, uv), times, lens, synth.D_TRUE, sigma=sr.SIGMA)
    lib = color.library()
    lib.rssync_set_panic_mode(1)
    L, T = np.ascontiguousarray(lens, np.float64), np.ascontiguousarray(times, np.float64)
    out_y, out_uv, out_u, out_v = np.zeros_like(y), np.zeros_like(uv), np.zeros_like(u), np.zeros_like(v)
    PD = C.POINTER(C.c_double)

    def image(arrays, w, h, fmt):
        img = color.ColorImage()
        rows = {color.NV12: (w, w), color.I420: (w, w // 2, w // 2), color.RGBA32: (4 * w,), color.GRAY8: (w,)}[fmt]
        heights = {color.NV12: (h, h // 2), color.I420: (h, h // 2, h // 2), color.RGBA32: (h,), color.GRAY8: (h,)}[fmt]
        for k, a in enumerate(arrays):
            img.plane[k] = a if isinstance(a, int) or a is None else a.ctypes.data
            img.pitch[k], img.stride[k] = rows[k], rows[k] * heights[k]
        return img

    def prm_with(site=0, fill_set=0, fills=(0, 0, 0, 0), **kw):
        q = color.ColorParams()
        q.stab = color.StabilizeParams(**dict(dict(sigma=sr.SIGMA), **kw))
        q.chroma_site, q.fill_set = site, fill_set
        for k in range(4):
            q.fill[k] = fills[k]
        return q

    def call(fmt=color.NV12, src=None, dst=None, w=W, h=H, ow=W, oh=H, n=NF, prm=None, t=T, handle=None, delay=synth.D_TRUE, edit=None):
        src = image((y, uv), w, h, color.NV12) if src is None else src
        dst = image((out_y, out_uv), ow, oh, color.NV12) if dst is None else dst
        if edit:
            edit(src, dst)
        prm = prm_with() if prm is None else prm
        return lib.rssync_color_stabilize(p._h if handle is None else handle, fmt, C.byref(src), n, w, h, t.ctypes.data_as(PD) if t is not None else None,
                                          L.ctypes.data, delay, None, C.byref(prm), C.byref(dst), ow, oh, None)

    def bad(match, **kw):
        assert call(**kw) != 0, match
        msg = lib.rssync_last_error().decode()
        assert match in msg, (match, msg)

    def set_(which, field, k, value):
        def edit(src, dst):
            getattr(src if which == "in" else dst, field)[k] = value
        return edit

    bad("format", fmt=4)
    bad("format", fmt=-1)
    bad("chroma_site", prm=prm_with(site=2))
    bad("chroma_site", prm=prm_with(site=-1))
    bad("is NULL", edit=set_("in", "plane", 1, None))
    bad("is NULL", edit=set_("out", "plane", 0, None))
    bad("is NULL", fmt=color.I420, src=image((y, u, None), W, H, color.I420), dst=image((out_y, out_u, out_v), W, H, color.I420))
    bad("pitch", edit=set_("in", "pitch", 0, W - 1))
    bad("pitch", edit=set_("in", "pitch", 1, W - 1))
    bad("pitch", edit=set_("out", "pitch", 1, W - 1))
    bad("pitch", fmt=color.I420, src=image((y, u, v), W, H, color.I420), dst=image((out_y, out_u, out_v), W, H, color.I420),
        edit=set_("out", "pitch", 2, W // 2 - 1))
    bad("pitch", fmt=color.RGBA32, src=image((y,), W // 4, H, color.RGBA32), dst=image((out_y,), W // 4, H, color.RGBA32), w=W // 4, ow=W // 4,
        edit=set_("in", "pitch", 0, W - 1))
    bad("stride", edit=set_("in", "stride", 1, W * (H // 2) - 1))
    bad("stride", edit=set_("out", "stride", 0, W * H - 1))
    assert call(n=1, src=image((y, uv), W, H, color.NV12), edit=set_("in", "stride", 1, 0)) == 0     # (one frame: no stride is read)
    bad("even", w=W - 1)
    bad("even", h=H - 1)
    bad("even", ow=W - 1)
    bad("even", oh=H - 1)
    bad("too small", w=2, h=2)
    bad("too small", ow=2)
    bad("too small", fmt=color.GRAY8, w=1)
    bad("fill 1", prm=prm_with(fill_set=1, fills=(0, 256, 0, 0)))
    bad("fill 0", prm=prm_with(fill_set=1, fills=(-1, 0, 0, 0)))
    bad("fill 3", fmt=color.RGBA32, src=image((y,), W // 4, H, color.RGBA32), dst=image((out_y,), W // 4, H, color.RGBA32), w=W // 4, ow=W // 4,
        prm=prm_with(fill_set=1, fills=(0, 0, 0, 300)))
    bad("fill", prm=prm_with(fill=256))
    assert call(prm=prm_with(fill_set=1, fills=(1, 2, 3, 0), fill=999)) == 0, lib.rssync_last_error().decode()   # (stab.fill is not read)
    bad("overlaps", dst=image((out_y, y.ctypes.data + 8), W, H, color.NV12))          # out UV inside in Y
    bad("overlaps", dst=image((uv.ctypes.data, out_uv), W, H, color.NV12))            # out Y over in UV
    dev_uv = torch.zeros((NF, H // 2, W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bad("mixed kinds", src=image((y, dev_uv.data_ptr()), W, H, color.NV12))
    bad("mixed kinds", dst=image((out_y, dev_uv.data_ptr()), W, H, color.NV12))
    # the stabiliser's own
    empty = _problem()
    bad("no gyro data", handle=empty._h)
    bad("leaves the gyro data", delay=synth.D_TRUE + 5.0)
    bad("no frame times", t=None)
    bad("sigma", prm=prm_with(sigma=-0.1))
    bad("camera", prm=prm_with(camera=2))
    bad("iterations", prm=prm_with(iterations=9))
    bad("given together", prm=prm_with(fx=300.0))
    # the map: plane 1 of a single-plane format, a plane that does not exist
    m = np.zeros((H, W, 2), np.float32)

    def cmap(fmt, plane, out=m.ctypes.data, prm=None):
        return lib.rssync_color_map(p._h, fmt, plane, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, None,
                                    C.byref(prm_with() if prm is None else prm), out)

    for fmt, plane in ((color.GRAY8, 1), (color.RGBA32, 1), (color.NV12, 2), (color.I420, -1)):
        assert cmap(fmt, plane) != 0
        assert "plane" in lib.rssync_last_error().decode()
    assert cmap(color.NV12, 1, out=None) != 0
    assert cmap(7, 0) != 0 and "format" in lib.rssync_last_error().decode()
    assert cmap(color.NV12, 1, prm=prm_with(site=3)) != 0
    assert cmap(color.NV12, 1) == 0, lib.rssync_last_error().decode()
    with pytest.raises(rssync_amd.RsSyncError, match="even"):
        p.stabilize_color(color.NV12, (y, uv), times, lens, synth.D_TRUE, out_size=(W - 1, H))
    with pytest.raises(ValueError):
        p.stabilize_color(color.NV12, (y, u), times, lens, synth.D_TRUE)
    # ... and the calls that follow work
    out_y[:], out_uv[:] = 0, 0
    assert call() == 0, lib.rssync_last_error().decode()
    np.testing.assert_array_equal(out_y, want_y)
    np.testing.assert_array_equal(out_uv, want_uv)
    (again_y, again_uv), again_n = p.stabilize_color(color.NV12, (y, uv), times, lens, synth.D_TRUE, sigma=sr.SIGMA)
    np.testing.assert_array_equal(again_y, want_y)
    np.testing.assert_array_equal(again_uv, want_uv)
    np.testing.assert_array_equal(again_n, want_n)
