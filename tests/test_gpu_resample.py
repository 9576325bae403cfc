"""The bicubic sampler on the device (filter=FILTER_BICUBIC: include/rssync_stabilize.h "Sampling", csrc/kernels/resample.hpp)
against its numpy restatement (tests/resample_reference.py) on the device's own maps, byte for byte, in every format; the
bilinear default untouched by the new field; identity, truth, buffers, batching and the errors of a bad filter."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color16_reference as c16
import color_reference as cr
import rectify_reference as rr
import resample_reference as q
import stabilize_reference as sr

pytestmark = pytest.mark.gpu

SMALL = (37, 29)       # rows, cols: smaller than one 64 x 4 tile
ODD = (331, 197)       # no multiple of the tile
CROWS, CCOLS = 38, 68  # the colour cases' chroma plane: luma 76 x 136, two tiles wide, no multiple of the tile's height
ROWS, COLS = 2 * CROWS, 2 * CCOLS
N = 2
SITES = [cr.CENTER, cr.LEFT]
CAMERAS = [sr.LENS, sr.PINHOLE]
BILINEAR, BICUBIC = 0, 1


def _problem(gyro=None):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    if gyro is not None:
        p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def scene(built):
    s = dict(rr.scene())
    s["problem"] = _problem(s["gyro"])
    return s


@pytest.fixture(scope="module")
def colour(scene):
    """N frames of the colour scene cut to 76 x 136 luma (its upper left corner: a picture, not noise), the lens of that
    size, and the planes in every layout; 16-bit: full-range noise with patches of both extremes (read-only)"""
    col = cr.scene()
    y = np.ascontiguousarray(col["y"][:N, :ROWS, :COLS])
    u = np.ascontiguousarray(col["u"][:N, :CROWS, :CCOLS])
    v = np.ascontiguousarray(col["v"][:N, :CROWS, :CCOLS])
    d = dict(lens=rr.scaled_lens(ROWS, COLS), y=y, u=u, v=v, uv=np.stack([u, v], axis=-1),
             rgba=np.stack([y, y[:, ::-1], y[:, :, ::-1], np.random.default_rng(3).integers(0, 256, y.shape, dtype=np.uint8)], axis=-1))
    for depth in (10, 16):
        rng, top = np.random.default_rng(depth), (1 << depth) - 1
        wy = rng.integers(0, top + 1, size=(N, ROWS, COLS), dtype=np.uint16)
        wu, wv = (rng.integers(0, top + 1, size=(N, CROWS, CCOLS), dtype=np.uint16) for _ in range(2))
        for a, s in ((wy, 2), (wu, 1), (wv, 1)):
            a[:, 5 * s:12 * s, 8 * s:20 * s] = 0
            a[:, 5 * s:12 * s, 20 * s:30 * s] = top          # (beside the zeros: an edge that overshoots at both ends)
            a[:, 20 * s:30 * s, 30 * s:50 * s] = top
            a[:, :2 * s, :] = top                            # (the first rows and the last columns: the clamped taps)
            a[:, :, -2 * s:] = 0
        d[depth] = (wy, wu, wv)
    for a in [d[k] for k in ("y", "u", "v", "uv", "rgba")] + list(d[10]) + list(d[16]):
        a.setflags(write=False)
    return d


def _noise(n=2, seed=11, rows=rr.ROWS, cols=rr.COLS):
    return np.random.default_rng(seed).integers(0, 256, size=(n, rows, cols), dtype=np.uint8)


def _uv(u, v):
    return np.stack([u, v], axis=-1)


def _colour_inputs(color, d):
    """format -> the frames argument of stabilize_color, every format of the library"""
    y10, u10, v10 = d[10]
    y16, u16, v16 = d[16]
    return {color.GRAY8: d["y"], color.NV12: (d["y"], d["uv"]), color.I420: (d["y"], d["u"], d["v"]), color.RGBA32: d["rgba"],
            color.GRAY16: y16, color.P010: (y10 << 6, _uv(u10, v10) << 6), color.P016: (y16, _uv(u16, v16)), color.I010: (y10, u10, v10)}


def _planes(res):
    return [res] if isinstance(res, np.ndarray) else list(res)


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_explicit_bilinear_is_the_default_byte_for_byte(scene, colour):
    from rssync_amd import color, synth
    p, times = scene["problem"], scene["times"]
    kw = dict(sigma=sr.SIGMA, zoom=0.9, fill=9)
    want, want_n = p.stabilize_frames(scene["frames"], times, scene["lens"], synth.D_TRUE, **kw)
    got, got_n = p.stabilize_frames(scene["frames"], times, scene["lens"], synth.D_TRUE, filter=BILINEAR, **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_n, want_n)
    assert want_n.sum() > 0
    for fmt, frames in _colour_inputs(color, colour).items():
        for camera in CAMERAS:
            ckw = dict(sigma=sr.SIGMA, zoom=0.9, camera=camera)
            want, want_n = p.stabilize_color(fmt, frames, times[:N], colour["lens"], synth.D_TRUE, **ckw)
            got, got_n = p.stabilize_color(fmt, frames, times[:N], colour["lens"], synth.D_TRUE, filter=BILINEAR, **ckw)
            for a, b in zip(_planes(got), _planes(want)):
                np.testing.assert_array_equal(a, b, err_msg="format %d camera %d" % (fmt, camera))
            np.testing.assert_array_equal(got_n, want_n)
            cub, cub_n = p.stabilize_color(fmt, frames, times[:N], colour["lens"], synth.D_TRUE, filter=BICUBIC, **ckw)
            np.testing.assert_array_equal(cub_n, want_n)                       # the counts do not depend on the filter
            assert any((a != b).any() for a, b in zip(_planes(cub), _planes(want))), fmt      # ... the pixels do


# 2, 3 ------------------------------------------------------------------------------------------------------------------
GRAY_CASES = [(sr.LENS, None, 1.0), (sr.LENS, (320, 200), 1.1), (sr.PINHOLE, None, 1.1), (sr.PINHOLE, (320, 200), 1.0)]


@pytest.mark.parametrize("camera,out_size,zoom", GRAY_CASES)
def test_gray_is_the_restatement_on_the_devices_own_map(scene, camera, out_size, zoom):
    """pitched input, pitched output whose padding stays, fill 77; the map and the counts are the bilinear call's"""
    from rssync_amd import synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    ocols, orows = (rr.COLS, rr.ROWS) if out_size is None else out_size
    kw = dict(sigma=sr.SIGMA, camera=camera, out_size=out_size, zoom=zoom)
    wide = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS + 45), np.uint8)
    wide[:, :, 7:7 + rr.COLS] = frames
    dst = np.full((rr.N_FRAMES, orows + 3, ocols + 21), 201, np.uint8)
    view = dst[:, 1:1 + orows, 5:5 + ocols]
    got, got_n = p.stabilize_frames(wide[:, :, 7:7 + rr.COLS], times, lens, synth.D_TRUE, fill=77, out=view, filter=BICUBIC, **kw)
    assert got is view
    _, lin_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, fill=77, **kw)
    np.testing.assert_array_equal(got_n, lin_n)
    for k in range(rr.N_FRAMES):
        m = p.stabilize_map(rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, filter=BICUBIC, **kw)
        np.testing.assert_array_equal(m.view(np.uint32), p.stabilize_map(rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw).view(np.uint32))
        want, want_n = q.sample_bicubic(frames[k], m, fill=77)
        np.testing.assert_array_equal(view[k], want, err_msg="frame %d" % k)
        assert int(got_n[k]) == want_n
    pad = np.ones(dst.shape, bool)
    pad[:, 1:1 + orows, 5:5 + ocols] = False
    assert (dst[pad] == 201).all()


@pytest.mark.parametrize("rows,cols", [SMALL, ODD, (rr.ROWS, rr.COLS)])
@pytest.mark.parametrize("camera", CAMERAS)
def test_gray_noise_is_the_restatement_at_every_size(scene, rows, cols, camera):
    """noise: the clamp works at both ends, and the restatement says so"""
    from rssync_amd import synth
    p, times = scene["problem"], scene["times"][:2]
    lens, frames = rr.scaled_lens(rows, cols), _noise(2, 11, rows, cols)
    kw = dict(sigma=sr.SIGMA, camera=camera, zoom=0.9)
    got, got_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, fill=3, filter=BICUBIC, **kw)
    low = high = 0
    for k in range(2):
        m = p.stabilize_map(cols, rows, lens, times[k], synth.D_TRUE, **kw)
        cl = {}
        want, want_n = q.sample_bicubic(frames[k], m, fill=3, clamped=cl)
        np.testing.assert_array_equal(got[k], want, err_msg="frame %d" % k)
        assert int(got_n[k]) == want_n
        low, high = low + cl["low"], high + cl["high"]
    assert low > 0 and high > 0 and got_n.sum() > 0


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_a_camera_at_rest_and_the_frames_own_orientation_are_the_identity(scene):
    from rssync_amd import synth
    g = scene["gyro"]
    quats = np.zeros_like(g.quats)
    quats[:, 0] = 1.0
    p = _problem()
    p.SetGyroQuaternions(quats, g.fs, g.t0)
    frames = _noise()
    out, _ = p.stabilize_frames(frames, scene["times"][:2], scene["lens"], synth.D_TRUE, sigma=0.2, filter=BICUBIC)
    np.testing.assert_array_equal(out[:, 1:-1, 1:-1], frames[:, 1:-1, 1:-1])
    lens = (0.0,) + tuple(scene["lens"][1:])
    targets = g.orientation(scene["times"][:2] + synth.D_TRUE)
    out, _ = scene["problem"].stabilize_frames(frames, scene["times"][:2], lens, synth.D_TRUE, targets=targets, filter=BICUBIC)
    np.testing.assert_array_equal(out[:, 1:-1, 1:-1], frames[:, 1:-1, 1:-1])


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_colour_planes_are_the_gray_stabiliser_with_that_planes_camera(scene, colour, site, camera):
    """explicit targets, as in the bilinear colour tests: Y is stabilize_frames of Y, U and V of those planes with the chroma
    lens, frame time and output camera; NV12 and I420 agree; RGBA32's channel k is the gray result of channel k"""
    from rssync_amd import color, synth
    p, times, d = scene["problem"], scene["times"][:N], colour
    targets = 2.5 * sr.path64(scene["gyro"], times, scene["lens"][0], synth.D_TRUE, 0.3)
    lens_c = cr.chroma_lens(d["lens"], site)
    times_c = np.array([cr.chroma_time(t, d["lens"], ROWS, site) for t in times])
    for (out_size, orows, ocols), zoom in (((None, ROWS, COLS), 0.8), (((100, 60), 60, 100), 1.0)):
        cam_c = cr.chroma_camera(d["lens"], ROWS, COLS, orows, ocols, site, zoom)
        kw = dict(camera=camera, targets=targets, filter=BICUBIC)
        ckw = dict(out_size=(ocols // 2, orows // 2), out_camera=cam_c, **kw)
        ykw = dict(out_size=out_size, zoom=zoom, **kw)
        (y1, uv), n1 = p.stabilize_color(color.NV12, (d["y"], d["uv"]), times, d["lens"], synth.D_TRUE, chroma_site=site, fills=(4, 55, 66), **ykw)
        (y2, u, v), n2 = p.stabilize_color(color.I420, (d["y"], d["u"], d["v"]), times, d["lens"], synth.D_TRUE, chroma_site=site,
                                           fills=(4, 55, 66), **ykw)
        want_y, want_ny = p.stabilize_frames(d["y"], times, d["lens"], synth.D_TRUE, fill=4, **ykw)
        want_u, want_nc = p.stabilize_frames(d["u"], times_c, lens_c, synth.D_TRUE, fill=55, **ckw)
        want_v, _ = p.stabilize_frames(d["v"], times_c, lens_c, synth.D_TRUE, fill=66, **ckw)
        np.testing.assert_array_equal(y1, want_y)
        np.testing.assert_array_equal(y2, want_y)
        np.testing.assert_array_equal(u, want_u)
        np.testing.assert_array_equal(v, want_v)
        np.testing.assert_array_equal(uv, _uv(u, v))
        np.testing.assert_array_equal(n1, n2)
        np.testing.assert_array_equal(n1[:, 0], want_ny)
        np.testing.assert_array_equal(n1[:, 1], want_nc)
        if zoom < 1:
            assert n1[:, 0].sum() > 0 and n1[:, 1].sum() > 0
        fills = (7, 99, 200, 31)
        rgba, n4 = p.stabilize_color(color.RGBA32, d["rgba"], times, d["lens"], synth.D_TRUE, fills=fills, **ykw)
        for k in range(4):
            want, want_n = p.stabilize_frames(d["rgba"][..., k], times, d["lens"], synth.D_TRUE, fill=fills[k], **ykw)
            np.testing.assert_array_equal(rgba[..., k], want, err_msg="channel %d" % k)
            np.testing.assert_array_equal(n4[:, 0], want_n)
        g8, n8 = p.stabilize_color(color.GRAY8, d["y"], times, d["lens"], synth.D_TRUE, fills=(4,), **ykw)
        np.testing.assert_array_equal(g8, want_y)
        np.testing.assert_array_equal(n8[:, 0], want_ny)


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_16_bit_formats_are_the_restatement_with_the_formats_range(scene, colour, site, camera):
    """full-range noise with edges between 0 and the maximum, on the device's own maps: every plane is the restatement's with
    vmax 1023 (P010, I010) or 65535 (GRAY16, P016); P010's low six bits are zero whatever the input's are"""
    from rssync_amd import color, synth
    p, times, lens = scene["problem"], scene["times"][:N], colour["lens"]
    fills = {10: (1001, 77, 888), 16: (60001, 777, 43210)}
    kw = dict(sigma=sr.SIGMA, camera=camera, chroma_site=site, zoom=0.8, filter=BICUBIC)
    maps = [(p.color_map(color.NV12, 0, COLS, ROWS, lens, t, synth.D_TRUE, **kw), p.color_map(color.NV12, 1, COLS, ROWS, lens, t, synth.D_TRUE, **kw))
            for t in times]
    rng = np.random.default_rng(1)
    for fmt, depth in ((color.P010, 10), (color.I010, 10), (color.P016, 16), (color.GRAY16, 16)):
        y, u, v = colour[depth]
        fl = fills[depth]
        stored = c16.pack(fmt, (y, u, v))
        sy, su, sv = stored
        if fmt == color.P010:
            junk = [rng.integers(0, 64, a.shape, dtype=np.uint16) for a in stored]
            frames, dirty = (sy, _uv(su, sv)), (sy | junk[0], _uv(su | junk[1], sv | junk[2]))
        elif fmt == color.P016:
            frames = (sy, _uv(su, sv))
        elif fmt == color.I010:
            frames = (sy, su, sv)
        else:
            frames = sy
        got, n_out = p.stabilize_color(fmt, frames, times, lens, synth.D_TRUE, fills=fl, **kw)
        got = _planes(got)
        clamps = {"low": 0, "high": 0}
        for k in range(N):
            cl = {}
            want, want_n = q.sample_bicubic16(fmt, sy[k], maps[k][0], fill=fl[0], clamped=cl)
            np.testing.assert_array_equal(got[0][k], want, err_msg="format %d frame %d luma" % (fmt, k))
            assert int(n_out[k, 0]) == want_n
            clamps = {e: clamps[e] + cl[e] for e in clamps}
            if fmt in (color.P010, color.P016):
                want, want_n = q.sample_bicubic_pairs16(fmt, _uv(su, sv)[k], maps[k][1], fill=fl[1:])
                np.testing.assert_array_equal(got[1][k], want, err_msg="format %d frame %d UV" % (fmt, k))
                assert int(n_out[k, 1]) == want_n
            elif fmt == color.I010:
                for plane, src, f in ((1, su, fl[1]), (2, sv, fl[2])):
                    want, want_n = q.sample_bicubic16(fmt, src[k], maps[k][1], fill=f)
                    np.testing.assert_array_equal(got[plane][k], want, err_msg="format %d frame %d plane %d" % (fmt, k, plane))
                    assert int(n_out[k, 1]) == want_n
        assert clamps["low"] > 0 and clamps["high"] > 0, (fmt, clamps)         # the restatement clamps at both ends
        assert n_out.sum() > 0
        assert max(int(a.max()) for a in got) <= ((1 << depth) - 1) << c16.SHIFT[fmt]
        if fmt == color.P010:
            assert all((a & 63 == 0).all() for a in got)
            again, n_again = p.stabilize_color(fmt, dirty, times, lens, synth.D_TRUE, fills=fl, **kw)
            for a, b in zip(again, got):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(n_again, n_out)


def test_8_bit_values_widened_give_the_8_bit_result_widened(scene, colour):
    """values confined to 48 .. 207: the two-dimensional kernel overshoots by at most 0.28125 of the taps' range (159), so
    nothing reaches 0 or 255, and the 16-bit formats, whose clamps lie higher still, compute the 8-bit numbers"""
    from rssync_amd import color, synth
    p, times, lens = scene["problem"], scene["times"][:N], colour["lens"]
    rng = np.random.default_rng(8)
    y = rng.integers(48, 208, size=(N, ROWS, COLS), dtype=np.uint8)
    u, v = (rng.integers(48, 208, size=(N, CROWS, CCOLS), dtype=np.uint8) for _ in range(2))
    yw, uw, vw = (a.astype(np.uint16) for a in (y, u, v))
    for camera in CAMERAS:
        kw = dict(sigma=sr.SIGMA, camera=camera, zoom=0.8, fills=(1, 2, 3), filter=BICUBIC)
        args = (times, lens, synth.D_TRUE)
        (y8, uv8), n8 = p.stabilize_color(color.NV12, (y, _uv(u, v)), *args, **kw)
        (yi8, u8, v8), ni8 = p.stabilize_color(color.I420, (y, u, v), *args, **kw)
        g8, ng8 = p.stabilize_color(color.GRAY8, y, *args, **dict(kw, fills=(9,)))
        assert 0 < y8.min() and y8.max() < 255 and (y8 > 207).any() and (y8 < 48).any()   # it overshoots, and clamps nowhere
        (y16, uv16), n16 = p.stabilize_color(color.P016, (yw, _uv(uw, vw)), *args, **kw)
        (y10, uv10), n10 = p.stabilize_color(color.P010, (yw << 6, _uv(uw, vw) << 6), *args, **kw)
        (yi, ui, vi), ni = p.stabilize_color(color.I010, (yw, uw, vw), *args, **kw)
        g16, ng16 = p.stabilize_color(color.GRAY16, yw, *args, **dict(kw, fills=(9,)))
        np.testing.assert_array_equal(y16, y8.astype(np.uint16))
        np.testing.assert_array_equal(uv16, uv8.astype(np.uint16))
        np.testing.assert_array_equal(y10, y8.astype(np.uint16) << 6)
        np.testing.assert_array_equal(uv10, uv8.astype(np.uint16) << 6)
        np.testing.assert_array_equal(yi, yi8.astype(np.uint16))
        np.testing.assert_array_equal(ui, u8.astype(np.uint16))
        np.testing.assert_array_equal(vi, v8.astype(np.uint16))
        np.testing.assert_array_equal(g16, g8.astype(np.uint16))
        for a, b in ((n16, n8), (n10, n8), (ni, ni8), (ng16, ng8)):
            np.testing.assert_array_equal(a, b)


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stabilised(scene):
    """the scene's three frames along the path at sigma 0.1, bicubic, with the device's maps (read-only)"""
    from rssync_amd import synth
    p = scene["problem"]
    out, n_out = p.stabilize_frames(scene["frames"], scene["times"], scene["lens"], synth.D_TRUE, sigma=sr.SIGMA, filter=BICUBIC)
    maps = [p.stabilize_map(rr.COLS, rr.ROWS, scene["lens"], t, synth.D_TRUE, sigma=sr.SIGMA) for t in scene["times"]]
    for a in [out, n_out] + maps:
        a.setflags(write=False)
    return out, n_out, maps


def test_error_against_the_global_shutter_truth(scene, stabilised):
    """the margin over the restatement's error is the one tests/test_gpu_stabilize.py gives the device's map over the
    reference's; the figure itself is no better than bilinear's (resample_reference.BICUBIC_ERROR)"""
    out, n_out, maps = stabilised
    frames, truth, ref_maps = scene["frames"], sr.truth(), sr.reference_maps()
    for k in range(rr.N_FRAMES):
        ok = rr.inside(maps[k])
        err = rr.grey_error(out[k], truth[k], ok)
        ref_img, _ = q.sample_bicubic(frames[k], ref_maps[k])
        both = ok & rr.inside(ref_maps[k])
        worst = np.abs(out[k].astype(int) - ref_img.astype(int))[both].max()
        print("frame %d: device %.4f restatement %.4f; device against the restatement on the reference map: %d grey levels" %
              (rr.F0 + k, err, q.BICUBIC_ERROR[k], worst))
        assert err <= 1.05 * q.BICUBIC_ERROR[k], (k, err)
        assert worst <= 1, (k, worst)


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_buffers_batches_and_chunks_agree(scene, stabilised):
    from rssync_amd import stabilize, synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    want, want_n, _ = stabilised
    kw = dict(sigma=sr.SIGMA, filter=BICUBIC)
    wide = np.zeros((rr.N_FRAMES, rr.ROWS, rr.COLS + 61), np.uint8)
    wide[:, :, 13:13 + rr.COLS] = frames
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")
    dwide = torch.from_numpy(wide).to("cuda:0")
    for src in (wide[:, :, 13:13 + rr.COLS], dev, dwide[:, :, 13:13 + rr.COLS]):
        got, n = p.stabilize_frames(src, times, lens, synth.D_TRUE, **kw)
        assert isinstance(got, torch.Tensor) == isinstance(src, torch.Tensor)
        np.testing.assert_array_equal(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
        np.testing.assert_array_equal(n, want_n)
    dout = torch.full((rr.N_FRAMES, rr.ROWS, rr.COLS + 19), 9, dtype=torch.uint8, device="cuda:0")
    p.stabilize_frames(frames, times, lens, synth.D_TRUE, out=dout[:, :, 3:3 + rr.COLS], **kw)
    back = dout.cpu().numpy()
    np.testing.assert_array_equal(back[:, :, 3:3 + rr.COLS], want)
    assert (back[:, :, :3] == 9).all() and (back[:, :, 3 + rr.COLS:] == 9).all()
    # a batch is its frames one at a time
    for k in range(rr.N_FRAMES):
        got, n = p.stabilize_frames(frames[k:k + 1], times[k:k + 1], lens, synth.D_TRUE, **kw)
        np.testing.assert_array_equal(got[0], want[k])
        assert n[0] == want_n[k]
    # a budget of one and a half frames per slot: three chunks through both slots
    per_frame = (rr.ROWS + 1) * 36 + 2 * rr.ROWS * rr.COLS
    got, got_n = stabilize.stabilize_frames_budget(p, frames, times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_n, want_n)


def test_colour_chunks_agree(scene, colour):
    from rssync_amd import color, synth
    p, lens = scene["problem"], colour["lens"]
    n = rr.N_FRAMES
    y, u, v = (np.concatenate([colour[k], colour[k][:1]]) for k in ("y", "u", "v"))
    times = scene["times"]
    for fmt, frames, depth in ((color.NV12, (y, _uv(u, v)), 8), (color.I010, tuple(a.astype(np.uint16) << 2 for a in (y, u, v)), 10)):
        one, one_n = p.stabilize_color(fmt, frames, times, lens, synth.D_TRUE, sigma=sr.SIGMA, filter=BICUBIC)
        b = depth // 8 if depth == 8 else 2
        per_frame = (ROWS + 1) * 36 + (CROWS + 1) * 36 + 2 * b * (ROWS * COLS * 3 // 2)
        got, got_n = color.stabilize_color_budget(p, fmt, frames, times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, sigma=sr.SIGMA, filter=BICUBIC)
        for a, w in zip(got, one):
            np.testing.assert_array_equal(a, w)
        np.testing.assert_array_equal(got_n, one_n)
        lin, _ = color.stabilize_color_budget(p, fmt, frames, times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, sigma=sr.SIGMA)
        assert (lin[0] != got[0]).any()
    assert n == 3


# 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [2, -1])
def test_a_filter_outside_the_enum_is_an_error_that_names_it(scene, colour, stabilised, bad):
    import rssync_amd
    from rssync_amd import color, stabilize, synth
    p, frames, times, lens = scene["problem"], scene["frames"], scene["times"], scene["lens"]
    stabilize.library().rssync_set_panic_mode(1)
    y16 = colour[16][0]
    calls = [
        lambda f: p.stabilize_frames(frames, times, lens, synth.D_TRUE, sigma=sr.SIGMA, filter=f),
        lambda f: p.stabilize_map(rr.COLS, rr.ROWS, lens, times[0], synth.D_TRUE, sigma=sr.SIGMA, filter=f),
        lambda f: p.stabilize_coverage(rr.COLS, rr.ROWS, lens, times, synth.D_TRUE, (1.0, 1.1), sigma=sr.SIGMA, filter=f),
        lambda f: p.stabilize_color(color.NV12, (colour["y"], colour["uv"]), times[:N], colour["lens"], synth.D_TRUE, sigma=sr.SIGMA, filter=f),
        lambda f: p.color_map(color.NV12, 1, COLS, ROWS, colour["lens"], times[0], synth.D_TRUE, sigma=sr.SIGMA, filter=f),
        lambda f: p.stabilize_color(color.GRAY16, y16, times[:N], colour["lens"], synth.D_TRUE, sigma=sr.SIGMA, filter=f),
    ]
    results = []
    for fn in calls:
        with pytest.raises(rssync_amd.RsSyncError, match="filter"):
            fn(bad)
        results.append(fn(BICUBIC))               # the next valid call works
    np.testing.assert_array_equal(results[0][0], stabilised[0])
    np.testing.assert_array_equal(results[1], stabilised[2][0])
    np.testing.assert_array_equal(results[2], p.stabilize_coverage(rr.COLS, rr.ROWS, lens, times, synth.D_TRUE, (1.0, 1.1), sigma=sr.SIGMA))
