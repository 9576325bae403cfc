"""The 16-bit colour front on the device (include/rssync_color16.h, csrc/kernels/color16.hpp): GRAY16, P010, P016 and I010
against the 8-bit path they widen -- the same map, so on 8-bit values the same numbers --, against the numpy restatement
of the sample (tests/color16_reference.py) on the device's own maps over the full range of 10 and 16 bits, and P010's
container, the default fills, the memory kinds and the errors of the new entry point."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color16_reference as c16
import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr

pytestmark = pytest.mark.gpu

# luma (rows, cols) as in tests/test_gpu_color.py: a 2 x 2 chroma plane with clamped taps, one under a tile of chroma samples,
# an odd chroma size that is no multiple of the tile, the scene's; and the output of another size
SIZES = [(4, 4), (38, 30), (330, 198), (rr.ROWS, rr.COLS)]
OUT = (200, 320)
SITES = [cr.CENTER, cr.LEFT]
CAMERAS = [sr.LENS, sr.PINHOLE]
N = 2


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
    """per luma size: lens and N frames of 8-bit Y, U, V -- the scene's planes at its size, noise elsewhere (read-only)"""
    out = {}
    col = cr.scene()
    for rows, cols in SIZES:
        rng = np.random.default_rng(rows * 1000 + cols)
        if (rows, cols) == (rr.ROWS, rr.COLS):
            y, u, v = (np.array(col[k][:N]) for k in ("y", "u", "v"))
        else:
            y = rng.integers(0, 256, size=(N, rows, cols), dtype=np.uint8)
            u, v = (rng.integers(0, 256, size=(N, rows // 2, cols // 2), dtype=np.uint8) for _ in range(2))
        d = dict(lens=rr.scaled_lens(rows, cols), y=y, u=u, v=v, uv=np.stack([u, v], axis=-1))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(rows, cols)] = d
    return out


@pytest.fixture(scope="module")
def wide_planes():
    """three frames of the scene's size with random samples of 10 and of 16 bits and patches of 0 and of the maximum
    (read-only): {depth: (y, u, v)}"""
    out = {}
    for depth in (10, 16):
        rng = np.random.default_rng(depth)
        top = (1 << depth) - 1
        y = rng.integers(0, top + 1, size=(rr.N_FRAMES, rr.ROWS, rr.COLS), dtype=np.uint16)
        u, v = (rng.integers(0, top + 1, size=(rr.N_FRAMES, cr.C_ROWS, cr.C_COLS), dtype=np.uint16) for _ in range(2))
        for a, s in ((y, 2), (u, 1), (v, 1)):
            a[:, 40 * s:70 * s, 50 * s:120 * s] = 0
            a[:, 90 * s:130 * s, 100 * s:250 * s] = top
            a[:, 60 * s:100 * s, 180 * s:200 * s] = top          # (beside the zeros: taps of both extremes)
            a[:, :3 * s, :] = top                                # (the first rows and the last columns: the clamped taps)
            a[:, :, -3 * s:] = 0
            a.setflags(write=False)
        out[depth] = (y, u, v)
    return out


def _outs(rows, cols):
    """(out_size argument (cols, rows), out rows, out cols): the input's size and OUT"""
    return [(None, rows, cols), ((OUT[1], OUT[0]), OUT[0], OUT[1])]


def _targets(scene, n):
    from rssync_amd import synth
    return 2.5 * sr.path64(scene["gyro"], scene["times"][:n], scene["lens"][0], synth.D_TRUE, 0.3)


def _uv(u, v):
    return np.stack([u, v], axis=-1)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("size", SIZES)
def test_on_8_bit_values_every_format_is_its_8_bit_sibling_widened(scene, planes, size, camera):
    """the anchor: the widened scene through each 16-bit format gives the sibling's bytes widened (P010, fed << 6, gives them
    << 6) and the sibling's counts, with the same fills, along the path"""
    from rssync_amd import color, synth
    p, times, d = scene["problem"], scene["times"][:N], planes[size]
    y, u, v, uv = (d[k].astype(np.uint16) for k in ("y", "u", "v", "uv"))
    for site in SITES:
        for (out_size, orows, ocols), zoom in zip(_outs(*size), (1.0, 0.8)):
            kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, zoom=zoom, chroma_site=site)
            args = (times, d["lens"], synth.D_TRUE)
            (y8, uv8), n8 = p.stabilize_color(color.NV12, (d["y"], d["uv"]), *args, fills=(1, 2, 3), **kw)
            (yi8, u8, v8), ni8 = p.stabilize_color(color.I420, (d["y"], d["u"], d["v"]), *args, fills=(1, 2, 3), **kw)
            g8, ng8 = p.stabilize_color(color.GRAY8, d["y"], *args, fills=(9,), **kw)
            (y16, uv16), n16 = p.stabilize_color(color.P016, (y, uv), *args, fills=(1, 2, 3), **kw)
            (y10, uv10), n10 = p.stabilize_color(color.P010, (y << 6, uv << 6), *args, fills=(1, 2, 3), **kw)
            (yi, ui, vi), ni = p.stabilize_color(color.I010, (y, u, v), *args, fills=(1, 2, 3), **kw)
            g16, ng16 = p.stabilize_color(color.GRAY16, y, *args, fills=(9,), **kw)
            for a in (y16, uv16, y10, uv10, yi, ui, vi, g16):
                assert a.dtype == np.uint16
            assert y16.shape == (N, orows, ocols) and uv16.shape == (N, orows // 2, ocols // 2, 2) and ui.shape == (N, orows // 2, ocols // 2)
            np.testing.assert_array_equal(y16, y8.astype(np.uint16))
            np.testing.assert_array_equal(uv16, uv8.astype(np.uint16))
            np.testing.assert_array_equal(y10, y8.astype(np.uint16) << 6)
            np.testing.assert_array_equal(uv10, uv8.astype(np.uint16) << 6)
            np.testing.assert_array_equal(yi, yi8.astype(np.uint16))
            np.testing.assert_array_equal(ui, u8.astype(np.uint16))
            np.testing.assert_array_equal(vi, v8.astype(np.uint16))
            np.testing.assert_array_equal(g16, g8.astype(np.uint16))
            np.testing.assert_array_equal(n16, n8)
            np.testing.assert_array_equal(n10, n8)
            np.testing.assert_array_equal(ni, ni8)
            np.testing.assert_array_equal(ng16, ng8)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_full_range_against_the_restatement_on_the_devices_own_map(scene, wide_planes, site, camera):
    """random 10- and 16-bit samples with patches of 0 and of the maximum: every output plane is sample16 / sample_pairs16
    applied to the device's color_map of the sibling format, and the counts are that map's.  Along the path at both output
    sizes, with targets given, and at zoom 0.8 so that the pinhole camera fills samples too; distinct fills per plane."""
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    targets = _targets(scene, rr.N_FRAMES)
    fills = {10: (1001, 77, 888), 16: (60001, 777, 43210)}
    some_outside = 0
    for (out_size, orows, ocols), zoom, tg in zip(_outs(rr.ROWS, rr.COLS) + _outs(rr.ROWS, rr.COLS)[:1], (1.0, 1.0, 0.8), (None, targets, None)):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, chroma_site=site, zoom=zoom)
        got = {}
        for fmt, depth in ((color.P010, 10), (color.I010, 10), (color.P016, 16), (color.GRAY16, 16)):
            y, u, v = wide_planes[depth]
            frames = {color.P010: (y << 6, _uv(u, v) << 6), color.I010: (y, u, v), color.P016: (y, _uv(u, v)), color.GRAY16: y}[fmt]
            f = fills[depth][:1] if fmt == color.GRAY16 else fills[depth]
            res, n_out = p.stabilize_color(fmt, frames, times, lens, synth.D_TRUE, targets=tg, fills=f, **kw)
            got[fmt] = ((res,) if fmt == color.GRAY16 else res, n_out)
        for k in range(rr.N_FRAMES):
            mkw = dict(kw, target=None if tg is None else tg[k])
            m0 = p.color_map(color.NV12, 0, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **mkw)
            m1 = p.color_map(color.NV12, 1, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **mkw)
            n0, n1 = int((~sr.inside(m0, rr.ROWS, rr.COLS)).sum()), int((~sr.inside(m1, cr.C_ROWS, cr.C_COLS)).sum())
            some_outside += n0 + n1
            for depth, fmts in ((10, (color.P010, color.I010)), (16, (color.P016, color.GRAY16))):
                y, u, v = wide_planes[depth]
                fy, fu, fv = fills[depth]
                want_y, cnt_y = c16.sample16(y[k], m0, fy)
                want_uv, cnt_uv = c16.sample_pairs16(_uv(u[k], v[k]), m1, (fu, fv))
                assert cnt_y == n0 and cnt_uv == n1
                for fmt in fmts:
                    res, n_out = got[fmt]
                    name = "format %d frame %d out %s zoom %.1f" % (fmt, k, out_size, zoom)
                    values = c16.unpack(fmt, [a[k] for a in res])
                    np.testing.assert_array_equal(values[0], want_y, err_msg=name)
                    assert int(n_out[k, 0]) == n0, name
                    if fmt == color.GRAY16:
                        assert int(n_out[k, 1]) == 0
                        continue
                    uv = values[1] if fmt != color.I010 else _uv(values[1], values[2])
                    np.testing.assert_array_equal(uv, want_uv, err_msg=name)
                    assert int(n_out[k, 1]) == n1, name
    assert some_outside > 0


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
def test_p010_keeps_its_values_in_the_ten_high_bits(scene, camera):
    """the low six bits of the input are ignored, those of the output are zero (in filled samples too), and P010 of x << 6 is
    P016 of x and I010 of x, shifted left by 6"""
    from rssync_amd import color, synth
    p, times = scene["problem"], scene["times"][:N]
    rows, cols = 330, 198
    rng = np.random.default_rng(10)
    lens = rr.scaled_lens(rows, cols)
    y = rng.integers(0, 1024, size=(N, rows, cols), dtype=np.uint16)
    u, v = (rng.integers(0, 1024, size=(N, rows // 2, cols // 2), dtype=np.uint16) for _ in range(2))
    uv = _uv(u, v)
    for (out_size, _, _), zoom in zip(_outs(rows, cols), (0.8, 1.0)):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, zoom=zoom, fills=(1023, 5, 700))
        (y10, uv10), n10 = p.stabilize_color(color.P010, (y << 6, uv << 6), times, lens, synth.D_TRUE, **kw)
        noise = (rng.integers(0, 64, size=y.shape, dtype=np.uint16), rng.integers(0, 64, size=uv.shape, dtype=np.uint16))
        (yn, uvn), nn = p.stabilize_color(color.P010, ((y << 6) | noise[0], (uv << 6) | noise[1]), times, lens, synth.D_TRUE, **kw)
        np.testing.assert_array_equal(yn, y10)
        np.testing.assert_array_equal(uvn, uv10)
        np.testing.assert_array_equal(nn, n10)
        assert not (y10 & 63).any() and not (uv10 & 63).any()
        if zoom < 1:
            assert n10[:, 0].min() > 0 and n10[:, 1].min() > 0 and (y10 == 1023 << 6).any() and (uv10[..., 1] == 700 << 6).any()
        (y16, uv16), n16 = p.stabilize_color(color.P016, (y, uv), times, lens, synth.D_TRUE, **kw)
        (yi, ui, vi), ni = p.stabilize_color(color.I010, (y, u, v), times, lens, synth.D_TRUE, **kw)
        np.testing.assert_array_equal(y10, y16 << 6)
        np.testing.assert_array_equal(uv10, uv16 << 6)
        np.testing.assert_array_equal(y10, yi << 6)
        np.testing.assert_array_equal(uv10, _uv(ui, vi) << 6)
        np.testing.assert_array_equal(n10, n16)
        np.testing.assert_array_equal(n10, ni)


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_default_fills_follow_the_depth(scene):
    """fill_set = 0 and stab.fill = 200: filled samples are 200 << 2, 512, 512 with ten bits (P010's << 6 as stored) and
    200 << 8, 32768, 32768 with sixteen"""
    from rssync_amd import color, synth
    p, times = scene["problem"], scene["times"][:N]
    rows, cols = 38, 30
    lens = rr.scaled_lens(rows, cols)
    rng = np.random.default_rng(4)
    y = rng.integers(300, 700, size=(N, rows, cols), dtype=np.uint16)
    u, v = (rng.integers(300, 500, size=(N, rows // 2, cols // 2), dtype=np.uint16) for _ in range(2))
    kw = dict(sigma=sr.SIGMA, zoom=0.7, fill=200)
    out_y = np.stack([~sr.inside(p.color_map(color.NV12, 0, cols, rows, lens, t, synth.D_TRUE, sigma=sr.SIGMA, zoom=0.7), rows, cols) for t in times])
    out_c = np.stack([~sr.inside(p.color_map(color.NV12, 1, cols, rows, lens, t, synth.D_TRUE, sigma=sr.SIGMA, zoom=0.7), rows // 2, cols // 2)
                      for t in times])
    assert out_y.any() and out_c.any() and not out_y.all() and not out_c.all()
    (a, b), n = p.stabilize_color(color.P010, (y << 6, _uv(u, v) << 6), times, lens, synth.D_TRUE, **kw)
    assert (a[out_y] == (200 << 2) << 6).all() and (b[out_c] == 512 << 6).all() and (a[~out_y] != (200 << 2) << 6).all()
    assert n[:, 0].sum() == out_y.sum() and n[:, 1].sum() == out_c.sum()
    (a, b, c), _ = p.stabilize_color(color.I010, (y, u, v), times, lens, synth.D_TRUE, **kw)
    assert (a[out_y] == 200 << 2).all() and (b[out_c] == 512).all() and (c[out_c] == 512).all() and (a[~out_y] != 200 << 2).all()
    (a, b), _ = p.stabilize_color(color.P016, (y, _uv(u, v)), times, lens, synth.D_TRUE, **kw)
    assert (a[out_y] == 200 << 8).all() and (b[out_c] == 32768).all() and (a[~out_y] < 1024).all() and (b[~out_c] < 1024).all()
    a, _ = p.stabilize_color(color.GRAY16, y, times, lens, synth.D_TRUE, **kw)
    assert (a[out_y] == 200 << 8).all() and (a[~out_y] < 1024).all()


# 5 ---------------------------------------------------------------------------------------------------------------------
def _off_by_two(n, rows, cols, pad_rows, pad_cols, value, pairs):
    """-> (backing uint16 array, view of n x rows x cols (x 2) whose every row starts at an address = 2 (mod 4))"""
    per = 2 if pairs else 1
    width = per * (cols + pad_cols)
    width += width & 1                                                    # rows a multiple of 4 bytes apart
    back = np.full((n, rows + pad_rows, width), value, np.uint16)
    first = 1 if back.ctypes.data % 4 == 0 else 2                         # (an odd sample offset from a 4-byte aligned base)
    win = back[:, pad_rows:, first:first + per * cols]
    view = np.lib.stride_tricks.as_strided(win, shape=(n, rows, cols, 2), strides=win.strides[:2] + (4, 2)) if pairs else win
    assert view.ctypes.data % 4 == 2 and view.strides[1] % 4 == 0 and view.strides[0] % 4 == 0
    return back, view, (slice(None), slice(pad_rows, None), slice(first, first + per * cols))


def test_chunks_pitched_views_and_device_tensors_do_not_change_the_result(scene, wide_planes):
    """P010 into the 200 x 320 output: pitched numpy views whose rows start at addresses = 2 (mod 4) in every plane, device
    tensors contiguous and pitched in both directions, and three frames as three chunks through both slots (a budget of one
    and a half frames per slot) all give the same bytes; the padding of `out` is not written"""
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    y10, u10, v10 = wide_planes[10]
    y, uv = y10 << 6, _uv(u10, v10) << 6
    NF = rr.N_FRAMES
    orows, ocols = OUT
    kw = dict(sigma=sr.SIGMA, out_size=(ocols, orows))
    (one_y, one_uv), one_n = p.stabilize_color(color.P010, (y, uv), times, lens, synth.D_TRUE, **kw)
    assert one_y.shape == (NF, orows, ocols) and one_uv.shape == (NF, orows // 2, ocols // 2, 2) and one_y.dtype == one_uv.dtype == np.uint16
    # chunks: a frame costs twice the 8-bit bytes
    per_frame = (rr.ROWS + 1) * 36 + (cr.C_ROWS + 1) * 36 + 2 * (rr.ROWS * rr.COLS * 3 // 2) + 2 * (orows * ocols * 3 // 2)
    (got_y, got_uv), got_n = color.stabilize_color_budget(p, color.P010, (y, uv), times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, **kw)
    np.testing.assert_array_equal(got_y, one_y)
    np.testing.assert_array_equal(got_uv, one_uv)
    np.testing.assert_array_equal(got_n, one_n)
    (iy, iu, iv), i_n = color.stabilize_color_budget(p, color.I010, (y10, u10, v10), times, lens, synth.D_TRUE, 2 * 1.5 * per_frame, **kw)
    np.testing.assert_array_equal(iy << 6, one_y)
    np.testing.assert_array_equal(_uv(iu, iv) << 6, one_uv)
    np.testing.assert_array_equal(i_n, one_n)
    # pitched views in, pitched views out, every row at an address = 2 (mod 4)
    _, src_y, _ = _off_by_two(NF, rr.ROWS, rr.COLS, 1, 45, 0, False)
    _, src_uv, _ = _off_by_two(NF, cr.C_ROWS, cr.C_COLS, 0, 9, 0, True)
    src_y[:], src_uv[:] = y, uv
    back_y, dst_y, where_y = _off_by_two(NF, orows, ocols, 2, 21, 0xabcd, False)
    back_uv, dst_uv, where_uv = _off_by_two(NF, orows // 2, ocols // 2, 1, 5, 0xdcba, True)
    res, n = p.stabilize_color(color.P010, (src_y, src_uv), times, lens, synth.D_TRUE, out=(dst_y, dst_uv), **kw)
    assert res[0] is dst_y and res[1] is dst_uv
    np.testing.assert_array_equal(dst_y, one_y)
    np.testing.assert_array_equal(dst_uv, one_uv)
    np.testing.assert_array_equal(n, one_n)
    pad_y, pad_uv = np.ones(back_y.shape, bool), np.ones(back_uv.shape, bool)
    pad_y[where_y] = False
    pad_uv[where_uv] = False
    assert (back_y[pad_y] == 0xabcd).all() and (back_uv[pad_uv] == 0xdcba).all()
    # device tensors: contiguous (uint16, and int16 with the same bits), then pitched in and out
    dev = (torch.from_numpy(np.array(y)).to("cuda:0"), torch.from_numpy(np.array(uv)).to("cuda:0"))
    (dy, duv), dn = p.stabilize_color(color.P010, dev, times, lens, synth.D_TRUE, **kw)
    assert isinstance(dy, torch.Tensor) and dy.dtype == torch.uint16 and duv.dtype == torch.uint16
    np.testing.assert_array_equal(dy.cpu().numpy(), one_y)
    np.testing.assert_array_equal(duv.cpu().numpy(), one_uv)
    np.testing.assert_array_equal(dn, one_n)
    (sy, suv), _ = p.stabilize_color(color.P010, tuple(t.view(torch.int16) for t in dev), times, lens, synth.D_TRUE, **kw)
    np.testing.assert_array_equal(sy.cpu().numpy(), one_y)
    np.testing.assert_array_equal(suv.cpu().numpy(), one_uv)
    wide_y = np.zeros((NF, rr.ROWS + 2, rr.COLS + 45), np.uint16)
    wide_y[:, 1:1 + rr.ROWS, 7:7 + rr.COLS] = y
    wide_uv = np.zeros((NF, cr.C_ROWS, cr.C_COLS + 9, 2), np.uint16)
    wide_uv[:, :, 4:4 + cr.C_COLS] = uv
    dwide = (torch.from_numpy(wide_y).to("cuda:0")[:, 1:1 + rr.ROWS, 7:7 + rr.COLS], torch.from_numpy(wide_uv).to("cuda:0")[:, :, 4:4 + cr.C_COLS])
    dout_y = torch.from_numpy(np.full((NF, orows, ocols + 19), 9, np.uint16)).to("cuda:0")
    dout_uv = torch.from_numpy(np.full((NF, orows // 2, ocols // 2 + 3, 2), 8, np.uint16)).to("cuda:0")
    p.stabilize_color(color.P010, dwide, times, lens, synth.D_TRUE, out=(dout_y[:, :, 3:3 + ocols], dout_uv[:, :, 1:1 + ocols // 2]), **kw)
    b_y, b_uv = dout_y.cpu().numpy(), dout_uv.cpu().numpy()
    np.testing.assert_array_equal(b_y[:, :, 3:3 + ocols], one_y)
    np.testing.assert_array_equal(b_uv[:, :, 1:1 + ocols // 2], one_uv)
    assert (b_y[:, :, :3] == 9).all() and (b_y[:, :, 3 + ocols:] == 9).all()
    assert (b_uv[:, :, :1] == 8).all() and (b_uv[:, :, 1 + ocols // 2:] == 8).all()
    # device frames into host arrays, and host frames into device tensors
    (hy, huv), _ = p.stabilize_color(color.P010, dev, times, lens, synth.D_TRUE, out=(np.zeros_like(one_y), np.zeros_like(one_uv)), **kw)
    np.testing.assert_array_equal(hy, one_y)
    np.testing.assert_array_equal(huv, one_uv)
    into = (torch.from_numpy(np.zeros_like(one_y)).to("cuda:0"), torch.from_numpy(np.zeros_like(one_uv)).to("cuda:0"))
    p.stabilize_color(color.P010, (y, uv), times, lens, synth.D_TRUE, out=into, **kw)
    np.testing.assert_array_equal(into[0].cpu().numpy(), one_y)
    np.testing.assert_array_equal(into[1].cpu().numpy(), one_uv)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene, wide_planes):
    from rssync_amd import color, synth
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    y10, u10, v10 = wide_planes[10]
    y, uv = np.ascontiguousarray(y10 << 6), np.ascontiguousarray(_uv(u10, v10) << 6)
    u, v = np.ascontiguousarray(u10), np.ascontiguousarray(v10)
    W, H, NF = rr.COLS, rr.ROWS, rr.N_FRAMES
    (want_y, want_uv), want_n = p.stabilize_color(color.P010, (y, uv), times, lens, synth.D_TRUE, sigma=sr.SIGMA)
    lib = color.library()
    lib.rssync_set_panic_mode(1)
    L, T = np.ascontiguousarray(lens, np.float64), np.ascontiguousarray(times, np.float64)
    out_y, out_uv, out_u, out_v = np.zeros_like(y), np.zeros_like(uv), np.zeros_like(u), np.zeros_like(v)
    PD = C.POINTER(C.c_double)
    SEMI = (color.P010, color.P016, color.NV12)

    def image(arrays, w, h, fmt):
        img = color.ColorImage()
        b = 2 if fmt >= 16 else 1
        rows = (b * w, b * w) if fmt in SEMI else (b * w, b * w // 2, b * w // 2)
        heights = (h, h // 2, h // 2)
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

    def call(fmt=color.P010, src=None, dst=None, w=W, h=H, ow=W, oh=H, n=NF, prm=None, edit=None, entry=None):
        src = image((y, uv), w, h, color.P010) if src is None else src
        dst = image((out_y, out_uv), ow, oh, color.P010) if dst is None else dst
        if edit:
            edit(src, dst)
        prm = prm_with() if prm is None else prm
        return (entry or lib.rssync_color16_stabilize)(p._h, fmt, C.byref(src), n, w, h, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE, None,
                                                       C.byref(prm), C.byref(dst), ow, oh, None)

    def bad(match, **kw):
        assert call(**kw) != 0, match
        msg = lib.rssync_last_error().decode()
        assert match in msg, (match, msg)

    def set_(which, field, k, value):
        def edit(src, dst):
            getattr(src if which == "in" else dst, field)[k] = value
        return edit

    def i010(**kw):
        return dict(fmt=color.I010, src=image((y, u, v), W, H, color.I010), dst=image((out_y, out_u, out_v), W, H, color.I010), **kw)

    # formats: the new entry takes 16 .. 19 alone, the old entries do not take them
    for fmt in (0, 1, 2, 3, 20, 15, -1):
        bad("format", fmt=fmt)
    m = np.zeros((H, W, 2), np.float32)
    for fmt in (16, 17, 18, 19):
        bad("format", fmt=fmt, entry=lib.rssync_color_stabilize)
        assert lib.rssync_color_map(p._h, fmt, 0, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, None, C.byref(prm_with()), m.ctypes.data) != 0
        assert "format" in lib.rssync_last_error().decode()
    # alignment: pointer, pitch, stride
    bad("alignment", edit=set_("in", "plane", 0, y.ctypes.data + 1))
    bad("alignment", edit=set_("out", "plane", 1, out_uv.ctypes.data + 1))
    bad("alignment", edit=set_("in", "pitch", 1, 2 * W + 1))
    bad("alignment", edit=set_("out", "pitch", 0, 2 * W + 1))
    bad("alignment", edit=set_("in", "stride", 0, 2 * W * H + 1))
    bad("alignment", edit=set_("out", "stride", 1, 2 * W * (H // 2) + 1))
    bad("alignment", **i010(edit=set_("in", "pitch", 2, W + 1)))
    assert call(n=1, edit=set_("in", "stride", 1, 1)) == 0, lib.rssync_last_error().decode()     # (one frame: no stride is read)
    # pitch below the row bytes
    bad("pitch", edit=set_("in", "pitch", 0, 2 * W - 2))
    bad("pitch", edit=set_("in", "pitch", 1, 2 * W - 2))
    bad("pitch", edit=set_("out", "pitch", 1, 2 * W - 2))
    bad("pitch", **i010(edit=set_("out", "pitch", 2, W - 2)))
    bad("pitch", fmt=color.GRAY16, edit=set_("out", "pitch", 0, 2 * W - 2))
    bad("stride", edit=set_("in", "stride", 1, 2 * W * (H // 2) - 2))
    bad("is NULL", edit=set_("in", "plane", 1, None))
    # fills
    bad("fill 1", prm=prm_with(fill_set=1, fills=(0, 1024, 0, 0)))
    bad("fill 2", **i010(prm=prm_with(fill_set=1, fills=(0, 0, 1024, 0))))
    bad("fill 0", fmt=color.P016, prm=prm_with(fill_set=1, fills=(65536, 0, 0, 0)))
    bad("fill 0", fmt=color.GRAY16, prm=prm_with(fill_set=1, fills=(65536, 0, 0, 0)))
    bad("fill 0", prm=prm_with(fill_set=1, fills=(-1, 0, 0, 0)))
    bad("fill 2", fmt=color.P016, prm=prm_with(fill_set=1, fills=(0, 0, -1, 0)))
    bad("fill", prm=prm_with(fill=256))
    assert call(fmt=color.P016, prm=prm_with(fill_set=1, fills=(65535, 65535, 0, 0), fill=999)) == 0, lib.rssync_last_error().decode()
    assert call(prm=prm_with(fill_set=1, fills=(1023, 0, 1023, 0))) == 0, lib.rssync_last_error().decode()
    # the colour front's own
    bad("even", w=W - 1)
    bad("even", oh=H - 1)
    bad("too small", w=2, h=2)
    bad("chroma_site", prm=prm_with(site=2))
    bad("overlaps", dst=image((out_y, y.ctypes.data + 8), W, H, color.P010))
    bad("overlaps", dst=image((uv.ctypes.data, out_uv), W, H, color.P010))
    dev_uv = torch.from_numpy(np.zeros((NF, H // 2, W), np.uint16)).to("cuda:0")
    torch.cuda.synchronize()
    bad("mixed kinds", src=image((y, dev_uv.data_ptr()), W, H, color.P010))
    bad("mixed kinds", dst=image((out_y, dev_uv.data_ptr()), W, H, color.P010))
    with pytest.raises(ValueError):
        p.stabilize_color(color.P010, (y.astype(np.uint8), uv), times, lens, synth.D_TRUE)
    with pytest.raises(ValueError):
        p.stabilize_color(color.NV12, (y, uv), times, lens, synth.D_TRUE)
    # ... and the calls that follow work
    out_y[:], out_uv[:] = 0, 0
    assert call() == 0, lib.rssync_last_error().decode()
    np.testing.assert_array_equal(out_y, want_y)
    np.testing.assert_array_equal(out_uv, want_uv)
    (again_y, again_uv), again_n = p.stabilize_color(color.P010, (y, uv), times, lens, synth.D_TRUE, sigma=sr.SIGMA)
    np.testing.assert_array_equal(again_y, want_y)
    np.testing.assert_array_equal(again_uv, want_uv)
    np.testing.assert_array_equal(again_n, want_n)
