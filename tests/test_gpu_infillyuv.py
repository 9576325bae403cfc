"""The infill for 4:2:2 and 4:4:4 video on the device (include/rssync_infillyuv.h, csrc/kernels/infillyuv.hpp): every 8-bit
plane against the gray infill of that plane with that plane's camera, byte for byte; the formats in 16-bit containers against
their 8-bit siblings widened and against the composition of rssync_yuv_stabilize calls; its anchors, its locality, chunks with
halos, memory kinds and pitches, its errors; and the borrowed 4:2:2 chroma samples against the global-shutter truth, held to
the float64 restatement's figures (tests/infillyuv_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import infill_reference as ir
import infillyuv_reference as iyr
import rectify_reference as rr
import stabilize_reference as sr
import yuv_reference as yr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

N = len(zr.TIMES)
RADIUS = 3
SCENE = (rr.ROWS, rr.COLS)
FILLS = (77, 55, 66)

# name -> (luma (rows, cols), keywords of the calls): the smallest legal 4:2:2 frame; 65 chroma columns, one lane into a second
# 64-wide tile; a frame under one tile; odd rows; the scene's.  Both cameras, both filters, both chroma sites, one resized
# output (131 rows x 198 columns) with a pinhole and zoom 0.8.
CASES = {
    "scene-lens-bilinear-center": (SCENE, dict(camera=sr.LENS, filter=0, chroma_site=yr.CENTER)),
    "mid-lens-bicubic-left": ((199, 330), dict(camera=sr.LENS, filter=1, chroma_site=yr.LEFT)),
    "mid-pinhole-resized-bicubic-center": ((199, 330), dict(camera=sr.PINHOLE, filter=1, chroma_site=yr.CENTER, out_size=(198, 131), zoom=0.8)),
    "wide-lens-bilinear-center": ((5, 130), dict(camera=sr.LENS, filter=0, chroma_site=yr.CENTER)),
    "small-pinhole-bicubic-center": ((31, 38), dict(camera=sr.PINHOLE, filter=1, chroma_site=yr.CENTER, zoom=0.8)),
    "least-pinhole-bilinear-center": ((3, 4), dict(camera=sr.PINHOLE, filter=0, chroma_site=yr.CENTER, zoom=0.8)),
}
FIRST = "scene-lens-bilinear-center"
MID = "mid-lens-bicubic-left"
LEAST = "least-pinhole-bilinear-center"


@pytest.fixture(scope="module")
def scene(built):
    import rssync_amd
    from rssync_amd import synth
    s = dict(rr.scene())
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(s["gyro"].quats, s["gyro"].fs, s["gyro"].t0)
    s["problem"] = p
    targets = p.stabilize_path(zr.TIMES, s["lens"][0], synth.D_TRUE, zr.SIGMA)
    targets.setflags(write=False)
    s["targets"] = targets
    return s


_PLANES = {}


def _planes(size):
    """lens and N frames of noise at a luma size: Y, the 4:2:2 U, V and UV, the 4:4:4 U4 and V4 (read-only)"""
    if size not in _PLANES:
        rows, cols = size
        rng = np.random.default_rng(rows * 1000 + cols)
        y, u4, v4 = (rng.integers(0, 256, size=(N, rows, cols), dtype=np.uint8) for _ in range(3))
        u, v = (rng.integers(0, 256, size=(N, rows, cols // 2), dtype=np.uint8) for _ in range(2))
        d = dict(lens=rr.scaled_lens(rows, cols), y=y, u=u, v=v, uv=np.stack([u, v], axis=-1), u4=u4, v4=v4)
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _PLANES[size] = d
    return _PLANES[size]


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _same(got, want):
    """(planes, n_outside, n_borrowed) against the same"""
    assert len(got[0]) == len(want[0])
    for k, (a, b) in enumerate(zip(got[0], want[0])):
        np.testing.assert_array_equal(_np(a), _np(b), err_msg="plane %d" % k)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])


def _uv(u, v):
    return np.stack([u, v], axis=-1)


def _gray_planes(scene, size, kw, radius=RADIUS, fills=FILLS):
    """the header's first consequence: every plane as the gray infill of that plane with that plane's lens, times, output
    camera and fill -> ((y, u, v) of 4:2:2, (u4, v4) of 4:4:4, n_outside (n, 2), n_borrowed (n, 2) of 4:2:2)"""
    from rssync_amd import synth
    p, d = scene["problem"], _planes(size)
    rows, cols = size
    kw = dict(kw)
    site, out_size, zoom = kw.pop("chroma_site"), kw.pop("out_size", None), kw.pop("zoom", 1.0)
    ocols, orows = (cols, rows) if out_size is None else out_size
    targets = scene["targets"]
    lens_c = yr.chroma_lens422(d["lens"], site)
    cam_c = yr.chroma_camera422(d["lens"], rows, cols, orows, ocols, site, zoom)
    ykw = dict(targets=targets, out_size=out_size, zoom=zoom, **kw)
    ckw = dict(targets=targets, out_size=(ocols // 2, orows), out_camera=cam_c, **kw)
    y, n_y, b_y = p.stabilize_frames_infilled(d["y"], zr.TIMES, d["lens"], synth.D_TRUE, radius, fill=fills[0], **ykw)
    u, n_c, b_c = p.stabilize_frames_infilled(d["u"], zr.TIMES, lens_c, synth.D_TRUE, radius, fill=fills[1], **ckw)
    v, n_v, b_v = p.stabilize_frames_infilled(d["v"], zr.TIMES, lens_c, synth.D_TRUE, radius, fill=fills[2], **ckw)
    np.testing.assert_array_equal(n_v, n_c)
    np.testing.assert_array_equal(b_v, b_c)
    # 4:4:4: the chroma planes have the luma's camera
    u4, n_4, b_4 = p.stabilize_frames_infilled(d["u4"], zr.TIMES, d["lens"], synth.D_TRUE, radius, fill=fills[1], **ykw)
    v4, _, _ = p.stabilize_frames_infilled(d["v4"], zr.TIMES, d["lens"], synth.D_TRUE, radius, fill=fills[2], **ykw)
    np.testing.assert_array_equal(n_4, n_y)
    np.testing.assert_array_equal(b_4, b_y)
    return (y, u, v), (u4, v4), np.stack([n_y, n_c], axis=-1), np.stack([b_y, b_c], axis=-1)


_CACHE = {}


def _case(scene, name):
    """-> (the I422 device result, the I444 device result, the gray infills) of a case, computed once (read-only)"""
    from rssync_amd import synth, yuv
    if name not in _CACHE:
        size, kw = CASES[name]
        d = _planes(size)
        args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
        got = scene["problem"].stabilize_yuv_infilled(yuv.I422, (d["y"], d["u"], d["v"]), *args, targets=scene["targets"], fills=FILLS, **kw)
        got4 = scene["problem"].stabilize_yuv_infilled(yuv.I444, (d["y"], d["u4"], d["v4"]), *args, targets=scene["targets"], fills=FILLS, **kw)
        want = _gray_planes(scene, size, kw)
        for a in got[0] + got[1:] + got4[0] + got4[1:] + want[0] + want[1] + want[2:]:
            a.setflags(write=False)
        _CACHE[name] = (got, got4, want)
    return _CACHE[name]


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_8_bit_planes_are_the_gray_infill_of_each_plane(scene, name):
    """Y, U and V of I422 and of I444 (whose chroma has the luma camera and whose second counts are its first), and NV16 as
    I422 with the chroma interleaved"""
    from rssync_amd import synth, yuv
    got, got4, (w422, w44, w_out, w_lent) = _case(scene, name)
    print(name, "outside", w_out.tolist(), "borrowed", w_lent.tolist())
    for planes, n_outside, n_borrowed in (got, got4):
        assert all(a.dtype == np.uint8 for a in planes) and n_outside.dtype == np.uint64 and n_borrowed.dtype == np.uint64
        assert n_outside.shape == n_borrowed.shape == (N, 2)
    _same(got, (w422, w_out, w_lent))
    _same(got4, ((w422[0],) + w44, np.stack([w_out[:, 0]] * 2, axis=-1), np.stack([w_lent[:, 0]] * 2, axis=-1)))
    size, kw = CASES[name]
    d = _planes(size)
    nv = scene["problem"].stabilize_yuv_infilled(yuv.NV16, (d["y"], d["uv"]), zr.TIMES, d["lens"], synth.D_TRUE, RADIUS, targets=scene["targets"],
                                                 fills=FILLS, **kw)
    _same(nv, ((w422[0], _uv(w422[1], w422[2])), w_out, w_lent))
    # from the gray calls' own counts: the case is not vacuous
    if name == LEAST:
        assert w_lent[:, 0].sum() > 0 and w_lent[:, 1].sum() > 0, w_lent.tolist()
    else:
        assert (w_lent > 0).all() and (w_out > 0).all(), (w_lent.tolist(), w_out.tolist())


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_16_bit_formats_on_8_bit_values_are_the_sibling_widened(scene, name):
    from rssync_amd import synth, yuv
    p = scene["problem"]
    ((y8, u8, v8), n8, nb8), ((_, u48, v48), n48, nb48), _ = _case(scene, name)
    size, kw = CASES[name]
    d = _planes(size)
    y, u, v, uv, u4, v4 = (d[k].astype(np.uint16) for k in ("y", "u", "v", "uv", "u4", "v4"))
    uv8 = _uv(u8, v8)
    args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
    ckw = dict(targets=scene["targets"], fills=FILLS, **kw)
    (yi, ui, vi), ni, nbi = p.stabilize_yuv_infilled(yuv.I210, (y, u, v), *args, **ckw)
    (y10, uv10), n10, nb10 = p.stabilize_yuv_infilled(yuv.P210, (y << 6, uv << 6), *args, **ckw)
    (y16, uv16), n16, nb16 = p.stabilize_yuv_infilled(yuv.P216, (y, uv), *args, **ckw)
    (y4, u4o, v4o), n4, nb4 = p.stabilize_yuv_infilled(yuv.I410, (y, u4, v4), *args, **ckw)
    assert (y10 & 63).max() == 0 and (uv10 & 63).max() == 0
    overshoot = 0
    for wide, narrow in ((yi, y8), (ui, u8), (vi, v8), (y10 >> 6, y8), (uv10 >> 6, uv8), (y16, y8), (uv16, uv8), (y4, y8), (u4o, u48), (v4o, v48)):
        assert wide.dtype == np.uint16 and wide.shape == narrow.shape
        if kw["filter"] == 0:
            np.testing.assert_array_equal(wide, narrow)
        else:   # the bicubic sampler clamps to the format's range: 255 may stand for more, every other value is the same
            assert ((wide == narrow) | ((narrow == 255) & (wide > 255))).all()
            overshoot += int((wide > 255).sum())
    assert (overshoot > 0) == (kw["filter"] == 1)
    for counts, want in (((ni, nbi), (n8, nb8)), ((n10, nb10), (n8, nb8)), ((n16, nb16), (n8, nb8)), ((n4, nb4), (n48, nb48))):
        np.testing.assert_array_equal(counts[0], want[0])
        np.testing.assert_array_equal(counts[1], want[1])


# 3 ---------------------------------------------------------------------------------------------------------------------
N16, RADIUS16 = 5, 2


def _compose16(p, fmt, frames, rows, cols, lens, targets, fills, **kw):
    """the header's second consequence through rssync_yuv_stabilize: every frame g alone with time T_g and target
    targets[f], merged per sample and per plane at the first candidate whose position (rssync_yuv_map) is inside its plane
    -> (planes, n_outside (n, 2), n_borrowed (n, 2)).  fills: sample values (P210's are stored << 6)."""
    from rssync_amd import synth, yuv
    n = N16
    shift = 6 if fmt == yuv.P210 else 0
    c_cols = cols // 2 if yuv.is_422(fmt) else cols
    outs, n_outside, n_borrowed = None, np.zeros((n, 2), np.uint64), np.zeros((n, 2), np.uint64)
    for f in range(n):
        done = None
        for k, g in enumerate(ir.candidates(f, n, RADIUS16)):
            one = tuple(a[g:g + 1] for a in frames)
            a, _ = p.stabilize_yuv(fmt, one, zr.TIMES[g:g + 1], lens, synth.D_TRUE, targets=targets[f:f + 1], fills=fills, **kw)
            mkw = {key: val for key, val in kw.items() if key != "filter"}
            maps = [p.yuv_map(fmt, pl, cols, rows, lens, zr.TIMES[g], synth.D_TRUE, target=targets[f], **mkw) for pl in (0, 1)]
            inside = [sr.inside(maps[0], rows, cols), sr.inside(maps[1], rows, c_cols)]
            inside += [inside[1]] * (len(a) - 2)
            if outs is None:
                outs = [np.empty((n,) + x.shape[1:], np.uint16) for x in a]
                outs[0][:] = fills[0] << shift
                if len(a) == 2:         # P210, P216: the interleaved pairs
                    outs[1][..., 0], outs[1][..., 1] = fills[1] << shift, fills[2] << shift
                else:
                    outs[1][:], outs[2][:] = fills[1], fills[2]
            if done is None:
                done = [np.zeros(m.shape, bool) for m in inside]
            for pl in range(len(a)):
                new = inside[pl] & ~done[pl]
                outs[pl][f][new] = a[pl][0][new]
                if pl < 2:
                    n_borrowed[f, pl] += int(new.sum()) if k else 0
                done[pl] |= new
        n_outside[f] = [int((~done[0]).sum()), int((~done[1]).sum())]
    return tuple(outs), n_outside, n_borrowed


@pytest.mark.parametrize("filter", [0, 1], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("fmt_name", ["I210", "P210", "P216", "I410"])
def test_true_10_and_16_bit_values_are_the_composition_of_single_frame_calls(scene, fmt_name, filter):
    from rssync_amd import synth, yuv
    p = scene["problem"]
    fmt = getattr(yuv, fmt_name)
    rows, cols = (31, 38) if filter else (199, 330)
    top = 1 << yuv.DEPTH[fmt]
    rng = np.random.default_rng(rows + 17 * filter + fmt)
    y, u4, v4 = (rng.integers(0, top, size=(N16, rows, cols), dtype=np.uint16) for _ in range(3))
    u, v = (rng.integers(0, top, size=(N16, rows, cols // 2), dtype=np.uint16) for _ in range(2))
    frames = {"I210": (y, u, v), "P210": (y << 6, _uv(u, v) << 6), "P216": (y, _uv(u, v)), "I410": (y, u4, v4)}[fmt_name]
    lens, targets = rr.scaled_lens(rows, cols), scene["targets"][:N16]
    fills = (5, 600, 700) if top == 1024 else (5, 60000, 700)
    kw = dict(filter=filter, camera=sr.LENS if filter else sr.PINHOLE, zoom=0.9, chroma_site=yr.LEFT if filter else yr.CENTER)
    got = p.stabilize_yuv_infilled(fmt, frames, zr.TIMES[:N16], lens, synth.D_TRUE, RADIUS16, targets=targets, fills=fills, **kw)
    want = _compose16(p, fmt, frames, rows, cols, lens, targets, fills, **kw)
    print(fmt_name, (rows, cols), filter, "outside", want[1].tolist(), "borrowed", want[2].tolist())
    assert want[2][:, 0].sum() > 0 and want[2][:, 1].sum() > 0
    if fmt == yuv.I410:
        np.testing.assert_array_equal(want[1][:, 1], want[1][:, 0])
        np.testing.assert_array_equal(want[2][:, 1], want[2][:, 0])
    _same(got, want)


# 4 ---------------------------------------------------------------------------------------------------------------------
def _frames_of(d, fmt_name):
    y, u, v, uv, u4, v4 = (d[k] for k in ("y", "u", "v", "uv", "u4", "v4"))
    w = lambda a: a.astype(np.uint16)  # noqa: E731
    return {"I422": (y, u, v), "NV16": (y, uv), "I444": (y, u4, v4), "I210": (w(y) << 2, w(u) << 2, w(v) << 2),
            "P210": (w(y) << 8, w(uv) << 8), "P216": (w(y) * 257, w(uv) * 257), "I410": (w(y) << 2, w(u4) << 2, w(v4) << 2)}[fmt_name]


@pytest.mark.parametrize("explicit", [False, True], ids=["path", "targets"])
@pytest.mark.parametrize("fmt_name", ["I422", "NV16", "I444", "I210", "P210", "P216", "I410"])
def test_radius_zero_and_a_single_frame_are_the_stabiliser(scene, fmt_name, explicit):
    from rssync_amd import synth, yuv
    p = scene["problem"]
    fmt = getattr(yuv, fmt_name)
    d = _planes((199, 330))
    frames = _frames_of(d, fmt_name)
    for filter in (0, 1):
        kw = dict(sigma=zr.SIGMA, fill=FILLS[0], filter=filter)
        t = scene["targets"] if explicit else None
        want, want_n = p.stabilize_yuv(fmt, frames, zr.TIMES, d["lens"], synth.D_TRUE, targets=t, **kw)
        assert want_n[:, 0].sum() > 0 and want_n[:, 1].sum() > 0
        got = p.stabilize_yuv_infilled(fmt, frames, zr.TIMES, d["lens"], synth.D_TRUE, 0, targets=t, **kw)
        _same(got, (want, want_n, np.zeros((N, 2), np.uint64)))
        for f in (0, 5):
            one = tuple(a[f:f + 1] for a in frames)
            got = p.stabilize_yuv_infilled(fmt, one, zr.TIMES[f:f + 1], d["lens"], synth.D_TRUE, RADIUS, targets=None if t is None else t[f:f + 1], **kw)
            _same(got, (tuple(a[f:f + 1] for a in want), want_n[f:f + 1], np.zeros((1, 2), np.uint64)))


def test_radius_8_skips_candidates_at_both_ends(scene):
    """radius 8 on the 9 frames: every frame's order names frames that are not frames of the call; the planes are the gray
    infill's at that radius"""
    from rssync_amd import synth, yuv
    size, kw = CASES[MID]
    d = _planes(size)
    assert all(len(ir.candidates(f, N, 8)) == N for f in range(N))
    (y, u, v), _, n_out, n_lent = _gray_planes(scene, size, kw, radius=8)
    got = scene["problem"].stabilize_yuv_infilled(yuv.NV16, (d["y"], d["uv"]), zr.TIMES, d["lens"], synth.D_TRUE, 8, targets=scene["targets"],
                                                  fills=FILLS, **kw)
    _same(got, ((y, _uv(u, v)), n_out, n_lent))
    # what is outside a frame's own plane does not depend on the radius; a larger one can only borrow more of it
    _, _, (_, _, out3, lent3) = _case(scene, MID)
    np.testing.assert_array_equal(n_out + n_lent, out3 + lent3)
    assert (n_lent >= lent3).all()


@pytest.mark.parametrize("fmt_name", ["NV16", "I444"])
def test_the_path_agrees_with_explicit_targets_from_stabilize_path(scene, fmt_name):
    from rssync_amd import synth, yuv
    got, got4, _ = _case(scene, MID)
    size, kw = CASES[MID]
    d = _planes(size)
    res = scene["problem"].stabilize_yuv_infilled(getattr(yuv, fmt_name), _frames_of(d, fmt_name), zr.TIMES, d["lens"], synth.D_TRUE, RADIUS,
                                                  sigma=zr.SIGMA, fills=FILLS, **kw)
    ((y, u, v), n, nb) = got
    _same(res, ((y, _uv(u, v)), n, nb) if fmt_name == "NV16" else got4)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4, 8])
def test_a_frame_depends_on_its_neighbourhood_alone(scene, f):
    from rssync_amd import synth, yuv
    ((y, u, v), n, nb), ((_, u4, v4), n4, nb4), _ = _case(scene, MID)
    size, kw = CASES[MID]
    d = _planes(size)
    lo, hi = max(0, f - RADIUS), min(N - 1, f + RADIUS)
    sub = slice(lo, hi + 1)
    args = (zr.TIMES[sub], d["lens"], synth.D_TRUE, RADIUS)
    ckw = dict(targets=scene["targets"][sub], fills=FILLS, **kw)
    (gy, gu, gv), gn, gnb = scene["problem"].stabilize_yuv_infilled(yuv.I422, (d["y"][sub], d["u"][sub], d["v"][sub]), *args, **ckw)
    for a, b in ((gy, y), (gu, u), (gv, v)):
        np.testing.assert_array_equal(a[f - lo], b[f])
    np.testing.assert_array_equal(gn[f - lo], n[f])
    np.testing.assert_array_equal(gnb[f - lo], nb[f])
    (gy, gu, gv), gn, gnb = scene["problem"].stabilize_yuv_infilled(yuv.I444, (d["y"][sub], d["u4"][sub], d["v4"][sub]), *args, **ckw)
    for a, b in ((gy, y), (gu, u4), (gv, v4)):
        np.testing.assert_array_equal(a[f - lo], b[f])
    np.testing.assert_array_equal(gn[f - lo], n4[f])
    np.testing.assert_array_equal(gnb[f - lo], nb4[f])


def _slot_bytes(frames_per_chunk):
    """a budget whose half pays for the halo of RADIUS frames on each side and that many I422 frames of the scene's size:
    2 radius + 1 tables of the one region, the input and the output planes"""
    rows, cols = SCENE
    image = rows * cols * 2
    per_frame = (2 * RADIUS + 1) * (rows + 1) * 36 + 2 * image
    return 2 * (2 * RADIUS * image + frames_per_chunk * per_frame)


@pytest.mark.parametrize("fmt_name", ["NV16", "I422"])
@pytest.mark.parametrize("budget", [1000, _slot_bytes(2.5), _slot_bytes(4.5)], ids=["one-frame", "two-frames", "four-frames"])
def test_chunks_with_halos(scene, fmt_name, budget):
    from rssync_amd import synth, yuv
    ((y, u, v), n, nb), _, _ = _case(scene, FIRST)
    size, kw = CASES[FIRST]
    d = _planes(size)
    nv16 = fmt_name == "NV16"
    got = scene["problem"].stabilize_yuv_infilled_budget(getattr(yuv, fmt_name), _frames_of(d, fmt_name), zr.TIMES, d["lens"], synth.D_TRUE, RADIUS,
                                                         budget, targets=scene["targets"], fills=FILLS + (0,), **kw)
    _same(got, ((y, _uv(u, v)) if nv16 else (y, u, v), n, nb))


def test_chunks_of_a_resized_pinhole_call_at_zoom_0_8(scene):
    """the launcher's configuration with a zoom, an output size and a pinhole, one frame per chunk: 4:4:4 and 16-bit 4:2:2"""
    from rssync_amd import synth, yuv
    name = "mid-pinhole-resized-bicubic-center"
    ((y, u, v), n, nb), got4, _ = _case(scene, name)
    size, kw = CASES[name]
    d = _planes(size)
    args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS, 1000)
    _same(scene["problem"].stabilize_yuv_infilled_budget(yuv.I444, _frames_of(d, "I444"), *args, targets=scene["targets"], fills=FILLS + (0,), **kw),
          got4)
    w16 = lambda a: a.astype(np.uint16)  # noqa: E731
    (y16, uv16), n16, nb16 = scene["problem"].stabilize_yuv_infilled_budget(yuv.P216, (w16(d["y"]), w16(d["uv"])), *args, targets=scene["targets"],
                                                                            fills=FILLS + (0,), **kw)
    uv8 = _uv(u, v)
    assert ((y16 == y) | ((y == 255) & (y16 > 255))).all() and ((uv16 == uv8) | ((uv8 == 255) & (uv16 > 255))).all()
    np.testing.assert_array_equal(n16, n)
    np.testing.assert_array_equal(nb16, nb)


def test_pitched_views_and_device_memory(scene):
    from rssync_amd import synth, yuv
    p = scene["problem"]
    ((y, u, v), n, nb), _, _ = _case(scene, MID)
    size, kw = CASES[MID]
    rows, cols = size
    hc = cols // 2
    d = _planes(size)
    want = ((y, _uv(u, v)), n, nb)
    want3 = ((y, u, v), n, nb)
    args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
    ckw = dict(targets=scene["targets"], fills=FILLS, **kw)
    dev_of = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")  # noqa: E731
    # device-resident tensors: NV16 and I422
    dev = (dev_of(d["y"]), dev_of(d["uv"]))
    got = p.stabilize_yuv_infilled(yuv.NV16, dev, *args, **ckw)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in got[0])
    _same(got, want)
    _same(p.stabilize_yuv_infilled(yuv.I422, (dev[0], dev_of(d["u"]), dev_of(d["v"])), *args, **ckw), want3)
    # host in, device out; device in, host out
    dout = (torch.zeros((N, rows, cols), dtype=torch.uint8, device="cuda:0"), torch.zeros((N, rows, hc, 2), dtype=torch.uint8, device="cuda:0"))
    got = p.stabilize_yuv_infilled(yuv.NV16, (d["y"], d["uv"]), *args, out=dout, **ckw)
    assert got[0] is dout
    _same(got, want)
    hout = (np.zeros((N, rows, cols), np.uint8), np.zeros((N, rows, hc, 2), np.uint8))
    _same(p.stabilize_yuv_infilled(yuv.NV16, dev, *args, out=hout, **ckw), want)
    # device frames through chunks: the neighbours are read in place
    hout[0][:], hout[1][:] = 0, 0
    _same(p.stabilize_yuv_infilled_budget(yuv.NV16, dev, *args, 1000, out=hout, targets=scene["targets"], fills=FILLS + (0,), **kw), want)
    # pitched device buffers, a guard pattern between the rows of the result
    wide_y = np.zeros((N, rows + 2, cols + 61), np.uint8)
    wide_y[:, 1:1 + rows, 13:13 + cols] = d["y"]
    wide_uv = np.zeros((N, rows + 1, hc + 9, 2), np.uint8)
    wide_uv[:, 1:, 4:4 + hc] = d["uv"]
    dwide = (torch.from_numpy(wide_y).to("cuda:0")[:, 1:1 + rows, 13:13 + cols], torch.from_numpy(wide_uv).to("cuda:0")[:, 1:, 4:4 + hc])
    dy = torch.full((N, rows + 3, cols + 19), 201, dtype=torch.uint8, device="cuda:0")
    duv = torch.full((N, rows + 1, hc + 5, 2), 202, dtype=torch.uint8, device="cuda:0")
    views = (dy[:, 2:2 + rows, 3:3 + cols], duv[:, :rows, 2:2 + hc])
    res, gn, gnb = p.stabilize_yuv_infilled(yuv.NV16, dwide, *args, out=views, **ckw)
    assert res is views
    by, buv = dy.cpu().numpy(), duv.cpu().numpy()
    _same(((by[:, 2:2 + rows, 3:3 + cols], buv[:, :rows, 2:2 + hc]), gn, gnb), want)
    gy, guv = np.ones(by.shape, bool), np.ones(buv.shape, bool)
    gy[:, 2:2 + rows, 3:3 + cols] = False
    guv[:, :rows, 2:2 + hc] = False
    assert (by[gy] == 201).all() and (buv[guv] == 202).all()
    # pitched host buffers, the same way, I422
    wide_u = np.zeros((N, rows, hc + 7), np.uint8)
    wide_u[:, :, 3:3 + hc] = d["u"]
    wide_v = np.zeros((N, rows + 2, hc), np.uint8)
    wide_v[:, 2:] = d["v"]
    hy = np.full((N, rows + 1, cols + 5), 9, np.uint8)
    hu = np.full((N, rows, hc + 3), 8, np.uint8)
    hv = np.full((N, rows + 1, hc), 7, np.uint8)
    _, gn, gnb = p.stabilize_yuv_infilled(yuv.I422, (wide_y[:, 1:1 + rows, 13:13 + cols], wide_u[:, :, 3:3 + hc], wide_v[:, 2:]), *args,
                                          out=(hy[:, :rows, 2:2 + cols], hu[:, :, 1:1 + hc], hv[:, :rows]), **ckw)
    _same(((hy[:, :rows, 2:2 + cols], hu[:, :, 1:1 + hc], hv[:, :rows]), gn, gnb), want3)
    assert (hy[:, rows:] == 9).all() and (hy[:, :, :2] == 9).all() and (hy[:, :, 2 + cols:] == 9).all()
    assert (hu[:, :, :1] == 8).all() and (hu[:, :, 1 + hc:] == 8).all() and (hv[:, rows:] == 7).all()
    # planes of one image must be of one kind
    with pytest.raises(yuv.RsSyncError, match="mixed kinds"):
        p.stabilize_yuv_infilled(yuv.NV16, (dev[0], d["uv"]), *args, **ckw)
    _same(p.stabilize_yuv_infilled(yuv.NV16, dev, *args, **ckw), want)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_borrowed_chroma_samples_against_the_global_shutter_truth(scene):
    """Mean absolute grey difference to the truth over the 4:2:2 chroma samples the device borrowed, frames 32, 33, 34, per
    plane U, V: within iyr.error_margin -- what positions that lie within the device tolerance (yr.device_tolerance) of the
    restatement's can move the figure by -- of the float64 restatement's iyr.BORROWED_ERROR, and far below the constant
    fill's iyr.FILL_ERROR; at least iyr.MIN_BORROWED_SHARE of the outside samples borrowed."""
    from rssync_amd import synth, yuv
    p, lens = scene["problem"], scene["lens"]
    y, u, v, times = iyr.video()
    targets = ir.video_targets()
    args = (yuv.I422, (y, u, v), times, lens, synth.D_TRUE)
    own0, own_n = p.stabilize_yuv(*args, targets=targets, fills=(0, 0, 0))
    own255, _ = p.stabilize_yuv(*args, targets=targets, fills=(255, 255, 255))
    out, n, nb = p.stabilize_yuv_infilled(*args, iyr.RADIUS, targets=targets, fills=(0, 0, 0))
    out255, _, _ = p.stabilize_yuv_infilled(*args, iyr.RADIUS, targets=targets, fills=(255, 255, 255))
    truth = yr.truth(yr.CENTER)
    for k, f in enumerate(range(*ir.VIDEO_SCENE.indices(len(times)))):
        for pl, name in ((1, "U"), (2, "V")):
            outside = own0[pl][f] != own255[pl][f]
            lent = outside & (out[pl][f] == out255[pl][f])
            assert outside.sum() == own_n[f, 1] and lent.sum() == nb[f, 1] and own_n[f, 1] == n[f, 1] + nb[f, 1]
            err = float(np.abs(out[pl][f].astype(np.float64) - truth[pl - 1][k].astype(np.float64))[lent].mean())
            share = float(nb[f, 1]) / float(own_n[f, 1])
            print("%s frame %d: %d of %d outside samples borrowed (%.4f; reference %d of %d), error %.3f (reference %.3f, fill %.1f)" %
                  (name, rr.F0 + k, nb[f, 1], own_n[f, 1], share, iyr.SEEN[yr.CENTER][k], iyr.OUTSIDE[yr.CENTER][k], err,
                   iyr.BORROWED_ERROR[pl - 1][k], iyr.FILL_ERROR[pl - 1][k]))
            assert abs(err - iyr.BORROWED_ERROR[pl - 1][k]) <= iyr.error_margin(k), (name, k, err, iyr.error_margin(k))
            assert err <= iyr.FAR_BELOW * iyr.FILL_ERROR[pl - 1][k], (name, k, err)
            assert share >= iyr.MIN_BORROWED_SHARE, (name, k, share)
        # the luma plane of the same call: infill_reference's share
        assert float(nb[f, 0]) / float(own_n[f, 0]) >= ir.MIN_BORROWED_SHARE and own_n[f, 0] == n[f, 0] + nb[f, 0]


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene):
    from rssync_amd import color, infillyuv, synth, yuv
    p = scene["problem"]
    size, kw = CASES[MID]
    rows, cols = size
    d = _planes(size)
    ((wy, wu, wv), wn, wnb), _, _ = _case(scene, MID)
    want = ((wy, _uv(wu, wv)), wn, wnb)
    lib = infillyuv.library()
    lib.rssync_set_panic_mode(1)
    PD, PU64 = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    L = np.ascontiguousarray(d["lens"], np.float64)
    T = np.ascontiguousarray(zr.TIMES)
    Q = np.ascontiguousarray(scene["targets"])
    prm = color.params(kw["chroma_site"], FILLS, camera=kw["camera"], filter=kw["filter"])
    y, uv = np.ascontiguousarray(d["y"]), np.ascontiguousarray(d["uv"])
    oy, ouv = np.zeros_like(y), np.zeros_like(uv)
    wide = np.zeros(2 * y.size + 2, np.uint8)       # a 16-bit plane that starts at an odd address
    n, nb = np.zeros((N, 2), np.uint64), np.zeros((N, 2), np.uint64)

    def image(a, b, w, h, second=True, scale=1):
        img = color.ColorImage()
        img.plane[0], img.pitch[0], img.stride[0] = a, scale * w, scale * w * h
        if second:
            img.plane[1], img.pitch[1], img.stride[1] = b, scale * w, scale * w * h
        return img

    def call(radius=RADIUS, w=cols, second=True, fmt=yuv.NV16, overlap=False, odd=False):
        src = image(y.ctypes.data, uv.ctypes.data, cols, rows, second)
        dst = image(y.ctypes.data if overlap else oy.ctypes.data, ouv.ctypes.data, cols, rows)
        if odd:     # P216, W16 wide, with a luma plane at an odd address: turned away before anything is read
            src = image(wide.ctypes.data + 1, uv.ctypes.data, W16, rows, scale=2)
        return lib.rssync_infillyuv_stabilize(p._h, fmt, C.byref(src), N, w, rows, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE,
                                              Q.ctypes.data_as(PD), C.byref(prm), C.byref(dst), w, rows, n.ctypes.data_as(PU64), radius,
                                              nb.ctypes.data_as(PU64))

    W16 = cols // 4 * 2         # even, and its rows of 16-bit words fit the 8-bit planes' pitches
    assert wide.ctypes.data % 2 == 0 and 2 * W16 <= cols and (cols * rows) % 2 == 0
    for match, bad in (("radius", dict(radius=-1)), ("radius", dict(radius=9)), ("format", dict(fmt=color.NV12)), ("format", dict(fmt=color.P010)),
                       ("format", dict(fmt=7)), ("even", dict(w=cols - 1)), ("alignment", dict(fmt=yuv.P216, w=cols // 4 * 2, odd=True)),
                       ("overlaps", dict(overlap=True)), ("is NULL", dict(second=False))):
        assert call(**bad) != 0, bad
        msg = lib.rssync_last_error().decode()
        assert match in msg and msg.startswith(("infillyuv: ", "color: ")), (match, msg)
        assert call() == 0, lib.rssync_last_error().decode()
        _same(((oy, ouv), n, nb), want)
    assert call(radius=8) == 0 and call(radius=0) == 0
    # the Python wrapper: its own checks raise before the library is called, the library's arrive as RsSyncError
    args = (yuv.NV16, (y, uv), zr.TIMES, d["lens"], synth.D_TRUE)
    with pytest.raises(infillyuv.RsSyncError, match="radius"):
        p.stabilize_yuv_infilled(*args, 9)
    with pytest.raises(ValueError, match="format"):
        p.stabilize_yuv_infilled(color.NV12, (y, uv), *args[2:], RADIUS)
    for bad in (np.zeros((N,), np.uint64), np.zeros((N + 1, 2), np.uint64), np.zeros((N, 2), np.int32)):
        with pytest.raises(ValueError, match="n_borrowed"):
            p.stabilize_yuv_infilled(*args, RADIUS, n_borrowed=bad)
    mine = np.zeros((N, 2), np.uint64)
    got = p.stabilize_yuv_infilled(*args, RADIUS, targets=scene["targets"], fills=FILLS, n_borrowed=mine, **kw)
    assert got[2].base is mine or got[2] is mine
    _same(got, want)
