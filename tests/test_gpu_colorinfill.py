"""The colour infill on the device (include/rssync_colorinfill.h, csrc/kernels/colorinfill.hpp): every 8-bit plane against
the gray infill of that plane with that plane's camera, byte for byte; the 16-bit formats against their 8-bit siblings widened
and against the composition of rssync_color16_stabilize calls; its anchors, its locality, chunks with halos, memory kinds and
pitches, its errors; and the borrowed samples against the global-shutter truth, held to the float64 restatement's figures
(tests/colorinfill_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color_reference as cr
import colorinfill_reference as cir
import infill_reference as ir
import rectify_reference as rr
import stabilize_reference as sr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

N = len(zr.TIMES)
RADIUS = 3
SCENE = (rr.ROWS, rr.COLS)
# luma (rows, cols): one under a 64 x 4 tile of chroma samples, an odd chroma size that is no multiple of the tile, the scene's
SIZES = [(38, 30), (330, 198), SCENE]
FILLS = (77, 55, 66)

# name -> (luma size, keywords of the colour calls): both cameras, both filters, both chroma sites, one resized output with
# zoom 0.8 and a pinhole
CASES = {
    "scene-lens-bilinear-center": (SCENE, dict(camera=sr.LENS, filter=0, chroma_site=cr.CENTER)),
    "mid-lens-bicubic-left": ((330, 198), dict(camera=sr.LENS, filter=1, chroma_site=cr.LEFT)),
    "mid-pinhole-resized-bicubic-center": ((330, 198), dict(camera=sr.PINHOLE, filter=1, chroma_site=cr.CENTER, out_size=(130, 198), zoom=0.8)),
    "small-pinhole-bilinear-left": ((38, 30), dict(camera=sr.PINHOLE, filter=0, chroma_site=cr.LEFT, zoom=0.8)),
}
FIRST = "scene-lens-bilinear-center"


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
    """lens and N frames of noise at a luma size: Y, U, V, UV and RGBA (read-only)"""
    if size not in _PLANES:
        rows, cols = size
        rng = np.random.default_rng(rows * 1000 + cols)
        y = rng.integers(0, 256, size=(N, rows, cols), dtype=np.uint8)
        u, v = (rng.integers(0, 256, size=(N, rows // 2, cols // 2), dtype=np.uint8) for _ in range(2))
        d = dict(lens=rr.scaled_lens(rows, cols), y=y, u=u, v=v, uv=np.stack([u, v], axis=-1),
                 rgba=rng.integers(0, 256, size=(N, rows, cols, 4), dtype=np.uint8))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _PLANES[size] = d
    return _PLANES[size]


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _same(got, want):
    """(planes, n_outside, n_borrowed) against the same"""
    gp, wp = (x if isinstance(x, (tuple, list)) else (x,) for x in (got[0], want[0]))
    assert len(gp) == len(wp)
    for k, (a, b) in enumerate(zip(gp, wp)):
        np.testing.assert_array_equal(_np(a), _np(b), err_msg="plane %d" % k)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])


def _gray_planes(scene, size, kw, radius=RADIUS, sub=slice(None), fills=FILLS):
    """the header's first consequence: Y, U and V as the gray infill of each plane with that plane's lens, times, output
    camera and fill -> ((y, u, v), n_outside (n, 2), n_borrowed (n, 2))"""
    from rssync_amd import synth
    p, d = scene["problem"], _planes(size)
    rows, cols = size
    kw = dict(kw)
    site, out_size, zoom = kw.pop("chroma_site"), kw.pop("out_size", None), kw.pop("zoom", 1.0)
    ocols, orows = (cols, rows) if out_size is None else out_size
    times, targets = zr.TIMES[sub], scene["targets"][sub]
    lens_c = cr.chroma_lens(d["lens"], site)
    times_c = np.array([cr.chroma_time(t, d["lens"], rows, site) for t in times])
    cam_c = cr.chroma_camera(d["lens"], rows, cols, orows, ocols, site, zoom)
    ckw = dict(out_size=(ocols // 2, orows // 2), out_camera=cam_c, **kw)
    y, n_y, b_y = p.stabilize_frames_infilled(d["y"][sub], times, d["lens"], synth.D_TRUE, radius, targets=targets, fill=fills[0],
                                              out_size=out_size, zoom=zoom, **kw)
    u, n_c, b_c = p.stabilize_frames_infilled(d["u"][sub], times_c, lens_c, synth.D_TRUE, radius, targets=targets, fill=fills[1], **ckw)
    v, n_v, b_v = p.stabilize_frames_infilled(d["v"][sub], times_c, lens_c, synth.D_TRUE, radius, targets=targets, fill=fills[2], **ckw)
    np.testing.assert_array_equal(n_v, n_c)
    np.testing.assert_array_equal(b_v, b_c)
    return (y, u, v), np.stack([n_y, n_c], axis=-1), np.stack([b_y, b_c], axis=-1)


_CACHE = {}


def _case(scene, name):
    """-> (the I420 device result, the three gray infills) of a case, computed once (read-only)"""
    from rssync_amd import color, synth
    if name not in _CACHE:
        size, kw = CASES[name]
        d = _planes(size)
        got = scene["problem"].stabilize_color_infilled(color.I420, (d["y"], d["u"], d["v"]), zr.TIMES, d["lens"], synth.D_TRUE, RADIUS,
                                                        targets=scene["targets"], fills=FILLS, **kw)
        want = _gray_planes(scene, size, kw)
        for a in got[0] + got[1:] + want[0] + want[1:]:
            a.setflags(write=False)
        _CACHE[name] = (got, want)
    return _CACHE[name]


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_i420_planes_are_the_gray_infill_of_each_plane(scene, name):
    got, want = _case(scene, name)
    planes, n_outside, n_borrowed = got
    print(name, "outside", n_outside.tolist(), "borrowed", n_borrowed.tolist())
    assert all(a.dtype == np.uint8 for a in planes) and n_outside.dtype == np.uint64 and n_borrowed.dtype == np.uint64
    assert n_outside.shape == n_borrowed.shape == (N, 2)
    _same(got, want)
    if name == FIRST:       # from the gray calls' own counts: the case is not vacuous
        _, w_out, w_lent = want
        assert (w_lent[:, 0] > 0).all() and (w_lent[:, 1] > 0).all(), w_lent.tolist()
        assert (w_out[:, 0] > 0).any() and (w_out[:, 1] > 0).any(), w_out.tolist()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_nv12_is_i420_with_the_chroma_interleaved(scene, name):
    from rssync_amd import color, synth
    ((y, u, v), n_outside, n_borrowed), _ = _case(scene, name)
    size, kw = CASES[name]
    d = _planes(size)
    got = scene["problem"].stabilize_color_infilled(color.NV12, (d["y"], d["uv"]), zr.TIMES, d["lens"], synth.D_TRUE, RADIUS,
                                                    targets=scene["targets"], fills=FILLS, **kw)
    _same(got, ((y, np.stack([u, v], axis=-1)), n_outside, n_borrowed))


@pytest.mark.parametrize("name", ["mid-lens-bicubic-left", "small-pinhole-bilinear-left", "mid-pinhole-resized-bicubic-center"])
def test_rgba_channels_are_the_gray_infill_with_the_luma_camera(scene, name):
    from rssync_amd import color, synth
    p = scene["problem"]
    size, kw = CASES[name]
    kw = {k: v for k, v in kw.items() if k != "chroma_site"}
    d = _planes(size)
    args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
    fills = (7, 99, 200, 31)
    got, n, nb = p.stabilize_color_infilled(color.RGBA32, d["rgba"], *args, targets=scene["targets"], fills=fills, fill=255, **kw)
    plain, plain_n, plain_nb = p.stabilize_color_infilled(color.RGBA32, d["rgba"], *args, targets=scene["targets"], fill=17, **kw)
    assert (n[:, 1] == 0).all() and (nb[:, 1] == 0).all() and nb[:, 0].sum() > 0
    for k in range(4):
        want, want_n, want_nb = p.stabilize_frames_infilled(d["rgba"][..., k], *args, targets=scene["targets"], fill=fills[k], **kw)
        np.testing.assert_array_equal(got[..., k], want, err_msg="channel %d" % k)
        np.testing.assert_array_equal(n[:, 0], want_n)
        np.testing.assert_array_equal(nb[:, 0], want_nb)
    # the default fills: A is 255
    np.testing.assert_array_equal(plain_n, n)
    np.testing.assert_array_equal(plain_nb, nb)
    want_a, _, _ = p.stabilize_frames_infilled(d["rgba"][..., 3], *args, targets=scene["targets"], fill=255, **kw)
    want_r, _, _ = p.stabilize_frames_infilled(d["rgba"][..., 0], *args, targets=scene["targets"], fill=17, **kw)
    np.testing.assert_array_equal(plain[..., 3], want_a)
    np.testing.assert_array_equal(plain[..., 0], want_r)


@pytest.mark.parametrize("name", list(CASES))
def test_gray8_is_the_gray_infill(scene, name):
    from rssync_amd import color, synth
    p = scene["problem"]
    size, kw = CASES[name]
    kw = {k: v for k, v in kw.items() if k != "chroma_site"}
    d = _planes(size)
    for targets in (scene["targets"], None):
        args = (d["y"], zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
        want, want_n, want_nb = p.stabilize_frames_infilled(*args, targets=targets, sigma=zr.SIGMA, fill=9, **kw)
        got, n, nb = p.stabilize_color_infilled(color.GRAY8, *args, targets=targets, sigma=zr.SIGMA, fill=9, **kw)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(n[:, 0], want_n)
        np.testing.assert_array_equal(nb[:, 0], want_nb)
        assert (n[:, 1] == 0).all() and (nb[:, 1] == 0).all() and want_nb.sum() > 0


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid-lens-bicubic-left", "mid-pinhole-resized-bicubic-center", "small-pinhole-bilinear-left",
                                  "scene-lens-bilinear-center"])
def test_16_bit_formats_on_8_bit_values_are_the_sibling_widened(scene, name):
    from rssync_amd import color, synth
    p = scene["problem"]
    ((y8, u8, v8), n8, nb8), _ = _case(scene, name)
    size, kw = CASES[name]
    d = _planes(size)
    y, u, v, uv = (d[k].astype(np.uint16) for k in ("y", "u", "v", "uv"))
    uv8 = np.stack([u8, v8], axis=-1)
    args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
    ckw = dict(targets=scene["targets"], fills=FILLS, **kw)
    assert nb8.min() > 0
    (y16, uv16), n16, nb16 = p.stabilize_color_infilled(color.P016, (y, uv), *args, **ckw)
    (y10, uv10), n10, nb10 = p.stabilize_color_infilled(color.P010, (y << 6, uv << 6), *args, **ckw)
    (yi, ui, vi), ni, nbi = p.stabilize_color_infilled(color.I010, (y, u, v), *args, **ckw)
    gkw = {k: v for k, v in kw.items() if k != "chroma_site"}
    g16, ng16, nbg16 = p.stabilize_color_infilled(color.GRAY16, y, *args, targets=scene["targets"], fills=(FILLS[0],), **gkw)
    assert (y10 & 63).max() == 0 and (uv10 & 63).max() == 0
    overshoot = 0
    for wide, narrow in ((y16, y8), (uv16, uv8), (y10 >> 6, y8), (uv10 >> 6, uv8), (yi, y8), (ui, u8), (vi, v8), (g16, y8)):
        assert wide.dtype == np.uint16 and wide.shape == narrow.shape
        if kw["filter"] == 0:
            np.testing.assert_array_equal(wide, narrow)
        else:   # the bicubic sampler clamps to the format's range: 255 may stand for more, every other value is the same
            assert ((wide == narrow) | ((narrow == 255) & (wide > 255))).all()
            overshoot += int((wide > 255).sum())
    assert (overshoot > 0) == (kw["filter"] == 1)
    for counts, want in (((n16, nb16), (n8, nb8)), ((n10, nb10), (n8, nb8)), ((ni, nbi), (n8, nb8))):
        np.testing.assert_array_equal(counts[0], want[0])
        np.testing.assert_array_equal(counts[1], want[1])
    np.testing.assert_array_equal(ng16[:, 0], n8[:, 0])
    np.testing.assert_array_equal(nbg16[:, 0], nb8[:, 0])
    assert (ng16[:, 1] == 0).all() and (nbg16[:, 1] == 0).all()


N16, RADIUS16 = 5, 2


def _compose16(p, fmt, frames, lens, targets, fills, **kw):
    """the header's second consequence through rssync_color16_stabilize: every frame g alone with time T_g and target
    targets[f], with two fills (the samples that differ are filled), merged per sample and per plane at the first candidate
    that does not fill it -> (planes, n_outside (n, 2), n_borrowed (n, 2)).  The chroma planes share one mask: U's.
    fills: sample values (P010's are stored << 6)."""
    from rssync_amd import color, synth
    top = (1 << color.DEPTH[fmt]) - 1
    n = N16
    outs, n_outside, n_borrowed = None, np.zeros((n, 2), np.uint64), np.zeros((n, 2), np.uint64)
    for f in range(n):
        done = None
        for k, g in enumerate(ir.candidates(f, n, RADIUS16)):
            one = tuple(a[g:g + 1] for a in frames)
            args = (fmt, one, zr.TIMES[g:g + 1], lens, synth.D_TRUE)
            a, _ = p.stabilize_color(*args, targets=targets[f:f + 1], fills=(0, 0, 0), **kw)
            b, _ = p.stabilize_color(*args, targets=targets[f:f + 1], fills=(top, top, top), **kw)
            if outs is None:
                shift = 6 if fmt == color.P010 else 0
                outs = [np.empty((n,) + x.shape[1:], np.uint16) for x in a]
                outs[0][:] = fills[0] << shift
                if len(a) == 2:         # P010, P016: the interleaved pairs
                    outs[1][..., 0], outs[1][..., 1] = fills[1] << shift, fills[2] << shift
                else:
                    outs[1][:], outs[2][:] = fills[1], fills[2]
            inside = [a[0][0] == b[0][0]] + [(a[1][0] == b[1][0]) if a[1].ndim == 3 else (a[1][0, ..., 0] == b[1][0, ..., 0])] * (len(a) - 1)
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
@pytest.mark.parametrize("size", [(38, 30), (330, 198)])
@pytest.mark.parametrize("fmt_name", ["P010", "I010"])
def test_true_10_bit_values_are_the_composition_of_single_frame_calls(scene, fmt_name, size, filter):
    from rssync_amd import color, synth
    p = scene["problem"]
    fmt = getattr(color, fmt_name)
    rows, cols = size
    rng = np.random.default_rng(rows + 17 * filter)
    y = rng.integers(0, 1024, size=(N16, rows, cols), dtype=np.uint16)
    u, v = (rng.integers(0, 1024, size=(N16, rows // 2, cols // 2), dtype=np.uint16) for _ in range(2))
    frames = (y << 6, np.stack([u, v], axis=-1) << 6) if fmt == color.P010 else (y, u, v)
    lens, targets, fills = rr.scaled_lens(rows, cols), scene["targets"][:N16], (5, 600, 700)
    kw = dict(filter=filter, camera=sr.LENS if filter else sr.PINHOLE, zoom=0.9, chroma_site=cr.LEFT if filter else cr.CENTER)
    got = p.stabilize_color_infilled(fmt, frames, zr.TIMES[:N16], lens, synth.D_TRUE, RADIUS16, targets=targets, fills=fills, **kw)
    want = _compose16(p, fmt, frames, lens, targets, fills, **kw)
    print(fmt_name, size, filter, "outside", want[1].tolist(), "borrowed", want[2].tolist())
    assert want[2][:, 0].sum() > 0 and want[2][:, 1].sum() > 0
    _same(got, want)


def test_true_16_bit_values_p016_and_gray16(scene):
    """the full sixteen bits through the same composition: P016's planes, and GRAY16 as P016's luma"""
    from rssync_amd import color, synth
    p = scene["problem"]
    rows, cols = 38, 30
    rng = np.random.default_rng(16)
    y = rng.integers(0, 65536, size=(N16, rows, cols), dtype=np.uint16)
    uv = rng.integers(0, 65536, size=(N16, rows // 2, cols // 2, 2), dtype=np.uint16)
    lens, targets, fills = rr.scaled_lens(rows, cols), scene["targets"][:N16], (5, 60000, 700)
    for filter in (0, 1):
        kw = dict(filter=filter, zoom=0.9)
        got = p.stabilize_color_infilled(color.P016, (y, uv), zr.TIMES[:N16], lens, synth.D_TRUE, RADIUS16, targets=targets, fills=fills, **kw)
        want = _compose16(p, color.P016, (y, uv), lens, targets, fills, **kw)
        assert want[2][:, 0].sum() > 0 and want[2][:, 1].sum() > 0
        _same(got, want)
        g, n, nb = p.stabilize_color_infilled(color.GRAY16, y, zr.TIMES[:N16], lens, synth.D_TRUE, RADIUS16, targets=targets, fills=fills[:1], **kw)
        np.testing.assert_array_equal(g, want[0][0])
        np.testing.assert_array_equal(n[:, 0], want[1][:, 0])
        np.testing.assert_array_equal(nb[:, 0], want[2][:, 0])


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["path", "targets"])
@pytest.mark.parametrize("fmt_name", ["NV12", "I420", "RGBA32", "P010", "GRAY16"])
def test_radius_zero_and_a_single_frame_are_the_colour_stabiliser(scene, fmt_name, explicit):
    from rssync_amd import color, synth
    p = scene["problem"]
    fmt = getattr(color, fmt_name)
    d = _planes((330, 198))
    frames = {"NV12": (d["y"], d["uv"]), "I420": (d["y"], d["u"], d["v"]), "RGBA32": d["rgba"],
              "P010": (d["y"].astype(np.uint16) << 8, d["uv"].astype(np.uint16) << 8), "GRAY16": d["y"].astype(np.uint16) * 257}[fmt_name]
    many = isinstance(frames, tuple)
    for filter in (0, 1):
        kw = dict(sigma=zr.SIGMA, fill=FILLS[0], filter=filter)
        t = scene["targets"] if explicit else None
        want, want_n = p.stabilize_color(fmt, frames, zr.TIMES, d["lens"], synth.D_TRUE, targets=t, **kw)
        assert want_n[:, 0].sum() > 0
        got = p.stabilize_color_infilled(fmt, frames, zr.TIMES, d["lens"], synth.D_TRUE, 0, targets=t, **kw)
        _same(got, (want, want_n, np.zeros((N, 2), np.uint64)))
        for f in (0, 5):
            one = tuple(a[f:f + 1] for a in frames) if many else frames[f:f + 1]
            got = p.stabilize_color_infilled(fmt, one, zr.TIMES[f:f + 1], d["lens"], synth.D_TRUE, RADIUS, targets=None if t is None else t[f:f + 1],
                                             **kw)
            w = tuple(a[f:f + 1] for a in want) if many else want[f:f + 1]
            _same(got, (w, want_n[f:f + 1], np.zeros((1, 2), np.uint64)))


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4, 8])
def test_a_frame_depends_on_its_neighbourhood_alone(scene, f):
    from rssync_amd import color, synth
    ((y, u, v), n, nb), _ = _case(scene, FIRST)
    size, kw = CASES[FIRST]
    d = _planes(size)
    lo, hi = max(0, f - RADIUS), min(N - 1, f + RADIUS)
    sub = slice(lo, hi + 1)
    (gy, gu, gv), gn, gnb = scene["problem"].stabilize_color_infilled(color.I420, (d["y"][sub], d["u"][sub], d["v"][sub]), zr.TIMES[sub], d["lens"],
                                                                      synth.D_TRUE, RADIUS, targets=scene["targets"][sub], fills=FILLS, **kw)
    for a, b in ((gy, y), (gu, u), (gv, v)):
        np.testing.assert_array_equal(a[f - lo], b[f])
    np.testing.assert_array_equal(gn[f - lo], n[f])
    np.testing.assert_array_equal(gnb[f - lo], nb[f])


# 6 ---------------------------------------------------------------------------------------------------------------------
def _slot_bytes(frames_per_chunk):
    """a budget whose half pays for the halo of RADIUS frames on each side and that many frames of the scene's 4:2:0 size:
    2 radius + 1 tables of both regions, the input and the output planes"""
    rows, cols = SCENE
    image = rows * cols * 3 // 2
    per_frame = (2 * RADIUS + 1) * ((rows + 1) * 36 + (rows // 2 + 1) * 36) + 2 * image
    return 2 * (2 * RADIUS * image + frames_per_chunk * per_frame)


@pytest.mark.parametrize("fmt_name", ["NV12", "I420"])
@pytest.mark.parametrize("budget", [1000, _slot_bytes(2.5), _slot_bytes(4.5)], ids=["one-frame", "two-frames", "four-frames"])
def test_chunks_with_halos(scene, fmt_name, budget):
    from rssync_amd import color, synth
    ((y, u, v), n, nb), _ = _case(scene, FIRST)
    size, kw = CASES[FIRST]
    d = _planes(size)
    nv12 = fmt_name == "NV12"
    frames = (d["y"], d["uv"]) if nv12 else (d["y"], d["u"], d["v"])
    got = scene["problem"].stabilize_color_infilled_budget(getattr(color, fmt_name), frames, zr.TIMES, d["lens"], synth.D_TRUE, RADIUS, budget,
                                                           targets=scene["targets"], fills=FILLS + (0,), **kw)
    _same(got, ((y, np.stack([u, v], axis=-1)) if nv12 else (y, u, v), n, nb))


def test_pitched_views_and_device_memory(scene):
    from rssync_amd import color, synth
    p = scene["problem"]
    ((y, u, v), n, nb), _ = _case(scene, FIRST)
    size, kw = CASES[FIRST]
    rows, cols = size
    d = _planes(size)
    want = ((y, np.stack([u, v], axis=-1)), n, nb)
    want3 = ((y, u, v), n, nb)
    args = (zr.TIMES, d["lens"], synth.D_TRUE, RADIUS)
    ckw = dict(targets=scene["targets"], fills=FILLS, **kw)
    # device-resident tensors: NV12 and I420
    dev = (torch.from_numpy(np.array(d["y"])).to("cuda:0"), torch.from_numpy(np.array(d["uv"])).to("cuda:0"))
    got = p.stabilize_color_infilled(color.NV12, dev, *args, **ckw)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in got[0])
    _same(got, want)
    dev3 = (dev[0], torch.from_numpy(np.array(d["u"])).to("cuda:0"), torch.from_numpy(np.array(d["v"])).to("cuda:0"))
    _same(p.stabilize_color_infilled(color.I420, dev3, *args, **ckw), want3)
    # host in, device out; device in, host out
    dout = (torch.zeros((N, rows, cols), dtype=torch.uint8, device="cuda:0"), torch.zeros((N, rows // 2, cols // 2, 2), dtype=torch.uint8, device="cuda:0"))
    got = p.stabilize_color_infilled(color.NV12, (d["y"], d["uv"]), *args, out=dout, **ckw)
    assert got[0] is dout
    _same(got, want)
    hout = (np.zeros((N, rows, cols), np.uint8), np.zeros((N, rows // 2, cols // 2, 2), np.uint8))
    _same(p.stabilize_color_infilled(color.NV12, dev, *args, out=hout, **ckw), want)
    # device frames through chunks: the neighbours are read in place
    _same(p.stabilize_color_infilled_budget(color.NV12, dev, *args, 1000, out=hout, targets=scene["targets"], fills=FILLS + (0,), **kw), want)
    # pitched device buffers, a guard pattern between the rows of the result
    wide_y = np.zeros((N, rows + 2, cols + 61), np.uint8)
    wide_y[:, 1:1 + rows, 13:13 + cols] = d["y"]
    wide_uv = np.zeros((N, rows // 2 + 1, cols // 2 + 9, 2), np.uint8)
    wide_uv[:, 1:, 4:4 + cols // 2] = d["uv"]
    dwide = (torch.from_numpy(wide_y).to("cuda:0")[:, 1:1 + rows, 13:13 + cols], torch.from_numpy(wide_uv).to("cuda:0")[:, 1:, 4:4 + cols // 2])
    dy = torch.full((N, rows + 3, cols + 19), 201, dtype=torch.uint8, device="cuda:0")
    duv = torch.full((N, rows // 2 + 1, cols // 2 + 5, 2), 202, dtype=torch.uint8, device="cuda:0")
    views = (dy[:, 2:2 + rows, 3:3 + cols], duv[:, :rows // 2, 2:2 + cols // 2])
    res, gn, gnb = p.stabilize_color_infilled(color.NV12, dwide, *args, out=views, **ckw)
    assert res is views
    by, buv = dy.cpu().numpy(), duv.cpu().numpy()
    _same(((by[:, 2:2 + rows, 3:3 + cols], buv[:, :rows // 2, 2:2 + cols // 2]), gn, gnb), want)
    gy, guv = np.ones(by.shape, bool), np.ones(buv.shape, bool)
    gy[:, 2:2 + rows, 3:3 + cols] = False
    guv[:, :rows // 2, 2:2 + cols // 2] = False
    assert (by[gy] == 201).all() and (buv[guv] == 202).all()
    # pitched host buffers, the same way, I420
    wide_u = np.zeros((N, rows // 2, cols // 2 + 7), np.uint8)
    wide_u[:, :, 3:3 + cols // 2] = d["u"]
    wide_v = np.zeros((N, rows // 2 + 2, cols // 2), np.uint8)
    wide_v[:, 2:] = d["v"]
    hy = np.full((N, rows + 1, cols + 5), 9, np.uint8)
    hu = np.full((N, rows // 2, cols // 2 + 3), 8, np.uint8)
    hv = np.full((N, rows // 2 + 1, cols // 2), 7, np.uint8)
    _, gn, gnb = p.stabilize_color_infilled(color.I420, (wide_y[:, 1:1 + rows, 13:13 + cols], wide_u[:, :, 3:3 + cols // 2], wide_v[:, 2:]), *args,
                                            out=(hy[:, :rows, 2:2 + cols], hu[:, :, 1:1 + cols // 2], hv[:, :rows // 2]), **ckw)
    _same(((hy[:, :rows, 2:2 + cols], hu[:, :, 1:1 + cols // 2], hv[:, :rows // 2]), gn, gnb), want3)
    assert (hy[:, rows:] == 9).all() and (hy[:, :, :2] == 9).all() and (hy[:, :, 2 + cols:] == 9).all()
    assert (hu[:, :, :1] == 8).all() and (hu[:, :, 1 + cols // 2:] == 8).all() and (hv[:, rows // 2:] == 7).all()
    # planes of one image must be of one kind
    with pytest.raises(color.RsSyncError, match="mixed kinds"):
        p.stabilize_color_infilled(color.NV12, (dev[0], d["uv"]), *args, **ckw)
    _same(p.stabilize_color_infilled(color.NV12, dev, *args, **ckw), want)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene):
    from rssync_amd import color, colorinfill, synth
    p = scene["problem"]
    size, kw = CASES["mid-lens-bicubic-left"]
    rows, cols = size
    d = _planes(size)
    ((wy, wu, wv), wn, wnb), _ = _case(scene, "mid-lens-bicubic-left")
    want = ((wy, np.stack([wu, wv], axis=-1)), wn, wnb)
    lib = colorinfill.library()
    lib.rssync_set_panic_mode(1)
    PD, PU64 = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    L = np.ascontiguousarray(d["lens"], np.float64)
    T = np.ascontiguousarray(zr.TIMES)
    Q = np.ascontiguousarray(scene["targets"])
    prm = color.params(kw["chroma_site"], FILLS, camera=kw["camera"], filter=kw["filter"])
    y, uv = np.ascontiguousarray(d["y"]), np.ascontiguousarray(d["uv"])
    oy, ouv = np.zeros_like(y), np.zeros_like(uv)
    n, nb = np.zeros((N, 2), np.uint64), np.zeros((N, 2), np.uint64)

    def image(a, b, w, h, second=True):
        img = color.ColorImage()
        img.plane[0], img.pitch[0], img.stride[0] = a.ctypes.data, w, w * h
        if second:
            img.plane[1], img.pitch[1], img.stride[1] = b.ctypes.data, w, w * h // 2
        return img

    def call(radius=RADIUS, w=cols, h=rows, second=True, fmt=color.NV12):
        src, dst = image(y, uv, cols, rows, second), image(oy, ouv, cols, rows)
        return lib.rssync_colorinfill_stabilize(p._h, fmt, C.byref(src), N, w, h, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE,
                                                Q.ctypes.data_as(PD), C.byref(prm), C.byref(dst), w, h, n.ctypes.data_as(PU64), radius,
                                                nb.ctypes.data_as(PU64))

    for match, bad in (("radius", dict(radius=-1)), ("radius", dict(radius=9)), ("even width", dict(w=cols - 1)), ("even width", dict(h=rows - 1)),
                       ("is NULL", dict(second=False)), ("format", dict(fmt=7))):
        assert call(**bad) != 0, bad
        msg = lib.rssync_last_error().decode()
        assert match in msg and msg.startswith(("colorinfill: ", "color: ")), (match, msg)
        assert call() == 0, lib.rssync_last_error().decode()
        _same(((oy, ouv), n, nb), want)
    assert call(radius=8) == 0 and call(radius=0) == 0
    # the Python wrapper: its own checks raise before the library is called, the library's arrive as RsSyncError
    args = (color.NV12, (y, uv), zr.TIMES, d["lens"], synth.D_TRUE)
    with pytest.raises(colorinfill.RsSyncError, match="radius"):
        p.stabilize_color_infilled(*args, 9)
    for bad in (np.zeros((N,), np.uint64), np.zeros((N + 1, 2), np.uint64), np.zeros((N, 2), np.int32)):
        with pytest.raises(ValueError, match="n_borrowed"):
            p.stabilize_color_infilled(*args, RADIUS, n_borrowed=bad)
    mine = np.zeros((N, 2), np.uint64)
    got = p.stabilize_color_infilled(*args, RADIUS, targets=scene["targets"], fills=FILLS, n_borrowed=mine, **kw)
    assert got[2].base is mine or got[2] is mine
    _same(got, want)


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_borrowed_samples_against_the_global_shutter_truth(scene):
    """Mean absolute grey difference to the truth over the samples the device borrowed, frames 32, 33, 34, per plane Y, U, V:
    within cir.error_margin -- what positions that lie within the colour front's device tolerance (cr.device_tolerance) of
    the restatement's can move the figure by -- of the float64 restatement's cir.BORROWED_ERROR, and far below the constant
    fill's cir.FILL_ERROR; at least cir.MIN_BORROWED_SHARE of the outside samples borrowed."""
    from rssync_amd import color, synth
    p, lens = scene["problem"], scene["lens"]
    y, u, v, times = cir.video()
    targets = ir.video_targets()
    args = (color.I420, (y, u, v), times, lens, synth.D_TRUE)
    own0, own_n = p.stabilize_color(*args, targets=targets, fills=(0, 0, 0))
    own255, _ = p.stabilize_color(*args, targets=targets, fills=(255, 255, 255))
    out, n, nb = p.stabilize_color_infilled(*args, cir.RADIUS, targets=targets, fills=(0, 0, 0))
    out255, _, _ = p.stabilize_color_infilled(*args, cir.RADIUS, targets=targets, fills=(255, 255, 255))
    truth = (sr.truth(),) + tuple(cr.truth())
    for k, f in enumerate(range(*ir.VIDEO_SCENE.indices(len(times)))):
        for pl, name in enumerate("YUV"):
            col = min(pl, 1)
            outside = own0[pl][f] != own255[pl][f]
            lent = outside & (out[pl][f] == out255[pl][f])
            assert outside.sum() == own_n[f, col] and lent.sum() == nb[f, col] and own_n[f, col] == n[f, col] + nb[f, col]
            err = float(np.abs(out[pl][f].astype(np.float64) - truth[pl][k].astype(np.float64))[lent].mean())
            share = float(nb[f, col]) / float(own_n[f, col])
            print("%s frame %d: %d of %d outside samples borrowed (%.4f; reference %d of %d), error %.3f (reference %.3f, fill %.1f)" %
                  (name, rr.F0 + k, nb[f, col], own_n[f, col], share, cir.SEEN[pl][k], cir.OUTSIDE[pl][k], err, cir.BORROWED_ERROR[pl][k],
                   cir.FILL_ERROR[pl][k]))
            assert abs(err - cir.BORROWED_ERROR[pl][k]) <= cir.error_margin(pl, k), (name, k, err, cir.error_margin(pl, k))
            assert err <= cir.FAR_BELOW * cir.FILL_ERROR[pl][k], (name, k, err)
            assert share >= cir.MIN_BORROWED_SHARE[pl], (name, k, share)
