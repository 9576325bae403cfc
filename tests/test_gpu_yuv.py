"""The 4:2:2 and 4:4:4 formats on the device (include/rssync_yuv.h, csrc/kernels/yuv.hpp) against the stabiliser they are
defined by -- every plane is rssync_stabilize_frames of that plane with that plane's camera, byte for byte --, their numpy
restatement (tests/yuv_reference.py) and global-shutter renders of the 4:2:2 scene at the smoothed path's orientations."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color16_reference as c16
import rectify_reference as rr
import resample_reference as rsr
import stabilize_reference as sr
import yuv_reference as yr

pytestmark = pytest.mark.gpu

# luma (rows, cols): the smallest 4:2:2 frame with an odd height; 65 chroma columns and 5 rows, one past a 64 x 4 tile each
# way; two sizes that are no multiple of the tile; the scene's.  4:4:4 adds a frame that is odd both ways.
SIZES = [(3, 4), (5, 130), (31, 38), (199, 330), (rr.ROWS, rr.COLS)]
SIZES444 = SIZES + [(3, 5)]
OUT = (131, 198)        # rows, cols of the other output size
ZOOMS = (0.8, 1.3)
SITES = [yr.CENTER, yr.LEFT]
CAMERAS = [sr.LENS, sr.PINHOLE]
FILTERS = [0, 1]        # bilinear, bicubic
N = 2                   # frames of the byte-for-byte cases


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
def planes():
    """per luma size: lens and N frames of Y, the 4:2:2 planes U, V (rows x cols / 2; the scene's at its size, noise
    elsewhere) and the 4:4:4 planes U4, V4 (noise) (read-only)"""
    out = {}
    col = yr.scene()
    for rows, cols in SIZES444:
        rng = np.random.default_rng(rows * 1000 + cols)
        if (rows, cols) == (rr.ROWS, rr.COLS):
            y, u, v = (np.array(col[k][:N]) for k in ("y", "u", "v"))
        else:
            y = rng.integers(0, 256, size=(N, rows, cols), dtype=np.uint8)
            u, v = (rng.integers(0, 256, size=(N, rows, cols // 2), dtype=np.uint8) for _ in range(2))
        u4, v4 = (rng.integers(0, 256, size=(N, rows, cols), dtype=np.uint8) for _ in range(2))
        d = dict(lens=rr.scaled_lens(rows, cols), y=y, u=u, v=v, uv=np.stack([u, v], axis=-1), u4=u4, v4=v4)
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(rows, cols)] = d
    return out


@pytest.fixture(scope="module")
def wide_planes():
    """three frames of the scene's size with random samples of 10 and of 16 bits and patches of 0 and of the maximum
    (read-only): {depth: (y, u 4:2:2, v 4:2:2, u 4:4:4, v 4:4:4)}"""
    out = {}
    for depth in (10, 16):
        rng = np.random.default_rng(100 + depth)
        top = (1 << depth) - 1
        y, u4, v4 = (rng.integers(0, top + 1, size=(rr.N_FRAMES, rr.ROWS, rr.COLS), dtype=np.uint16) for _ in range(3))
        u, v = (rng.integers(0, top + 1, size=(rr.N_FRAMES, yr.C_ROWS, yr.C_COLS), dtype=np.uint16) for _ in range(2))
        for a, s in ((y, 2), (u4, 2), (v4, 2), (u, 1), (v, 1)):
            a[:, 80:140, 50 * s:120 * s] = 0
            a[:, 180:260, 100 * s:250 * s] = top
            a[:, 120:200, 180 * s:200 * s] = top                 # (beside the zeros: taps of both extremes)
            a[:, :6, :] = top                                    # (the first rows and the last columns: the clamped taps)
            a[:, :, -3 * s:] = 0
            a.setflags(write=False)
        out[depth] = (y, u, v, u4, v4)
    return out


def _outs(rows, cols):
    """(out_size argument (cols, rows), out rows, out cols): the input's size and OUT"""
    return [(None, rows, cols), ((OUT[1], OUT[0]), OUT[0], OUT[1])]


def _targets(scene, n=N):
    """explicit targets as tests/test_gpu_color.py forms them: another smoothing's orientations, not of unit length"""
    from rssync_amd import synth
    return 2.5 * sr.path64(scene["gyro"], scene["times"][:n], scene["lens"][0], synth.D_TRUE, 0.3)


def _uv(u, v):
    return np.stack([u, v], axis=-1)


def _frames(fmt, d, widen=True):
    """the planes of dict d in the layout of `fmt`; a 16-bit format gets the 8-bit values widened (P210: << 6)"""
    from rssync_amd import yuv
    sib = yuv.SIBLING.get(fmt, fmt)
    fr = {yuv.I422: (d["y"], d["u"], d["v"]), yuv.NV16: (d["y"], d["uv"]), yuv.I444: (d["y"], d["u4"], d["v4"])}[sib]
    if fmt in yuv.SIBLING and widen:
        fr = tuple(a.astype(np.uint16) << (6 if fmt == yuv.P210 else 0) for a in fr)
    return fr


def _formats(cols):
    from rssync_amd import yuv
    f444 = [yuv.I444, yuv.I410]
    return f444 + ([yuv.I422, yuv.NV16, yuv.I210, yuv.P210, yuv.P216] if cols % 2 == 0 else [])


def _check_both(outside, total, what):
    """a byte-for-byte case holds inside and outside samples over its zooms together"""
    assert 0 < outside < total, (what, outside, total)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("camera", CAMERAS)
def test_luma_plane_is_the_stabiliser_byte_for_byte(scene, planes, camera, filt):
    """the luma plane of every format and its count are rssync_stabilize_frames', and rssync_yuv_map's plane 0 is
    rssync_stabilize_map bit for bit.  A format in a 16-bit container gets the 8-bit values widened (P210: << 6) and gives
    the stabiliser's bytes widened: with the bilinear sampler everywhere; with the bicubic one wherever the stabiliser's
    byte is below 255, since its clamp is the 8-bit range's and theirs the container's (there the value is 255 or above).
    Both zooms at every size and output: together they hold inside and outside samples, luma and chroma."""
    from rssync_amd import synth, yuv
    p, times = scene["problem"], scene["times"][:N]
    for size in SIZES444:
        rows, cols = size
        d = planes[size]
        for out_size, orows, ocols in _outs(*size):
            outside = outside_c = 0
            for zoom in ZOOMS:
                kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, zoom=zoom, filter=filt)
                name = "%s -> %s zoom %.1f" % (size, out_size, zoom)
                want, want_n = p.stabilize_frames(d["y"], times, d["lens"], synth.D_TRUE, fill=3, **kw)
                want_map = p.stabilize_map(cols, rows, d["lens"], times[1], synth.D_TRUE, **kw).view(np.uint32)
                for fmt in _formats(cols):
                    res, n = p.stabilize_yuv(fmt, _frames(fmt, d), times, d["lens"], synth.D_TRUE, fills=(3, 128, 128), **kw)
                    luma = res[0]
                    assert luma.shape == (N, orows, ocols)
                    if fmt in yuv.SIBLING:
                        shift = 6 if fmt == yuv.P210 else 0
                        assert luma.dtype == np.uint16 and (luma & ((1 << shift) - 1)).max() == 0
                        luma = luma >> shift
                        if filt == 1:
                            top = want == 255
                            assert (luma[top] >= 255).all(), "format %d %s" % (fmt, name)
                            luma = np.where(top, 255, luma)
                    np.testing.assert_array_equal(luma, want, err_msg="format %d %s" % (fmt, name))
                    np.testing.assert_array_equal(n[:, 0], want_n)
                    got = p.yuv_map(fmt, 0, cols, rows, d["lens"], times[1], synth.D_TRUE, **kw)
                    np.testing.assert_array_equal(got.view(np.uint32), want_map)
                    if fmt == (yuv.NV16 if cols % 2 == 0 else yuv.I444):
                        outside_c += int(n[:, 1].sum())
                outside += int(want_n.sum())
            _check_both(outside, len(ZOOMS) * N * orows * ocols, ("luma", size, out_size))
            _check_both(outside_c, len(ZOOMS) * N * orows * (ocols // 2 if cols % 2 == 0 else ocols), ("chroma", size, out_size))


# 2, 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_422_chroma_planes_are_the_stabiliser_with_the_chroma_camera(scene, planes, site, camera, filt):
    """explicit targets: plane 1's map is rssync_stabilize_map of the chroma lens, T and the chroma output camera bit for
    bit, and U and V are rssync_stabilize_frames of those planes byte for byte, with the count.  NV16's chroma is I422's,
    interleaved.  Both zooms at every size and output: together they hold inside and outside samples."""
    from rssync_amd import synth, yuv
    p, times, targets = scene["problem"], scene["times"][:N], _targets(scene)
    for size in SIZES:
        rows, cols = size
        d = planes[size]
        lens_c = yr.chroma_lens422(d["lens"], site)
        for out_size, orows, ocols in _outs(*size):
            outside = total = 0
            for zoom in ZOOMS:
                cam_c = yr.chroma_camera422(d["lens"], rows, cols, orows, ocols, site, zoom)
                kw = dict(camera=camera, iterations=3)
                ckw = dict(out_size=(ocols // 2, orows), out_camera=cam_c, **kw)
                name = "%s -> %s zoom %.1f" % (size, out_size, zoom)
                got = p.yuv_map(yuv.NV16, 1, cols, rows, d["lens"], times[1], synth.D_TRUE, target=targets[1], out_size=out_size, zoom=zoom,
                                chroma_site=site, **kw)
                want = p.stabilize_map(cols // 2, rows, lens_c, times[1], synth.D_TRUE, target=targets[1], **ckw)
                assert got.shape == (orows, ocols // 2, 2)
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=name)
                ykw = dict(targets=targets, out_size=out_size, zoom=zoom, chroma_site=site, fills=(0, 55, 66), filter=filt, **kw)
                (y1, u, v), n_out = p.stabilize_yuv(yuv.I422, (d["y"], d["u"], d["v"]), times, d["lens"], synth.D_TRUE, **ykw)
                want_u, want_n = p.stabilize_frames(d["u"], times, lens_c, synth.D_TRUE, targets=targets, fill=55, filter=filt, **ckw)
                want_v, _ = p.stabilize_frames(d["v"], times, lens_c, synth.D_TRUE, targets=targets, fill=66, filter=filt, **ckw)
                assert u.shape == v.shape == (N, orows, ocols // 2)
                np.testing.assert_array_equal(u, want_u, err_msg="U " + name)
                np.testing.assert_array_equal(v, want_v, err_msg="V " + name)
                np.testing.assert_array_equal(n_out[:, 1], want_n)
                (y2, uv), n2 = p.stabilize_yuv(yuv.NV16, (d["y"], d["uv"]), times, d["lens"], synth.D_TRUE, **ykw)
                assert uv.shape == (N, orows, ocols // 2, 2)
                np.testing.assert_array_equal(uv, _uv(u, v), err_msg="NV16 " + name)
                np.testing.assert_array_equal(y2, y1)
                np.testing.assert_array_equal(n2, n_out)
                outside += int(n_out[:, 1].sum())
                total += N * orows * (ocols // 2)
            _check_both(outside, total, (size, out_size))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("camera", CAMERAS)
def test_444_chroma_planes_are_the_stabiliser_with_the_lumas_camera(scene, planes, camera, filt):
    """explicit targets: U and V of I444 are rssync_stabilize_frames of those planes with the luma's camera, both counts are
    equal, plane 1's map is plane 0's, and chroma_site changes nothing"""
    from rssync_amd import synth, yuv
    p, times, targets = scene["problem"], scene["times"][:N], _targets(scene)
    for size in SIZES444:
        rows, cols = size
        d = planes[size]
        for out_size, orows, ocols in _outs(*size):
            outside = total = 0
            for zoom in ZOOMS:
                kw = dict(targets=targets, out_size=out_size, zoom=zoom, camera=camera, filter=filt)
                res, n_out = p.stabilize_yuv(yuv.I444, (d["y"], d["u4"], d["v4"]), times, d["lens"], synth.D_TRUE, fills=(9, 55, 66), **kw)
                for k, (name, fill) in enumerate((("y", 9), ("u4", 55), ("v4", 66))):
                    want, want_n = p.stabilize_frames(d[name], times, d["lens"], synth.D_TRUE, fill=fill, **kw)
                    assert res[k].shape == (N, orows, ocols)
                    np.testing.assert_array_equal(res[k], want, err_msg="%s %s -> %s zoom %.1f" % (name, size, out_size, zoom))
                    np.testing.assert_array_equal(n_out[:, 0], want_n)
                np.testing.assert_array_equal(n_out[:, 1], n_out[:, 0])
                left, n_left = p.stabilize_yuv(yuv.I444, (d["y"], d["u4"], d["v4"]), times, d["lens"], synth.D_TRUE, fills=(9, 55, 66),
                                               chroma_site=yr.LEFT, **kw)
                for a, b in zip(left, res):
                    np.testing.assert_array_equal(a, b)
                mkw = dict(target=targets[1], out_size=out_size, zoom=zoom, camera=camera)
                m0 = p.yuv_map(yuv.I444, 0, cols, rows, d["lens"], times[1], synth.D_TRUE, **mkw)
                m1 = p.yuv_map(yuv.I444, 1, cols, rows, d["lens"], times[1], synth.D_TRUE, **mkw)
                np.testing.assert_array_equal(m0.view(np.uint32), m1.view(np.uint32))
                outside += int(n_out[:, 1].sum())
                total += N * orows * ocols
            _check_both(outside, total, (size, out_size))


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_on_8_bit_values_every_16_bit_format_is_its_sibling_widened(scene, planes, site, camera):
    """tests/test_gpu_color16.py's anchor for these formats: the widened planes through I210, P210 (fed << 6), P216 and
    I410 give the sibling's bytes widened (P210: << 6) and the sibling's counts, with the same fills, along the path.  Both
    zooms at every size and output: together they hold inside and outside samples, luma and chroma."""
    from rssync_amd import synth, yuv
    p, times = scene["problem"], scene["times"][:N]
    for size in SIZES444:
        d = planes[size]
        even = size[1] % 2 == 0
        for out_size, orows, ocols in _outs(*size):
            outside = outside_c = 0
            for zoom in ZOOMS:
                kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, zoom=zoom, chroma_site=site, fills=(1, 2, 3))
                args = (times, d["lens"], synth.D_TRUE)
                got8 = {}
                for fmt in _formats(size[1]):
                    if fmt not in yuv.SIBLING:
                        got8[fmt] = p.stabilize_yuv(fmt, _frames(fmt, d), *args, **kw)
                for fmt in _formats(size[1]):
                    if fmt not in yuv.SIBLING:
                        continue
                    res, n = p.stabilize_yuv(fmt, _frames(fmt, d), *args, **kw)
                    res8, n8 = got8[yuv.SIBLING[fmt]]
                    for a, b in zip(res, res8):
                        assert a.dtype == np.uint16 and a.shape == b.shape
                        np.testing.assert_array_equal(a, b.astype(np.uint16) << (6 if fmt == yuv.P210 else 0),
                                                      err_msg="format %d %s -> %s zoom %.1f" % (fmt, size, out_size, zoom))
                    np.testing.assert_array_equal(n, n8)
                n8 = got8[yuv.NV16 if even else yuv.I444][1]
                outside += int(n8[:, 0].sum())
                outside_c += int(n8[:, 1].sum())
            _check_both(outside, len(ZOOMS) * N * orows * ocols, ("luma", size, out_size))
            _check_both(outside_c, len(ZOOMS) * N * orows * (ocols // 2 if even else ocols), ("chroma", size, out_size))


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("camera", CAMERAS)
def test_full_range_against_the_restatement_on_the_devices_own_map(scene, wide_planes, camera, filt):
    """random 10- and 16-bit samples with patches of 0 and of the maximum: every output plane is the restated sampler
    (c16.sample16, rsr.sample_bicubic with the format's clamp) applied to the device's own map of that plane, and the
    counts are that map's.  Zoom 0.8 so that both cameras fill samples; distinct fills per plane; P210's words keep their
    low six bits zero."""
    from rssync_amd import synth, yuv
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    fills = {10: (1001, 77, 888), 16: (60001, 777, 43210)}
    site = yr.LEFT

    def sample(vals, m, fill, vmax):
        return c16.sample16(vals, m, fill) if filt == 0 else rsr.sample_bicubic(np.ascontiguousarray(vals), m, fill, vmax)

    for out_size, orows, ocols in _outs(rr.ROWS, rr.COLS):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, chroma_site=site, zoom=0.8)
        maps = [[p.yuv_map(yuv.NV16, pl, rr.COLS, rr.ROWS, lens, t, synth.D_TRUE, **kw) for pl in (0, 1)] for t in times]
        for fmt, depth, shift in ((yuv.I210, 10, 0), (yuv.P210, 10, 6), (yuv.P216, 16, 0), (yuv.I410, 10, 0)):
            y, u, v, u4, v4 = wide_planes[depth]
            top = (1 << depth) - 1
            is444 = fmt == yuv.I410
            vals = (y, u4, v4) if is444 else (y, u, v)
            frames = vals if fmt in (yuv.I210, yuv.I410) else (y << shift, _uv(u, v) << shift)
            res, n_out = p.stabilize_yuv(fmt, frames, times, lens, synth.D_TRUE, fills=fills[depth], filter=filt, **kw)
            if fmt in (yuv.P210, yuv.P216):
                assert (res[0] & ((1 << shift) - 1)).max() == 0 and (res[1] & ((1 << shift) - 1)).max() == 0
                res = (res[0] >> shift, res[1][..., 0] >> shift, res[1][..., 1] >> shift)
            for k in range(rr.N_FRAMES):
                for pl in range(3):
                    m = maps[k][0 if (pl == 0 or is444) else 1]
                    want, cnt = sample(vals[pl][k], m, fills[depth][pl], top)
                    np.testing.assert_array_equal(res[pl][k], want, err_msg="format %d plane %d frame %d out %s" % (fmt, pl, k, out_size))
                    assert int(n_out[k, min(pl, 1)]) == cnt > 0


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("site", SITES)
def test_422_chroma_along_the_path_against_the_restatement(scene, site, camera):
    """targets = NULL: the chroma bytes are the restated sampler's from the device's own plane-1 map, the count is that
    map's, and the map is within the tolerance of the float64 restatement: four times the float32 restatement's spread
    (yr.device_tolerance, from the reference alone).  Both output sizes, zoom 0.8: both cameras fill samples there."""
    from rssync_amd import synth, yuv
    import color_reference as cr
    p, g, lens, times = scene["problem"], scene["gyro"], scene["lens"], scene["times"]
    col = yr.scene(site)
    tol = yr.device_tolerance(camera)
    for out_size, orows, ocols in _outs(rr.ROWS, rr.COLS):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera, chroma_site=site, zoom=0.8)
        (_, uv), n_out = p.stabilize_yuv(yuv.NV16, (col["y"], col["uv"]), times, lens, synth.D_TRUE, fills=(0, 77, 88), **kw)
        for k in range(rr.N_FRAMES):
            m = p.yuv_map(yuv.NV16, 1, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw)
            want, want_n = cr.sample_pairs(col["uv"][k], m, fill=(77, 88))
            np.testing.assert_array_equal(uv[k], want, err_msg="frame %d" % k)
            assert int(n_out[k, 1]) == want_n == int((~sr.inside(m, yr.C_ROWS, yr.C_COLS)).sum()) > 0
            ref = yr.chroma_map64(g, lens, rr.ROWS, rr.COLS, times[k], synth.D_TRUE, site, sigma=sr.SIGMA, out_size=out_size, camera=camera,
                                  zoom=0.8)
            diff = np.abs(m.astype(np.float64) - ref).max()
            print("site %d camera %d out %s frame %d: %.3g chroma px (tolerance %.3g), %d outside" % (site, camera, out_size, k, diff, tol, n_out[k, 1]))
            assert diff <= tol


# 8 ---------------------------------------------------------------------------------------------------------------------
def _against_truth(name, img, ok, m, ref_img, ref_map, raw, truth, rows, cols, tol):
    """tests/test_gpu_color.py's four rules"""
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
    from rssync_amd import synth, yuv
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col, truth_uv = yr.scene(site), yr.truth(site)
    kw = dict(sigma=sr.SIGMA, chroma_site=site)
    (y, uv), _ = p.stabilize_yuv(yuv.NV16, (col["y"], col["uv"]), times, lens, synth.D_TRUE, **kw)
    for k in range(rr.N_FRAMES):
        m = p.yuv_map(yuv.NV16, 0, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw)
        ref_map = sr.reference_maps()[k]
        _against_truth("Y frame %d" % k, y[k], sr.inside(m, rr.ROWS, rr.COLS), m, rr.sample(col["y"][k], ref_map)[0], ref_map, col["y"][k],
                       sr.truth()[k], rr.ROWS, rr.COLS, sr.device_tolerance(sr.LENS))
        m = p.yuv_map(yuv.NV16, 1, rr.COLS, rr.ROWS, lens, times[k], synth.D_TRUE, **kw)
        ref_map = yr.reference_maps(site)[k]
        ok = sr.inside(m, yr.C_ROWS, yr.C_COLS)
        for c, name in enumerate("uv"):
            _against_truth("%s frame %d" % (name.upper(), k), uv[k, ..., c], ok, m, sr.sample(col[name][k], ref_map, fill=128)[0], ref_map,
                           col[name][k], truth_uv[c][k], yr.C_ROWS, yr.C_COLS, yr.device_tolerance(sr.LENS))


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_chunks_pitched_views_device_tensors_and_mixed_kinds_do_not_change_the_result(scene, wide_planes):
    """budgets below a frame pair per slot: the three frames go as three chunks through both slots into a 131 x 198
    output; pitched numpy views, device tensors and mixed kinds for in and out give the same bytes; the padding of `out`
    is not written"""
    from rssync_amd import synth, yuv
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col = yr.scene()
    y, uv, u, v = col["y"], col["uv"], col["u"], col["v"]
    orows, ocols = OUT
    kw = dict(sigma=sr.SIGMA, out_size=(ocols, orows))
    (one_y, one_uv), one_n = p.stabilize_yuv(yuv.NV16, (y, uv), times, lens, synth.D_TRUE, **kw)
    assert one_y.shape == (rr.N_FRAMES, orows, ocols) and one_uv.shape == (rr.N_FRAMES, orows, ocols // 2, 2)
    tabs, px_in, px_out = (rr.ROWS + 1) * 36, rr.ROWS * rr.COLS * 2, orows * ocols * 2     # (one row table per frame)
    budget = 2 * 1.5 * (tabs + px_in + px_out)
    (got_y, got_uv), got_n = p.stabilize_yuv_budget(yuv.NV16, (y, uv), times, lens, synth.D_TRUE, budget, **kw)
    np.testing.assert_array_equal(got_y, one_y)
    np.testing.assert_array_equal(got_uv, one_uv)
    np.testing.assert_array_equal(got_n, one_n)
    (iy, iu, iv), i_n = p.stabilize_yuv_budget(yuv.I422, (y, u, v), times, lens, synth.D_TRUE, budget, **kw)
    np.testing.assert_array_equal(iy, one_y)
    np.testing.assert_array_equal(_uv(iu, iv), one_uv)
    np.testing.assert_array_equal(i_n, one_n)
    # 4:4:4 in a 16-bit container through the chunks
    y10, _, _, u10, v10 = wide_planes[10]
    want, want_n = p.stabilize_yuv(yuv.I410, (y10, u10, v10), times, lens, synth.D_TRUE, **kw)
    got, got_n = p.stabilize_yuv_budget(yuv.I410, (y10, u10, v10), times, lens, synth.D_TRUE, 2 * 1.5 * (tabs + 3 * px_in + 3 * px_out), **kw)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got_n, want_n)
    # pitched views in, pitched views out
    wide_y = np.zeros((rr.N_FRAMES, rr.ROWS + 2, rr.COLS + 45), np.uint8)
    wide_y[:, 1:1 + rr.ROWS, 7:7 + rr.COLS] = y
    wide_uv = np.zeros((rr.N_FRAMES, yr.C_ROWS, yr.C_COLS + 9, 2), np.uint8)
    wide_uv[:, :, 4:4 + yr.C_COLS] = uv
    dst_y = np.full((rr.N_FRAMES, orows + 3, ocols + 21), 201, np.uint8)
    dst_uv = np.full((rr.N_FRAMES, orows + 1, ocols // 2 + 5, 2), 202, np.uint8)
    views = (dst_y[:, 1:1 + orows, 5:5 + ocols], dst_uv[:, 1:, 2:2 + ocols // 2])
    res, n = p.stabilize_yuv(yuv.NV16, (wide_y[:, 1:1 + rr.ROWS, 7:7 + rr.COLS], wide_uv[:, :, 4:4 + yr.C_COLS]), times, lens, synth.D_TRUE,
                             out=views, **kw)
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
    (dy, duv), dn = p.stabilize_yuv(yuv.NV16, dev, times, lens, synth.D_TRUE, **kw)
    assert isinstance(dy, torch.Tensor) and isinstance(duv, torch.Tensor)
    np.testing.assert_array_equal(dy.cpu().numpy(), one_y)
    np.testing.assert_array_equal(duv.cpu().numpy(), one_uv)
    np.testing.assert_array_equal(dn, one_n)
    dwide = (torch.from_numpy(wide_y).to("cuda:0")[:, 1:1 + rr.ROWS, 7:7 + rr.COLS], torch.from_numpy(wide_uv).to("cuda:0")[:, :, 4:4 + yr.C_COLS])
    dout_y = torch.full((rr.N_FRAMES, orows, ocols + 19), 9, dtype=torch.uint8, device="cuda:0")
    dout_uv = torch.full((rr.N_FRAMES, orows, ocols // 2 + 3, 2), 8, dtype=torch.uint8, device="cuda:0")
    p.stabilize_yuv(yuv.NV16, dwide, times, lens, synth.D_TRUE, out=(dout_y[:, :, 3:3 + ocols], dout_uv[:, :, 1:1 + ocols // 2]), **kw)
    back_y, back_uv = dout_y.cpu().numpy(), dout_uv.cpu().numpy()
    np.testing.assert_array_equal(back_y[:, :, 3:3 + ocols], one_y)
    np.testing.assert_array_equal(back_uv[:, :, 1:1 + ocols // 2], one_uv)
    assert (back_y[:, :, :3] == 9).all() and (back_y[:, :, 3 + ocols:] == 9).all()
    assert (back_uv[:, :, :1] == 8).all() and (back_uv[:, :, 1 + ocols // 2:] == 8).all()
    # mixed kinds across chunks: device frames into host arrays, host frames into device tensors; the budget counts the
    # planes that then pass through a slot
    (hy, huv), hn = p.stabilize_yuv_budget(yuv.NV16, dev, times, lens, synth.D_TRUE, 2 * 1.5 * (tabs + px_out), **kw)
    np.testing.assert_array_equal(hy, one_y)
    np.testing.assert_array_equal(huv, one_uv)
    np.testing.assert_array_equal(hn, one_n)
    dout = (torch.zeros(one_y.shape, dtype=torch.uint8, device="cuda:0"), torch.zeros(one_uv.shape, dtype=torch.uint8, device="cuda:0"))
    _, mn = p.stabilize_yuv_budget(yuv.NV16, (y, uv), times, lens, synth.D_TRUE, 2 * 1.5 * (tabs + px_in), out=dout, **kw)
    np.testing.assert_array_equal(dout[0].cpu().numpy(), one_y)
    np.testing.assert_array_equal(dout[1].cpu().numpy(), one_uv)
    np.testing.assert_array_equal(mn, one_n)


# 10 --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene):
    import rssync_amd
    from rssync_amd import color, colorinfill, colorzoom, synth, yuv
    p, lens, times = scene["problem"], scene["lens"], scene["times"]
    col = yr.scene()
    y, uv, u, v = (np.ascontiguousarray(col[k]) for k in ("y", "uv", "u", "v"))
    W, H, NF = rr.COLS, rr.ROWS, rr.N_FRAMES
    (want_y, want_uv), want_n = p.stabilize_yuv(yuv.NV16, (y, uv), times, lens, synth.D_TRUE, sigma=sr.SIGMA)
    lib = yuv.library()
    lib.rssync_set_panic_mode(1)
    L, T = np.ascontiguousarray(lens, np.float64), np.ascontiguousarray(times, np.float64)
    out_y, out_uv, out_u, out_v = np.zeros_like(y), np.zeros_like(uv), np.zeros_like(u), np.zeros_like(v)
    y16, uv16, out_y16, out_uv16 = y.astype(np.uint16), uv.astype(np.uint16), np.zeros(y.shape, np.uint16), np.zeros(uv.shape, np.uint16)
    PD = C.POINTER(C.c_double)

    def image(arrays, w, h, fmt):
        img = yuv.ColorImage()
        b = 2 if fmt in yuv.SIBLING else 1
        rows = {yuv.NV16: (w, w), yuv.I422: (w, w // 2, w // 2), yuv.I444: (w, w, w)}[yuv.SIBLING.get(fmt, fmt)]
        for k, a in enumerate(arrays):
            img.plane[k] = a if isinstance(a, int) or a is None else a.ctypes.data
            img.pitch[k], img.stride[k] = b * rows[k], b * rows[k] * h
        return img

    def prm_with(site=0, fill_set=0, fills=(0, 0, 0, 0), **kw):
        q = yuv.ColorParams()
        q.stab = color.StabilizeParams(**dict(dict(sigma=sr.SIGMA), **kw))
        q.chroma_site, q.fill_set = site, fill_set
        for k in range(4):
            q.fill[k] = fills[k]
        return q

    def call(fmt=yuv.NV16, src=None, dst=None, w=W, h=H, ow=W, oh=H, n=NF, prm=None, edit=None, entry=None):
        src = image((y, uv), w, h, yuv.NV16) if src is None else src
        dst = image((out_y, out_uv), ow, oh, yuv.NV16) if dst is None else dst
        if edit:
            edit(src, dst)
        prm = prm_with() if prm is None else prm
        return (entry or lib.rssync_yuv_stabilize)(p._h, fmt, C.byref(src), n, w, h, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE, None,
                                                   C.byref(prm), C.byref(dst), ow, oh, None)

    def bad(match, **kw):
        assert call(**kw) != 0, match
        msg = lib.rssync_last_error().decode()
        assert match in msg, (match, msg)

    def set_(which, field, k, value):
        def edit(src, dst):
            getattr(src if which == "in" else dst, field)[k] = value
        return edit

    def p216():
        """a P216 call's format and images, fresh every time: an edit changes them"""
        return dict(fmt=yuv.P216, src=image((y16, uv16), W, H, yuv.P216), dst=image((out_y16, out_uv16), W, H, yuv.P216))

    # the new entry takes its seven numbers alone
    for fmt in (0, 1, 2, 3, 16, 17, 18, 19, 35, 47, 52, -1):
        bad("format", fmt=fmt)
    # ... and the old entries turn them away, as every other number they turn away today
    clib, zlib, ilib = color.library(), colorzoom.library(), colorinfill.library()
    zooms = np.ones(NF)
    borrowed = np.zeros((NF, 2), np.uint64)
    for fmt in list(range(32, 52)) + [4, 7, 15, 20]:
        for entry in (clib.rssync_color_stabilize, clib.rssync_color16_stabilize):
            assert call(fmt=fmt, entry=entry) != 0 and "format" in lib.rssync_last_error().decode(), fmt
        src, dst, q = image((y, uv), W, H, yuv.NV16), image((out_y, out_uv), W, H, yuv.NV16), prm_with()
        assert zlib.rssync_colorzoom_stabilize(p._h, fmt, C.byref(src), NF, W, H, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE, None,
                                               C.byref(q), C.byref(dst), W, H, None, zooms.ctypes.data_as(PD)) != 0, fmt
        assert "format" in lib.rssync_last_error().decode()
        assert ilib.rssync_colorinfill_stabilize(p._h, fmt, C.byref(src), NF, W, H, T.ctypes.data_as(PD), L.ctypes.data, synth.D_TRUE, None,
                                                 C.byref(q), C.byref(dst), W, H, None, 1, borrowed.ctypes.data_as(C.POINTER(C.c_uint64))) != 0, fmt
        assert "format" in lib.rssync_last_error().decode()
    bad("chroma_site", prm=prm_with(site=2))
    bad("chroma_site", fmt=yuv.I444, src=image((y, y, y), W, H, yuv.I444), dst=image((out_y, out_y, out_y), W, H, yuv.I444), prm=prm_with(site=-1))
    bad("is NULL", edit=set_("in", "plane", 1, None))
    bad("is NULL", edit=set_("out", "plane", 0, None))
    bad("is NULL", fmt=yuv.I422, src=image((y, u, None), W, H, yuv.I422), dst=image((out_y, out_u, out_v), W, H, yuv.I422))
    bad("pitch", edit=set_("in", "pitch", 0, W - 1))
    bad("pitch", edit=set_("in", "pitch", 1, W - 1))
    bad("pitch", edit=set_("out", "pitch", 1, W - 1))
    bad("pitch", fmt=yuv.I422, src=image((y, u, v), W, H, yuv.I422), dst=image((out_y, out_u, out_v), W, H, yuv.I422),
        edit=set_("out", "pitch", 2, W // 2 - 1))
    bad("pitch", edit=set_("in", "pitch", 1, 2 * W - 2), **p216())
    bad("stride", edit=set_("in", "stride", 1, W * H - 1))
    bad("even", w=W - 1)
    bad("even", ow=W - 1)
    assert call(h=H - 1, oh=H - 1) == 0, lib.rssync_last_error().decode()          # (odd heights are allowed)
    bad("too small", w=2)
    bad("too small", ow=2)
    bad("too small", h=1)
    bad("alignment", edit=set_("in", "pitch", 1, 2 * W + 1), **p216())
    bad("alignment", edit=set_("out", "plane", 0, out_y16.ctypes.data + 1), **p216())
    bad("alignment", edit=set_("in", "stride", 0, 2 * W * H + 1), **p216())
    bad("fill 1", prm=prm_with(fill_set=1, fills=(0, 256, 0, 0)))
    bad("fill 0", prm=prm_with(fill_set=1, fills=(-1, 0, 0, 0)))
    bad("fill 2", prm=prm_with(fill_set=1, fills=(0, 0, 65536, 0)), **p216())
    bad("fill", prm=prm_with(fill=256))
    assert call(prm=prm_with(fill_set=1, fills=(65535, 65535, 0, 0), fill=999), **p216()) == 0, lib.rssync_last_error().decode()
    bad("overlaps", dst=image((out_y, y.ctypes.data + 8), W, H, yuv.NV16))
    dev_uv = torch.zeros((NF, H, W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bad("mixed kinds", src=image((y, dev_uv.data_ptr()), W, H, yuv.NV16))
    # the map: a plane that does not exist, a format of another entry
    m = np.zeros((H, W, 2), np.float32)

    def cmap(fmt, plane, out=m.ctypes.data, prm=None):
        return lib.rssync_yuv_map(p._h, fmt, plane, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, None,
                                  C.byref(prm_with() if prm is None else prm), out)

    for fmt, plane in ((yuv.NV16, 2), (yuv.I422, -1), (yuv.I444, 2), (yuv.P210, 3)):
        assert cmap(fmt, plane) != 0
        assert "plane" in lib.rssync_last_error().decode()
    assert cmap(yuv.NV16, 1, out=None) != 0
    assert cmap(1, 0) != 0 and "format" in lib.rssync_last_error().decode()
    assert clib.rssync_color_map(p._h, yuv.NV16, 0, W, H, L.ctypes.data, W, H, float(times[0]), synth.D_TRUE, None, C.byref(prm_with()),
                                 m.ctypes.data) != 0 and "format" in lib.rssync_last_error().decode()
    assert cmap(yuv.NV16, 1, prm=prm_with(site=3)) != 0 and "chroma_site" in lib.rssync_last_error().decode()
    assert cmap(yuv.NV16, 1) == 0, lib.rssync_last_error().decode()
    with pytest.raises(rssync_amd.RsSyncError, match="even"):
        p.stabilize_yuv(yuv.NV16, (y, uv), times, lens, synth.D_TRUE, out_size=(W - 1, H))
    with pytest.raises(ValueError):
        p.stabilize_yuv(yuv.NV16, (y, u), times, lens, synth.D_TRUE)
    # ... and the calls that follow work
    out_y[:], out_uv[:] = 0, 0
    assert call() == 0, lib.rssync_last_error().decode()
    np.testing.assert_array_equal(out_y, want_y)
    np.testing.assert_array_equal(out_uv, want_uv)
    (again_y, again_uv), again_n = p.stabilize_yuv(yuv.NV16, (y, uv), times, lens, synth.D_TRUE, sigma=sr.SIGMA)
    np.testing.assert_array_equal(again_y, want_y)
    np.testing.assert_array_equal(again_uv, want_uv)
    np.testing.assert_array_equal(again_n, want_n)
