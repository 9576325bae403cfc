"""Every infill kernel on the device -- gray (include/rssync_infill.h, csrc/kernels/infill.hpp), the colour front's 28 donor_*
kernels (include/rssync_colorinfill.h, csrc/kernels/colorinfill.hpp) and the 28 lend* kernels of 4:2:2 / 4:4:4
(include/rssync_infillyuv.h, csrc/kernels/infillyuv.hpp) -- across the lenses and motions of tests/warp_cases.py: a lens with
thousands of samples without a ray ('half'), a 250 rad/s roll, a 20-fold motion that leaves half a frame for the fill, both
cameras, both samplers, other output sizes and an odd one (tests/infill_cases.py; the conditions these comparisons rest on are
proved in tests/test_infill_cases_cpu.py).  94 x 170 luma, three frames, radius 2: every frame's order skips steps.  What
tests/test_gpu_render_lenses.py and tests/test_gpu_yuv_lenses.py are to the renderers.

     what is compared                                                   kernels and paths reached
  a  the donor maps -- candidate g's time against frame f's target --   the map kernels with a target that is not the frame's own: plane 0, the
     of every (f, g) of the three orders against float64: plane 0, the   4:2:2 chroma camera (the luma's row tables, halved in x alone) and the
     4:2:2 and the 4:2:0 chroma plane with both sitings                  4:2:0 chroma camera (its own row tables at the chroma frame time)
  b  4:2:2 and 4:4:4: the bytes and all four counters of seven formats  all 28 lend* instantiations: lend422_8 <NV16 or not>, lend422_16 <I210,
     with both samplers, from numpy on the device's own maps             P210, P216>, lend444_8, lend444_16, x LENS / PINHOLE x FILTER 0 / 1
  c  gray and the colour front the same way: GRAY8, NV12, I420, RGBA32,  the gray infill kernel with both cameras and samplers and all 28 donor_*
     P010, P016, I010, GRAY16                                            instantiations
  d  the LENS camera at 110 x 62 and at the odd 109 x 61                 rays read as rays[v * out_cols + u] with the chroma plane's own extent
  e  one frame per chunk against the unchunked call that b and c anchor  f0, src0 and the halo arithmetic of donor_plane when frame 0 and frame 2
                                                                         borrow from the far end of the call
"""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color_reference as cr
import infill_cases as ic
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
import yuv_cases as yc

pytestmark = pytest.mark.gpu


def _problem(gyro):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def problems(built):
    """one problem per motion of the cases"""
    return {m: _problem(wc.gyro(m)) for m in sorted({c.motion for c in ic.CASES.values()})}


_TARGETS, _MAPS = {}, {}


def _targets(problems, name):
    """the device's path at the three frame times: the targets every call and every map of a case is given"""
    from rssync_amd import synth
    c = ic.case(name)
    key = (c.lens, c.motion)
    if key not in _TARGETS:
        _TARGETS[key] = problems[c.motion].stabilize_path(wc.frame_times(), ic.lens(c)[0], synth.D_TRUE, rc.SIGMA)
        _TARGETS[key].setflags(write=False)
    return _TARGETS[key]


def _map(problems, name, kind, site, f, g, api=None):
    """the device's map of candidate g's time against frame f's target in a plane's camera; api: the call that is asked
    (None: stabilize_map for plane 0, NV16's plane 1, NV12's plane 1)"""
    from rssync_amd import synth
    c = ic.case(name)
    p, L, times, targets = problems[c.motion], ic.lens(c), wc.frame_times(), _targets(problems, name)
    args = (rc.COLS, rc.ROWS, L, times[g], synth.D_TRUE)
    kw = dict(target=targets[f], zoom=c.zoom, camera=c.camera, out_size=c.out_size)
    if kind == ic.LUMA and api is None:
        return p.stabilize_map(*args, **kw)
    if kind == ic.LUMA:
        family, fmt = ic.FORMATS[api]
        return (p.yuv_map if family == ic.YUV else p.color_map)(fmt, 0, *args, chroma_site=site, **kw)
    if kind == ic.C422:
        return p.yuv_map(yc.NV16, 1, *args, chroma_site=site, **kw)
    return p.color_map(rc.NV12, 1, *args, chroma_site=site, **kw)


def _maps(problems, name, kind, site):
    """(f, g) -> the device's map, of every pair of the three orders; cached per case, plane and siting (section a of
    tests/test_gpu_yuv_lenses.py and section b of tests/test_gpu_render_lenses.py hold every other format's map to these)"""
    key = (name, kind, site if kind != ic.LUMA else cr.CENTER)
    if key not in _MAPS:
        _MAPS[key] = {(f, g): _map(problems, name, kind, site, f, g) for f, g in ic.pairs()}
        for m in _MAPS[key].values():
            m.setflags(write=False)
    return _MAPS[key]


# a -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ic.CASES))
def test_a_donor_maps_against_the_float64_reference(problems, name):
    """rc.check_map's three assertions for every (f, g) with the float64 map at the same target; the tolerance is
    wc.tolerance's for that very map, and at least a quarter of its samples are compared.  Plane 0 is asked of
    stabilize_map; yuv_map and color_map give its bits."""
    c, targets = ic.case(name), _targets(problems, name)
    worst, worst_tol, smallest_share = 0.0, 0.0, 1.0
    for kind in ic.kinds(name):
        for site in ((cr.CENTER,) if kind == ic.LUMA else rc.SITES):
            cs = c._replace(site422=site, site420=site)
            maps = _maps(problems, name, kind, site)
            for f, g in ic.pairs():
                m = ic.map_case(cs, kind, f, g, targets)
                share = m["compared"].sum() / m["compared"].size
                assert share >= ic.MIN_COMPARED_SHARE, (kind, site, f, g)
                d = rc.check_map("a %s %s site %d f %d g %d" % (name, kind, site, f, g), maps[(f, g)], m, *ic.source_size(kind))
                if d > worst:
                    worst, worst_tol = d, m["tol"]
                smallest_share = min(smallest_share, share)
                if kind == ic.LUMA:
                    for api in (("i444", "rgba32") if name in ic.ODD_CASES else ("nv16", "i444", "nv12", "rgba32")):
                        np.testing.assert_array_equal(rc.u32(_map(problems, name, kind, site, f, g, api)), rc.u32(maps[(f, g)]), err_msg=api)
    print("section a %s: largest distance %.3g px (its tolerance %.3g), smallest compared share %.2f" % (name, worst, worst_tol, smallest_share))


# b, c, d -----------------------------------------------------------------------------------------------------------------
def _call(p, fmt_name, src, c, targets, filter, out=None, budget=None):
    """the infill call of a format's family -> (planes, n_outside (n, 1 or 2), n_borrowed)"""
    from rssync_amd import synth
    family, fmt = ic.FORMATS[fmt_name]
    L, times, fills = ic.lens(c), wc.frame_times(), ic.fills(fmt_name)
    kw = dict(targets=targets, zoom=c.zoom, camera=c.camera, filter=filter, out_size=c.out_size, sigma=rc.SIGMA)
    if family == ic.GRAY:
        res, n, nb = p.stabilize_frames_infilled(src[0], times, L, synth.D_TRUE, ic.RADIUS, fill=fills[0], out=None if out is None else out[0], **kw)
        return (res,), n[:, None], nb[:, None]
    site = ic.site_of(c, ic.kind_of(fmt_name, len(src) - 1))
    frames = src if len(src) > 1 else src[0]
    if budget is not None:
        fn = p.stabilize_yuv_infilled_budget if family == ic.YUV else p.stabilize_color_infilled_budget
        res, n, nb = fn(fmt, frames, times, L, synth.D_TRUE, ic.RADIUS, budget, chroma_site=site, fills=tuple(fills) + (0,) * (4 - len(fills)), **kw)
    else:
        fn = p.stabilize_yuv_infilled if family == ic.YUV else p.stabilize_color_infilled
        res, n, nb = fn(fmt, frames, times, L, synth.D_TRUE, ic.RADIUS, chroma_site=site, fills=fills,
                        out=None if out is None else (out if len(out) > 1 else out[0]), **kw)
    return rc.as_tuple(res), n, nb


def _out_shape(c, fmt_name, k, a):
    rows, cols = ic.out_shape(c, ic.kind_of(fmt_name, k))
    return (a.shape[0], rows, cols) + a.shape[3:]


def _check_infill(problems, name, fmt_name):
    """Both filters.  Per plane k and frame f the picture is rc.compose_plane over the device's maps of f's candidates through
    the format's numpy sampler (the third plane of a planar format on plane 1's map, a 4:4:4 plane 1 and RGBA on plane 0's);
    n_outside[f, pl] is the number of samples with place < 0, n_borrowed[f, pl] with place > 0 (4:4:4: both entries equal;
    single-plane colour formats: the chroma entries 0); the padding of the pitched outputs stays; with 'half' every sample
    without a ray holds its plane's stored fill and is among the filled; every plane borrows from both later places and
    leaves samples filled, by the composed places."""
    c, targets = ic.case(name), _targets(problems, name)
    family, fmt = ic.FORMATS[fmt_name]
    p, src = problems[c.motion], ic.frames(fmt_name)
    kind = [ic.kind_of(fmt_name, k) for k in range(len(src))]
    maps = [_maps(problems, name, kd, ic.site_of(c, kd)) for kd in kind]
    shift = ic.shift(fmt_name)
    for filter in (0, 1):
        pad_value = 0xABCD if src[0].dtype == np.uint16 else 0xAB
        whole, views = zip(*[rc.padded(_out_shape(c, fmt_name, k, a), a.dtype, pad_value) for k, a in enumerate(src)])
        res, n_out, n_lent = _call(p, fmt_name, src, c, targets, filter, out=views)
        print("%s %s filter %d: filled %s borrowed %s" % (name, fmt_name, filter, n_out.T.tolist(), n_lent.T.tolist()))
        want_out, want_lent = np.zeros(n_out.shape, np.uint64), np.zeros(n_out.shape, np.uint64)
        for k, (w, v) in enumerate(zip(whole, views)):
            outr = ic.masks(c, kind[k])[1]
            second = third = filled = 0
            for f in range(ic.N_FRAMES):
                pic, place = ic.compose(fmt_name, k, src, maps[k], f, filter)
                np.testing.assert_array_equal(v[f], pic, err_msg="%s %s plane %d frame %d filter %d" % (name, fmt_name, k, f, filter))
                second, third, filled = second + int((place == 1).sum()), third + int((place == 2).sum()), filled + int((place < 0).sum())
                if k < n_out.shape[1]:
                    want_out[f, k], want_lent[f, k] = (place < 0).sum(), (place > 0).sum()
                if c.lens == "half":
                    assert outr.sum() >= ic.MIN_NAN and (place[outr] < 0).all(), (k, f)
                    assert (v[f][outr] == ic.stored_fill(fmt_name, k)).all(), (k, f)
                    assert all(np.isnan(maps[k][(f, g)][outr]).all() for g in range(ic.N_FRAMES)), (k, f)
            assert second > 0 and third > 0 and filled > 0, (name, fmt_name, k, second, third, filled)
            if shift:
                assert (v & ((1 << shift) - 1)).max() == 0, (fmt_name, k)   # P010's and P210's words keep their low six bits zero
            pad = np.ones(w.shape, bool)
            pad[:, 1:1 + v.shape[1], 4:4 + v.shape[2]] = False
            assert (w[pad] == pad_value).all(), (fmt_name, k)
        np.testing.assert_array_equal(n_out, want_out, err_msg="%s %s filter %d: filled" % (name, fmt_name, filter))
        np.testing.assert_array_equal(n_lent, want_lent, err_msg="%s %s filter %d: borrowed" % (name, fmt_name, filter))
        if family == ic.YUV and fmt in yc.F444:
            np.testing.assert_array_equal(n_out[:, 1], n_out[:, 0])
            np.testing.assert_array_equal(n_lent[:, 1], n_lent[:, 0])
        if c.lens == "half":
            for pl in range(min(n_out.shape[1], len(src))):
                assert (n_out[:, pl] >= ic.masks(c, kind[pl])[1].sum()).all(), pl


@pytest.mark.parametrize("name", ic.INPUT_SIZE_CASES)
@pytest.mark.parametrize("fmt_name", ic.YUV_FORMATS)
def test_b_yuv_infill_bytes_and_counters_from_the_devices_own_maps(problems, fmt_name, name):
    _check_infill(problems, name, fmt_name)


@pytest.mark.parametrize("name", ic.INPUT_SIZE_CASES)
@pytest.mark.parametrize("fmt_name", ic.COLOR_FORMATS)
def test_c_gray_and_colour_infill_bytes_and_counters_from_the_devices_own_maps(problems, fmt_name, name):
    _check_infill(problems, name, fmt_name)


@pytest.mark.parametrize("name", ic.RESIZED_CASES)
@pytest.mark.parametrize("fmt_name", ["nv16", "i210", "i444", "nv12", "p010", "gray8"])
def test_d_another_output_size_with_the_lens_camera(problems, fmt_name, name):
    assert ic.case(name).camera == sr.LENS and ic.case(name).out_size == ic.OUT
    _check_infill(problems, name, fmt_name)


@pytest.mark.parametrize("name", ic.ODD_CASES)
@pytest.mark.parametrize("fmt_name", ["i444", "i410", "rgba32", "gray8"])
def test_d_an_odd_output_width_with_the_lens_camera(problems, fmt_name, name):
    assert ic.case(name).camera == sr.LENS and ic.case(name).out_size[0] % 2 == 1
    _check_infill(problems, name, fmt_name)


# e -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.CHUNK_CASES)
@pytest.mark.parametrize("fmt_name", ["i210", "i410", "i420", "rgba32"])
def test_e_one_frame_per_chunk_is_the_unchunked_call(problems, fmt_name, name):
    """a budget that pays for one frame per chunk: frame 2 borrows from frame 0, two chunks away, and with 'half' frame 0
    from frame 2 (ic.COUNTS' third places); byte for byte and counter for counter the unchunked call, which sections b and c
    anchor"""
    c, targets = ic.case(name), _targets(problems, name)
    p, src = problems[c.motion], ic.frames(fmt_name)
    for filter in (0, 1):
        want, n_out, n_lent = _call(p, fmt_name, src, c, targets, filter)
        got, g_out, g_lent = _call(p, fmt_name, src, c, targets, filter, budget=1000)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(a, b, err_msg="%s %s plane %d filter %d" % (name, fmt_name, k, filter))
        np.testing.assert_array_equal(g_out, n_out)
        np.testing.assert_array_equal(g_lent, n_lent)
        assert n_lent[2].sum() > 0 and n_out.sum() > 0
