"""Every renderer built on the stabiliser, on the device, across the lenses and motions of tests/warp_cases.py: off-centre,
anisotropic and strongly distorted lenses, lenses that cannot image every pixel (NaN rays), the scene's motion, its 20-fold and
a 250 rad/s roll (tests/render_cases.py; the conditions these comparisons rest on are proved in
tests/test_render_cases_cpu.py).  94 x 170 luma, 47 x 85 chroma: more than one tile and part tiles in both planes.

     what is compared                                                   kernels and paths reached
  a  the gray stabiliser's map with the PINHOLE camera against float64, the host's output camera scaled to another size (stabilize_host.hpp),
     at the input's size and at another                                 stab_pinhole_ray in the map kernel
  b  color_map of plane 0 and plane 1 against float64 (NV12; a 16-bit   the host's chroma camera of both sitings (color_host.hpp, color_math.hpp), the
     format's map IS its sibling's: c holds P010 to it), both sitings,   ray maps of both cache places (LENS), the constant-camera position ColorPos
     both cameras, two output sizes
  c  the bytes and both counters of every body with both samplers, from  the constant-camera bodies yuv8 (NV12, I420), rgba8, yuv16 (P010, P016, I010) and
     the numpy samplers on the device's own map; NaN rays in both planes gray16, FILTER 0 and 1, under ColorPos<LENS> and ColorPos<PINHOLE>
  d  a zoom per frame against the constant-camera call at that zoom,     zoom_render_kernel, the percam_* kernels (PercamPos, rays computed in place in
     bytes and counts, seven formats, both samplers, both cameras        fp64), the LDS-staged I420 / I010 kernels with the LENS camera
  e  fitted zooms, strengths and statuses against the float64 bisection, zoom_fit_kernel (also through fit_zoom_color's chroma camera) and
     exactly                                                             limit_fit_kernel, LENS and PINHOLE, NaN rays at the border
  f  the infill under large fills: bytes and counts from the numpy       the donor kernels, gray and colour (NV12, P010), with donor maps
     samplers on the device's own maps of every candidate                against another frame's target
  g  one problem through ten calls that must refresh one, both or none   both places of the ray-map cache (rect_rays_into: the luma place shared with
     of the two cached ray maps, against fresh problems                  the rectifier, the chroma place), the row tables
"""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color_reference as cr
import infill_reference as ir
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc

pytestmark = pytest.mark.gpu

GRAY8, NV12, I420, RGBA32 = rc.GRAY8, rc.NV12, rc.I420, rc.RGBA32
GRAY16, P010, P016, I010 = rc.GRAY16, rc.P010, rc.P016, rc.I010
FORMATS = (GRAY8, NV12, I420, RGBA32, P010, I010, GRAY16)            # section d
BODIES = {"yuv8-nv12": NV12, "yuv8-i420": I420, "rgba8": RGBA32, "yuv16-p010": P010, "yuv16-p016": P016, "yuv16-i010": I010,
          "gray16": GRAY16}                                           # section c
SIBLING, FILLS8, FILLS16 = rc.COLOR_SIBLING, rc.FILLS8, rc.FILLS16


def _problem(gyro):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def problems(built):
    """one problem per motion"""
    return {m: _problem(wc.gyro(m)) for m in rc.MOTIONS}


# the three assertions of a map, the padded output and the bit view: shared with tests/test_gpu_yuv_lenses.py
_u32, _check_map, _padded = rc.u32, rc.check_map, rc.padded


# the formats' noise planes, fills and numpy samplers: shared with tests/test_gpu_infill_lenses.py
_input, _fills, _as_tuple, _sample_plane, _plane_fill = rc.color_frames, rc.color_fills, rc.as_tuple, rc.color_sample_plane, rc.color_plane_fill


# a -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,motion", wc.pinhole_cases())
def test_a_stabiliser_map_with_the_pinhole_camera_against_the_float64_reference(problems, name, motion):
    worst = 0.0
    for out_size in (None, wc.PINHOLE_OUT):
        c = wc.stab_case(name, motion, sr.PINHOLE, out_size)
        got = problems[motion].stabilize_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"], sigma=wc.STAB_SIGMA, zoom=wc.STAB_ZOOM,
                                             camera=sr.PINHOLE, out_size=out_size)
        worst = max(worst, _check_map("a pinhole %s %s out %s" % (name, motion, out_size), got, c, wc.ROWS, wc.COLS))
    print("section a largest distance %.3g px" % worst)


# b -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,motion", [(n, m) for n in rc.MAP_LENSES for m in rc.MOTIONS])
def test_b_plane_maps_of_the_colour_front_against_the_float64_reference(problems, name, motion):
    p, L, worst = problems[motion], rc.lens(name), 0.0
    for camera in rc.CAMERAS:
        for out_size in rc.out_sizes():
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, camera=camera, out_size=out_size)
            c = rc.plane_case(name, motion, 0, cr.CENTER, camera, rc.ZOOM, out_size)
            m0 = p.color_map(NV12, 0, rc.COLS, rc.ROWS, L, c["time"], c["delay"], **kw)
            worst = max(worst, _check_map("b %s %s camera %d out %s plane 0" % (name, motion, camera, out_size), m0, c, rc.ROWS, rc.COLS))
            for fmt in (I420, RGBA32, GRAY8):
                for site in rc.SITES:       # (plane 0 does not know the siting)
                    np.testing.assert_array_equal(_u32(p.color_map(fmt, 0, rc.COLS, rc.ROWS, L, c["time"], c["delay"], chroma_site=site, **kw)), _u32(m0))
            for site in rc.SITES:
                c = rc.plane_case(name, motion, 1, site, camera, rc.ZOOM, out_size)
                m1 = p.color_map(NV12, 1, rc.COLS, rc.ROWS, L, c["time"], c["delay"], chroma_site=site, **kw)
                worst = max(worst, _check_map("b %s %s camera %d out %s plane 1 site %d" % (name, motion, camera, out_size, site), m1, c, rc.C_ROWS,
                                              rc.C_COLS))
                np.testing.assert_array_equal(_u32(p.color_map(I420, 1, rc.COLS, rc.ROWS, L, c["time"], c["delay"], chroma_site=site, **kw)), _u32(m1))
    print("section b largest distance %.3g px" % worst)


# c -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(rc.BODY_CASES)), ids=["%s-%s" % c[:2] for c in rc.BODY_CASES])
@pytest.mark.parametrize("body", list(BODIES))
def test_c_bodies_bytes_and_counts_from_the_devices_own_map(problems, body, case):
    """three frames per call, distinct fills per plane, noise over the format's whole range, pitched output whose padding
    stays; per plane every byte is the numpy sampler's on the device's map, every outside sample the plane's fill, and both
    counters the map's outside counts"""
    from rssync_amd import synth
    name, motion, zoom, camera = rc.BODY_CASES[case]
    fmt, site = BODIES[body], (cr.LEFT, cr.CENTER)[case % 2]
    p, L, times = problems[motion], rc.lens(name), wc.frame_times()
    src, fills = _as_tuple(_input(fmt)), _fills(fmt)
    yuv = SIBLING.get(fmt, fmt) in (NV12, I420)
    kw = dict(sigma=rc.SIGMA, zoom=zoom, camera=camera, chroma_site=site)
    maps = [[p.color_map(SIBLING.get(fmt, fmt), pl, rc.COLS, rc.ROWS, L, t, synth.D_TRUE, **kw) for pl in ((0, 1) if yuv else (0,))] for t in times]
    sizes = [(rc.ROWS, rc.COLS), (rc.C_ROWS, rc.C_COLS)]
    outside = np.array([[int((~sr.inside(m, *sizes[pl])).sum()) for pl, m in enumerate(mk)] + [0] * (2 - len(mk)) for mk in maps], np.uint64)
    if camera == sr.LENS:
        for pl in range(2 if yuv else 1):
            outr = rc.plane_masks(L, pl, site, zoom, camera, None)[1]
            assert np.isnan(maps[1][pl][outr]).all()
            assert (outside[:, pl] >= outr.sum()).all()
            if zoom == 1.0:
                assert outr.sum() >= 9        # NaN rays in this plane
    for filter in (0, 1):
        pad_value = 0xABCD if fmt in SIBLING else 0xAB
        whole, views = zip(*[_padded(a.shape, a.dtype, pad_value) for a in src])
        res, n_out = p.stabilize_color(fmt, src if len(src) > 1 else src[0], times, L, synth.D_TRUE, fills=fills, filter=filter,
                                       out=views if len(views) > 1 else views[0], **kw)
        print("c %s %s %s zoom %.1f camera %d filter %d: outside %s" % (body, name, motion, zoom, camera, filter, n_out.tolist()))
        np.testing.assert_array_equal(n_out, outside)
        assert (n_out[:, 0] > 0).all() and (n_out[:, 0] < rc.ROWS * rc.COLS).all()
        if yuv:
            assert (n_out[:, 1] > 0).all() and (n_out[:, 1] < rc.C_ROWS * rc.C_COLS).all()
        if (name, motion) in rc.ROLL_COUNTS_DIFFER:
            assert len(set(n_out[:, 0].tolist())) == 3
        for k, (w, v) in enumerate(zip(whole, views)):
            pl = min(k, 1)
            for f in range(rc.N_FRAMES):
                m = maps[f][pl]
                want, n = _sample_plane(fmt, k, src[k][f], m, _plane_fill(fmt, k, fills), filter)
                np.testing.assert_array_equal(v[f], want, err_msg="%s plane %d frame %d filter %d" % (body, k, f, filter))
                assert n == int(outside[f, pl])
                miss = ~sr.inside(m, *sizes[pl])
                stored = np.asarray(_plane_fill(fmt, k, fills)) << (6 if fmt == P010 else 0)
                assert miss.any() and (v[f][miss] == stored).all(), (body, k, f)
            pad = np.ones(w.shape, bool)
            pad[:, 1:1 + v.shape[1], 4:4 + v.shape[2]] = False
            assert (w[pad] == pad_value).all(), (body, k)


# d -----------------------------------------------------------------------------------------------------------------------
def _constant(p, fmt, frames, times, L, zoom, **kw):
    from rssync_amd import synth
    if fmt == GRAY8:
        kw = {k: v for k, v in kw.items() if k not in ("chroma_site", "fills")}
        out, n = p.stabilize_frames(frames, times, L, synth.D_TRUE, zoom=zoom, fill=FILLS8[0], **kw)
        return (out,), n
    out, n = p.stabilize_color(fmt, frames, times, L, synth.D_TRUE, zoom=zoom, **kw)
    return _as_tuple(out), n


def _zoomed(p, fmt, frames, times, L, zooms, **kw):
    from rssync_amd import synth
    if fmt == GRAY8:
        kw = {k: v for k, v in kw.items() if k not in ("chroma_site", "fills")}
        out, n = p.stabilize_frames_zoomed(frames, times, L, synth.D_TRUE, zooms, fill=FILLS8[0], **kw)
        return (out,), n
    out, n = p.stabilize_color_zoomed(fmt, frames, times, L, synth.D_TRUE, zooms, **kw)
    return _as_tuple(out), n


@pytest.mark.parametrize("camera", rc.CAMERAS, ids=["lens", "pinhole"])
@pytest.mark.parametrize("name,motion,zoom", rc.PERCAM_CASES)
def test_d_a_zoom_per_frame_is_the_constant_camera_at_that_zoom(problems, name, motion, zoom, camera):
    """three equal zooms: the bytes and counts of the constant-camera call; three different zooms: every frame is the
    single-frame constant-camera call at its zoom.  With the LENS camera 'half' and 'nonmono' have NaN rays in both planes:
    computed in place here, read from the cached ray map there."""
    p, L, times = problems[motion], rc.lens(name), wc.frame_times()
    site = cr.LEFT if name in ("half", "strong") else cr.CENTER
    filled = 0
    for fmt in FORMATS:
        frames = _input(fmt)
        for filter in (0, 1):
            kw = dict(sigma=rc.SIGMA, camera=camera, filter=filter, chroma_site=site, fills=_fills(fmt))
            got, n = _zoomed(p, fmt, frames, times, L, [zoom] * rc.N_FRAMES, **kw)
            want, want_n = _constant(p, fmt, frames, times, L, zoom, **kw)
            what = "%s %s camera %d format %d filter %d" % (name, motion, camera, fmt, filter)
            for k, (a, b) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(a, b, err_msg="%s equal zooms plane %d" % (what, k))
            np.testing.assert_array_equal(n, want_n, err_msg=what)
            filled += int(np.asarray(n).sum())
            got, n = _zoomed(p, fmt, frames, times, L, rc.PERCAM_ZOOMS, **kw)
            for f, z in enumerate(rc.PERCAM_ZOOMS):
                one = _input(fmt, slice(f, f + 1))
                want, want_n = _constant(p, fmt, one, times[f:f + 1], L, z, **kw)
                for k, (a, b) in enumerate(zip(got, want)):
                    np.testing.assert_array_equal(a[f], b[0], err_msg="%s frame %d at zoom %.1f plane %d" % (what, f, z, k))
                np.testing.assert_array_equal(np.asarray(n)[f], np.asarray(want_n)[0], err_msg="%s frame %d" % (what, f))
                if fmt == NV12 and filter == 0 and f == 0 and camera == sr.LENS and z == 1.0:
                    for pl in (0, 1):
                        outr = rc.plane_masks(L, pl, site, z, camera, None)[1]
                        assert int(np.asarray(want_n)[0, pl]) >= outr.sum()
                        assert outr.sum() >= 9 or name not in ("half", "nonmono")
    print("d %s %s camera %d: %d samples filled in all" % (name, motion, camera, filled))
    assert filled > 0 or camera == sr.PINHOLE


# e -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rc.FIT_CASES))
def test_e_fitted_zooms_are_the_float64_bisections(problems, case):
    """fit_zoom on plane 0, and fit_zoom_color of NV12: include/rssync_colorzoom.h -- the larger of plane 0's zoom and the
    chroma plane's (a camera of its own at half the size, against the path at the luma's frame times), the statuses OR-ed"""
    from rssync_amd import synth
    name, motion, camera, steps, k_l, st_l, k_c, st_c = rc.FIT_CASES[case]
    p, L = problems[motion], rc.lens(name)
    kw = dict(steps=steps, sigma=rc.SIGMA, camera=camera)
    z, st = p.fit_zoom(rc.COLS, rc.ROWS, L, wc.frame_times(), synth.D_TRUE, rc.FIT_LO, rc.FIT_HI, **kw)
    print("e %s: luma %s %s" % (case, z.tolist(), st.tolist()))
    np.testing.assert_array_equal(z, rc.fit_zooms(k_l, steps))
    np.testing.assert_array_equal(st, np.array(st_l, np.uint32))
    for fmt in (GRAY16, RGBA32):
        zg, sg = p.fit_zoom_color(fmt, rc.COLS, rc.ROWS, L, wc.frame_times(), synth.D_TRUE, rc.FIT_LO, rc.FIT_HI, **kw)
        np.testing.assert_array_equal(zg, z)
        np.testing.assert_array_equal(sg, st)
    zc, sc = p.fit_zoom_color(NV12, rc.COLS, rc.ROWS, L, wc.frame_times(), synth.D_TRUE, rc.FIT_LO, rc.FIT_HI, chroma_site=cr.CENTER, **kw)
    print("e %s: NV12 %s %s" % (case, zc.tolist(), sc.tolist()))
    np.testing.assert_array_equal(zc, np.maximum(rc.fit_zooms(k_l, steps), rc.fit_zooms(k_c, steps)))
    np.testing.assert_array_equal(sc, np.array(st_l, np.uint32) | np.array(st_c, np.uint32))
    if 0 < sum(st_l) < rc.N_FRAMES:         # clear and not-clear frames in one call, each in its place
        assert st.tolist() == list(st_l) and set(st.tolist()) == {rc.CLEAR, rc.NOT_CLEAR}
        assert (z[np.array(st_l) == rc.NOT_CLEAR] == rc.FIT_HI).all()


@pytest.mark.parametrize("case", list(rc.STRENGTH_CASES))
def test_e_fitted_strengths_are_the_float64_bisections(problems, case):
    from rssync_amd import synth
    name, motion, camera, zoom, k, want_st = rc.STRENGTH_CASES[case]
    a, st = problems[motion].fit_strength(rc.COLS, rc.ROWS, rc.lens(name), wc.frame_times(), synth.D_TRUE, zoom=zoom, steps=rc.FIT_STEPS,
                                          sigma=rc.SIGMA, camera=camera)
    print("e %s: strengths %s %s" % (case, (a * 1024).tolist(), st.tolist()))
    np.testing.assert_array_equal(a, rc.fit_strengths(k))
    np.testing.assert_array_equal(st, np.array(want_st, np.uint32))
    if 0 < sum(want_st) < rc.N_FRAMES:
        assert set(st.tolist()) == {rc.CLEAR, rc.NOT_CLEAR} and (a[np.array(want_st) == rc.NOT_CLEAR] == 0).all()


# f -----------------------------------------------------------------------------------------------------------------------
def _infill_want(fmt, k, planes, get_map, fills, f):
    """plane k of frame f composed from the device's maps of its candidates -> (picture, filled, borrowed)"""
    cand = ir.candidates(f, rc.N_FRAMES, rc.INFILL_RADIUS)
    pl = min(k, 1)
    rows, cols = ((rc.ROWS, rc.COLS), (rc.C_ROWS, rc.C_COLS))[pl]
    fill = _plane_fill(fmt, k, fills)
    stored = np.asarray(fill) << (6 if fmt == P010 else 0)
    out, place = rc.compose_plane([planes[k][g] for g in cand], [get_map(pl, g, f) for g in cand], rows, cols, stored,
                                  lambda fr, m: _sample_plane(fmt, k, fr, m, fill, 0)[0])
    return out, int((place < 0).sum()), int((place > 0).sum())


@pytest.mark.parametrize("name,motion", rc.INFILL_CASES)
def test_f_infill_under_large_fills_from_the_devices_own_maps(problems, name, motion):
    from rssync_amd import synth
    p, L, times = problems[motion], rc.lens(name), wc.frame_times()
    targets = p.stabilize_path(times, L[0], synth.D_TRUE, rc.SIGMA)
    kw = dict(zoom=rc.ZOOM, camera=sr.LENS)
    # gray
    y = rc.noise8()["y"]
    out, n_out, n_lent = p.stabilize_frames_infilled(y, times, L, synth.D_TRUE, rc.INFILL_RADIUS, targets=targets, fill=FILLS8[0], **kw)
    want = [_infill_want(GRAY8, 0, (y,), lambda pl, g, f: p.stabilize_map(rc.COLS, rc.ROWS, L, times[g], synth.D_TRUE, target=targets[f], **kw),
                         FILLS8[:1], f) for f in range(rc.N_FRAMES)]
    print("f %s %s gray: filled %s borrowed %s" % (name, motion, n_out.tolist(), n_lent.tolist()))
    for f in range(rc.N_FRAMES):
        np.testing.assert_array_equal(out[f], want[f][0], err_msg="gray frame %d" % f)
    assert n_out.tolist() == [w[1] for w in want] and n_lent.tolist() == [w[2] for w in want]
    assert n_out.sum() > 0 and n_lent.sum() > 0
    # colour
    for fmt, site in ((NV12, cr.LEFT), (P010, cr.CENTER)):
        src, fills = _input(fmt), _fills(fmt)
        ckw = dict(chroma_site=site, **kw)
        res, n_out, n_lent = p.stabilize_color_infilled(fmt, src, times, L, synth.D_TRUE, rc.INFILL_RADIUS, targets=targets, fills=fills, **ckw)
        print("f %s %s format %d: filled %s borrowed %s" % (name, motion, fmt, n_out.tolist(), n_lent.tolist()))
        cache = {}

        def get_map(pl, g, f):
            if (pl, g, f) not in cache:
                cache[(pl, g, f)] = p.color_map(SIBLING.get(fmt, fmt), pl, rc.COLS, rc.ROWS, L, times[g], synth.D_TRUE, target=targets[f], **ckw)
            return cache[(pl, g, f)]

        for k in (0, 1):
            for f in range(rc.N_FRAMES):
                pic, filled, lent = _infill_want(fmt, k, src, get_map, fills, f)
                np.testing.assert_array_equal(res[k][f], pic, err_msg="format %d plane %d frame %d" % (fmt, k, f))
                assert (int(n_out[f, k]), int(n_lent[f, k])) == (filled, lent), (fmt, k, f)
            assert n_out[:, k].sum() > 0 and n_lent[:, k].sum() > 0, (fmt, k)


# g -----------------------------------------------------------------------------------------------------------------------
def test_g_both_places_of_the_ray_cache_through_a_sequence_of_calls(built):
    """after every step the long-lived problem gives the bits of a freshly constructed one: map of plane 0, map of plane 1,
    frames, counts (at most two contexts alive); a step that returns to an earlier configuration gives that step's bits"""
    from rssync_amd import synth
    A, B = rc.cache_lenses()
    r, c, t, d = rc.CACHE_ROWS, rc.CACHE_COLS, wc.frame_time(), synth.D_TRUE
    rng = np.random.default_rng([7, r, c])
    y = rng.integers(0, 256, (1, r, c), dtype=np.uint8)
    uv = rng.integers(0, 256, (1, r // 2, c // 2, 2), dtype=np.uint8)
    rgba = rng.integers(0, 256, (1, r, c, 4), dtype=np.uint8)
    g1, g20 = wc.gyro("x1"), wc.gyro("x20")

    def nv12(L, site, out_size=None):
        def run(p):
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, chroma_site=site, out_size=out_size)
            m0, m1 = (p.color_map(NV12, pl, c, r, L, t, d, **kw) for pl in (0, 1))
            (oy, ouv), n = p.stabilize_color(NV12, (y, uv), [t], L, d, fills=(1, 2, 3), **kw)
            return m0, m1, oy, ouv, n
        return run

    def rgba32(L):
        def run(p):
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
            out, n = p.stabilize_color(RGBA32, rgba, [t], L, d, fills=FILLS8, **kw)
            return p.color_map(RGBA32, 0, c, r, L, t, d, **kw), out, n
        return run

    def gray_rect(L):
        def run(p):
            out, n = p.rectify_frames(y, [t], L, d, fill=wc.FILL)
            return p.rectify_map(c, r, L, t, d), out, n
        return run

    def zoomed(L):
        def run(p):
            (oy, ouv), n = p.stabilize_color_zoomed(NV12, (y, uv), [t], L, d, [1.2], sigma=rc.SIGMA, camera=sr.LENS, fills=(1, 2, 3))
            return oy, ouv, n
        return run

    p = _problem(g1)
    seen = {}

    def step(k, run, gyro=g1):
        got = run(p)
        fresh = _problem(gyro)
        want = run(fresh)
        fresh.close()
        for i, (a, b) in enumerate(zip(got, want)):
            a, b = (_u32(x) if x.dtype == np.float32 else x for x in (a, b))
            np.testing.assert_array_equal(a, b, err_msg="step %d: result %d" % (k, i))
        seen[k] = got
        return got

    def same(k, j):
        for a, b in zip(seen[k], seen[j]):
            a, b = (_u32(x) if x.dtype == np.float32 else x for x in (a, b))
            np.testing.assert_array_equal(a, b, err_msg="step %d is not step %d" % (k, j))

    def against_reference(k, got, gyro):
        kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
        for pl, (f64, f32, rows, cols) in enumerate(((sr.map64, sr.map32, r, c), (cr.chroma_map64, cr.chroma_map32, r // 2, c // 2))):
            m64, m32 = f64(gyro, A, r, c, t, d, **kw), f32(gyro, A, r, c, t, d, **kw)
            cmp_ = wc.near_frame(m64, rows, cols)
            tol = wc.tolerance(m32, m64, cmp_)
            worst = float(np.abs(got[pl].astype(np.float64) - m64)[cmp_].max())
            print("g step %d plane %d against the reference: %.3g px (tolerance %.3g, %d of %d compared)" % (k, pl, worst, tol, cmp_.sum(), cmp_.size))
            assert cmp_.sum() > 0.25 * cmp_.size and worst <= tol, (k, pl)

    against_reference(1, step(1, nv12(A, cr.CENTER)), g1)
    step(2, nv12(A, cr.LEFT))                               # only the chroma place may change
    np.testing.assert_array_equal(_u32(seen[2][0]), _u32(seen[1][0]))
    assert (_u32(seen[2][1]) != _u32(seen[1][1])).any()
    step(3, nv12(B, cr.LEFT))                               # both places change
    assert (_u32(seen[3][0]) != _u32(seen[2][0])).any() and (_u32(seen[3][1]) != _u32(seen[2][1])).any()
    step(4, rgba32(A))                                      # the luma place back to A, the chroma place untouched (B's)
    np.testing.assert_array_equal(_u32(seen[4][0]), _u32(seen[1][0]))
    step(5, nv12(A, cr.LEFT))
    same(5, 2)
    step(6, gray_rect(A))                                   # the rectifier shares the luma place
    step(7, nv12(A, cr.LEFT, rc.CACHE_OUT))                 # another output size: another ray per sample index
    assert seen[7][0].shape != seen[5][0].shape
    step(8, zoomed(A))                                      # a zoom per frame with the LENS camera uses no cache
    step(9, nv12(A, cr.CENTER))
    same(9, 1)
    p.SetGyroQuaternions(g20.quats, g20.fs, g20.t0)
    against_reference(10, step(10, nv12(A, cr.CENTER), g20), g20)
    assert (_u32(seen[10][0]) != _u32(seen[1][0])).any() and (_u32(seen[10][1]) != _u32(seen[1][1])).any()
    p.close()
