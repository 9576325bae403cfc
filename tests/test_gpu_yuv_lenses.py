"""The 4:2:2 and 4:4:4 renderers on the device -- the constant camera (include/rssync_yuv.h, csrc/kernels/yuv.hpp) and a zoom
per frame (include/rssync_zoomyuv.h, csrc/kernels/zoomyuv.hpp) -- across the lenses and motions of tests/warp_cases.py:
off-centre, anisotropic and strongly distorted lenses, lenses that cannot image every sample (NaN rays), the scene's motion, its
20-fold and a 250 rad/s roll (tests/yuv_cases.py; the conditions these comparisons rest on are proved in
tests/test_yuv_cases_cpu.py).  94 x 170 luma, 94 x 85 chroma: more than one tile and part tiles in both planes, an output
width that is 2 mod 4.  What tests/test_gpu_render_lenses.py is to the 4:2:0, RGBA and gray renderers.

     what is compared                                                   kernels and paths reached
  a  yuv_map of plane 0 and plane 1 against float64 (NV16; every other   the host's 4:2:2 chroma camera of both sitings (color_host.hpp,
     4:2:2 format's map IS NV16's, a 4:4:4 format's plane 1 its plane    color_chroma422_camera), the ray maps of both cache places (LENS), the
     0), both sitings, both cameras, two output sizes and an odd one     map kernel with the chroma extent (width / 2, height)
  b  the bytes and both counters of every body with both samplers, from  yuv422_8 (NV16, I422), yuv422_16 (P210, P216, I210), yuv444_8 (I444) and
     the numpy samplers on the device's own map; NaN rays in both planes yuv444_16 (I410), FILTER 0 and 1, under YuvPos<LENS> and YuvPos<PINHOLE>;
                                                                         yuv_count2's three ballots
  c  a zoom per frame against the constant-camera call at that zoom,     the framecam_* kernels (FramecamPos, rays computed in place in fp64), the
     bytes and counts, seven formats, both samplers, both cameras        LDS-staged I422 / I210 kernels with the LENS camera and NaN rays
  d  fit_zoom_yuv against the float64 bisection of both planes, exactly  rssync_zoomyuv_fit: zoom_fit_kernel on the luma's and on the 4:2:2 chroma
                                                                         plane's camera, the maximum and the OR-ed status
  e  one problem through fifteen calls that must refresh one, both or    both places of the ray-map cache (rect_rays_into) under 4:2:0, 4:2:2 and
     none of the two cached ray maps, against fresh problems             4:4:4 calls, among them two whose chroma keys differ in the height alone
"""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import color_reference as cr
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
import yuv_cases as yc
import yuv_reference as yr

pytestmark = pytest.mark.gpu

NV12 = 1                                                                                         # section e's 4:2:0 calls
BODIES = {"yuv422_8-nv16": yc.NV16, "yuv422_8-i422": yc.I422, "yuv422_16-p210": yc.P210, "yuv422_16-p216": yc.P216,
          "yuv422_16-i210": yc.I210, "yuv444_8-i444": yc.I444, "yuv444_16-i410": yc.I410}          # section b


def _problem(gyro):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def problems(built):
    """one problem per motion"""
    return {m: _problem(wc.gyro(m)) for m in rc.MOTIONS}


# a -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,motion", [(n, m) for n in rc.MAP_LENSES for m in rc.MOTIONS])
def test_a_plane_maps_against_the_float64_reference(problems, name, motion):
    """plane 1's range masks are those of the 4:2:2 chroma output camera taken as a lens (yc.plane_masks).  rssync_yuv_map
    offers plane 0 and plane 1 alone: the third plane of a planar format has no map of its own to ask for, and section b
    holds its bytes to plane 1's (4:4:4: plane 0's) map."""
    p, L, worst = problems[motion], rc.lens(name), 0.0
    for camera in rc.CAMERAS:
        for out_size in rc.out_sizes():
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, camera=camera, out_size=out_size)
            c = yc.plane_case(name, motion, 0, cr.CENTER, camera, rc.ZOOM, out_size)
            args = (rc.COLS, rc.ROWS, L, c["time"], c["delay"])
            m0 = p.yuv_map(yc.NV16, 0, *args, **kw)
            worst = max(worst, rc.check_map("a %s %s camera %d out %s plane 0" % (name, motion, camera, out_size), m0, c, rc.ROWS, rc.COLS))
            for fmt in yc.FORMATS:          # (plane 0 does not know the format or the siting, nor does a 4:4:4 format's plane 1)
                for site in rc.SITES:
                    for pl in (0, 1) if fmt in yc.F444 else (0,):
                        np.testing.assert_array_equal(rc.u32(p.yuv_map(fmt, pl, *args, chroma_site=site, **kw)), rc.u32(m0), err_msg=yc.NAMES[fmt])
            for site in rc.SITES:
                c = yc.plane_case(name, motion, 1, site, camera, rc.ZOOM, out_size)
                m1 = p.yuv_map(yc.NV16, 1, *args, chroma_site=site, **kw)
                worst = max(worst, rc.check_map("a %s %s camera %d out %s plane 1 site %d" % (name, motion, camera, out_size, site), m1, c,
                                                yc.C_ROWS, yc.C_COLS))
                for fmt in yc.F422:
                    np.testing.assert_array_equal(rc.u32(p.yuv_map(fmt, 1, *args, chroma_site=site, **kw)), rc.u32(m1), err_msg=yc.NAMES[fmt])
        # an odd output width, which the 4:4:4 formats alone take
        kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, camera=camera, out_size=yc.OUT444)
        c = yc.plane_case(name, motion, 0, cr.CENTER, camera, rc.ZOOM, yc.OUT444)
        m0 = p.yuv_map(yc.I444, 0, rc.COLS, rc.ROWS, L, c["time"], c["delay"], **kw)
        worst = max(worst, rc.check_map("a %s %s camera %d out %s 4:4:4" % (name, motion, camera, yc.OUT444), m0, c, rc.ROWS, rc.COLS))
        for fmt, pl in ((yc.I444, 1), (yc.I410, 0), (yc.I410, 1)):
            np.testing.assert_array_equal(rc.u32(p.yuv_map(fmt, pl, rc.COLS, rc.ROWS, L, c["time"], c["delay"], **kw)), rc.u32(m0))
    print("section a largest distance %.3g px" % worst)


# b -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(rc.BODY_CASES)), ids=["%s-%s" % c[:2] for c in rc.BODY_CASES])
@pytest.mark.parametrize("body", list(BODIES))
def test_b_bodies_bytes_and_counts_from_the_devices_own_map(problems, body, case):
    """three frames per call, distinct fills per plane, noise over the format's whole range, pitched output whose padding
    stays; per plane every byte is the numpy sampler's on the device's map of that plane, every outside sample the plane's
    stored fill, and both counters the maps' outside counts (4:4:4: the two are equal)"""
    from rssync_amd import synth
    name, motion, zoom, camera = rc.BODY_CASES[case]
    fmt, site = BODIES[body], (cr.LEFT, cr.CENTER)[case % 2]
    p, L, times = problems[motion], rc.lens(name), wc.frame_times()
    src, fills = yc.frames(fmt), yc.fills(fmt)
    kw = dict(sigma=rc.SIGMA, zoom=zoom, camera=camera, chroma_site=site)
    maps = [[p.yuv_map(fmt, pl, rc.COLS, rc.ROWS, L, t, synth.D_TRUE, **kw) for pl in (0, 1)] for t in times]
    sizes = [yc.plane_size(fmt, pl) for pl in (0, 1)]
    outside = np.array([[int((~sr.inside(m, *sizes[pl])).sum()) for pl, m in enumerate(mk)] for mk in maps], np.uint64)
    if fmt in yc.F444:
        np.testing.assert_array_equal(outside[:, 1], outside[:, 0])
    if camera == sr.LENS:
        for pl in (0, 1):
            outr = yc.plane_masks(L, pl if fmt in yc.F422 else 0, site, zoom, camera, None)[1]
            for f in range(rc.N_FRAMES):
                assert maps[f][pl].shape[:2] == outr.shape and np.isnan(maps[f][pl][outr]).all()
            assert (outside[:, pl] >= outr.sum()).all()
            if zoom == 1.0:
                assert outr.sum() >= 9        # NaN rays in this plane
    shift = yc.SHIFT.get(fmt, 0)
    for filter in (0, 1):
        pad_value = 0xABCD if yc.DEPTH[fmt] > 8 else 0xAB
        whole, views = zip(*[rc.padded(a.shape, a.dtype, pad_value) for a in src])
        res, n_out = p.stabilize_yuv(fmt, src, times, L, synth.D_TRUE, fills=fills, filter=filter, out=views, **kw)
        print("b %s %s %s zoom %.1f camera %d filter %d: outside %s" % (body, name, motion, zoom, camera, filter, n_out.tolist()))
        np.testing.assert_array_equal(n_out, outside)
        for pl in (0, 1):
            assert (n_out[:, pl] > 0).all() and (n_out[:, pl] < sizes[pl][0] * sizes[pl][1]).all()
        if (name, motion) in rc.ROLL_COUNTS_DIFFER:
            assert len(set(n_out[:, 0].tolist())) == 3
        for k, (w, v) in enumerate(zip(whole, views)):
            pl = min(k, 1)
            for f in range(rc.N_FRAMES):
                m = maps[f][pl]
                want, n = yc.sample_plane(fmt, src[k][f], m, yc.plane_fill(fmt, k), filter)
                np.testing.assert_array_equal(v[f], want, err_msg="%s plane %d frame %d filter %d" % (body, k, f, filter))
                assert n == int(outside[f, pl])
                miss = ~sr.inside(m, *sizes[pl])
                stored = np.asarray(yc.plane_fill(fmt, k)) << shift
                assert miss.any() and (v[f][miss] == stored).all(), (body, k, f)
            if shift:
                assert (v & ((1 << shift) - 1)).max() == 0, (body, k)        # P210's words keep their low six bits zero
            pad = np.ones(w.shape, bool)
            pad[:, 1:1 + v.shape[1], 4:4 + v.shape[2]] = False
            assert (w[pad] == pad_value).all(), (body, k)


# c -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", rc.CAMERAS, ids=["lens", "pinhole"])
@pytest.mark.parametrize("name,motion,zoom", rc.PERCAM_CASES)
def test_c_a_zoom_per_frame_is_the_constant_camera_at_that_zoom(problems, name, motion, zoom, camera):
    """three equal zooms: the bytes and counts of the constant-camera call, which section b anchors; three different zooms:
    every frame is the single-frame constant-camera call at its zoom.  With the LENS camera 'half' and 'nonmono' have NaN
    rays in both planes: computed in place here, read from the cached ray map there."""
    from rssync_amd import synth
    p, L, times = problems[motion], rc.lens(name), wc.frame_times()
    site = cr.LEFT if name in ("half", "strong") else cr.CENTER
    filled = 0
    for fmt in yc.FORMATS:
        frames = yc.frames(fmt)
        for filter in (0, 1):
            kw = dict(sigma=rc.SIGMA, camera=camera, filter=filter, chroma_site=site, fills=yc.fills(fmt))
            what = "%s %s camera %d format %s filter %d" % (name, motion, camera, yc.NAMES[fmt], filter)
            got, n = p.stabilize_yuv_zoomed(fmt, frames, times, L, synth.D_TRUE, [zoom] * rc.N_FRAMES, **kw)
            want, want_n = p.stabilize_yuv(fmt, frames, times, L, synth.D_TRUE, zoom=zoom, **kw)
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(a, b, err_msg="%s equal zooms plane %d" % (what, k))
            np.testing.assert_array_equal(n, want_n, err_msg=what)
            filled += int(n.sum())
            got, n = p.stabilize_yuv_zoomed(fmt, frames, times, L, synth.D_TRUE, rc.PERCAM_ZOOMS, **kw)
            for f, z in enumerate(rc.PERCAM_ZOOMS):
                want, want_n = p.stabilize_yuv(fmt, yc.frames(fmt, slice(f, f + 1)), times[f:f + 1], L, synth.D_TRUE, zoom=z, **kw)
                for k, (a, b) in enumerate(zip(got, want)):
                    np.testing.assert_array_equal(a[f], b[0], err_msg="%s frame %d at zoom %.1f plane %d" % (what, f, z, k))
                np.testing.assert_array_equal(n[f], want_n[0], err_msg="%s frame %d" % (what, f))
                if f == 0 and camera == sr.LENS and z == 1.0 and name in ("half", "nonmono"):
                    for pl in (0, 1):       # the samples without a ray are among the filled ones, in both planes
                        outr = yc.plane_masks(L, pl if fmt in yc.F422 else 0, site, z, camera, None)[1]
                        assert outr.sum() >= 9 and int(want_n[0, pl]) >= outr.sum(), (what, pl)
    print("c %s %s camera %d: %d samples filled in all" % (name, motion, camera, filled))
    assert filled > 0 or camera == sr.PINHOLE


# d -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(yc.FIT_CASES))
def test_d_fitted_zooms_are_the_float64_bisections_of_both_planes(problems, case):
    """include/rssync_zoomyuv.h: a 4:2:2 format's zoom is the larger of plane 0's and the chroma plane's (a camera of its own,
    half as wide, at the luma's frame times against the path at those times), the statuses OR-ed; a 4:4:4 format's is the
    luma's.  Both from the float64 bisection, whose three readings agree (tests/test_yuv_cases_cpu.py)."""
    from rssync_amd import synth
    name, motion, camera, site, steps, k_l, st_l, k_c, st_c = yc.FIT_CASES[case]
    p, L = problems[motion], rc.lens(name)
    args = (rc.COLS, rc.ROWS, L, wc.frame_times(), synth.D_TRUE, rc.FIT_LO, rc.FIT_HI)
    kw = dict(steps=steps, sigma=rc.SIGMA, camera=camera, chroma_site=site)
    want_l, want_c = rc.fit_zooms(k_l, steps), rc.fit_zooms(k_c, steps)
    for fmt in yc.F444:
        z, st = p.fit_zoom_yuv(fmt, *args, **kw)
        np.testing.assert_array_equal(z, want_l, err_msg=yc.NAMES[fmt])
        np.testing.assert_array_equal(st, np.array(st_l, np.uint32))
    z, st = p.fit_zoom_yuv(yc.NV16, *args, **kw)
    print("d %s: NV16 %s %s; luma alone %s, chroma alone %s" % (case, z.tolist(), st.tolist(), want_l.tolist(), want_c.tolist()))
    assert z.dtype == np.float64 and st.dtype == np.uint32
    np.testing.assert_array_equal(z, np.maximum(want_l, want_c))
    np.testing.assert_array_equal(st, np.array(st_l, np.uint32) | np.array(st_c, np.uint32))
    for fmt in yc.F422:
        again, st2 = p.fit_zoom_yuv(fmt, *args, **kw)
        np.testing.assert_array_equal(again.view(np.uint64), z.view(np.uint64), err_msg=yc.NAMES[fmt])
        np.testing.assert_array_equal(st2, st)
    if case in yc.CHROMA_DECIDES:
        assert (z > want_l).any()
    if case in yc.LUMA_DECIDES:
        assert (z > want_c).any()
    if case in yc.MIXED_STATUS:         # clear and not-clear frames in one call, each in its place
        assert set(st.tolist()) == {rc.CLEAR, rc.NOT_CLEAR} and (z[st == rc.NOT_CLEAR] == rc.FIT_HI).all()


# e -----------------------------------------------------------------------------------------------------------------------
def test_e_the_ray_cache_across_chroma_geometries(built):
    """after every step the long-lived problem gives the bits of a freshly constructed one: maps, planes, counts (at most two
    contexts alive); a step that returns to an earlier configuration gives that step's bits"""
    from rssync_amd import synth
    A, B = rc.cache_lenses()
    cam_420, cam_422 = yc.cache_trap_cameras()
    r, c, t, d = rc.CACHE_ROWS, rc.CACHE_COLS, wc.frame_time(), synth.D_TRUE
    rng = np.random.default_rng([9, r, c])
    y, u4, v4 = (rng.integers(0, 256, (1, r, c), dtype=np.uint8) for _ in range(3))
    uv420 = rng.integers(0, 256, (1, r // 2, c // 2, 2), dtype=np.uint8)
    uv422 = rng.integers(0, 256, (1, r, c // 2, 2), dtype=np.uint8)
    g1 = wc.gyro("x1")

    def nv12(L, site, out_camera=None):
        def run(p):
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, chroma_site=site, out_camera=out_camera)
            m0, m1 = (p.color_map(NV12, pl, c, r, L, t, d, **kw) for pl in (0, 1))
            (oy, ouv), n = p.stabilize_color(NV12, (y, uv420), [t], L, d, fills=(1, 2, 3), **kw)
            return m0, m1, oy, ouv, n
        return run

    def nv16(L, site, out_size=None, out_camera=None):
        def run(p):
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, chroma_site=site, out_size=out_size, out_camera=out_camera)
            m0, m1 = (p.yuv_map(yc.NV16, pl, c, r, L, t, d, **kw) for pl in (0, 1))
            (oy, ouv), n = p.stabilize_yuv(yc.NV16, (y, uv422), [t], L, d, fills=(1, 2, 3), **kw)
            return m0, m1, oy, ouv, n
        return run

    def i444(L):
        def run(p):
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
            (oy, ou, ov), n = p.stabilize_yuv(yc.I444, (y, u4, v4), [t], L, d, fills=(1, 2, 3), **kw)
            return p.yuv_map(yc.I444, 1, c, r, L, t, d, **kw), oy, ou, ov, n
        return run

    def gray(L):
        def run(p):
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
            out, n = p.stabilize_frames(y, [t], L, d, fill=wc.FILL, **kw)
            return p.stabilize_map(c, r, L, t, d, **kw), out, n
        return run

    def zoomed(L):
        def run(p):
            (oy, ouv), n = p.stabilize_yuv_zoomed(yc.NV16, (y, uv422), [t], L, d, [1.2], sigma=rc.SIGMA, camera=sr.LENS, fills=(1, 2, 3))
            return oy, ouv, n
        return run

    p = _problem(g1)
    seen = {}

    def step(k, run):
        got = run(p)
        fresh = _problem(g1)
        want = run(fresh)
        fresh.close()
        for i, (a, b) in enumerate(zip(got, want)):
            a, b = (rc.u32(x) if x.dtype == np.float32 else x for x in (a, b))
            np.testing.assert_array_equal(a, b, err_msg="step %d: result %d" % (k, i))
        seen[k] = got
        return got

    def same(k, j):
        for a, b in zip(seen[k], seen[j]):
            a, b = (rc.u32(x) if x.dtype == np.float32 else x for x in (a, b))
            np.testing.assert_array_equal(a, b, err_msg="step %d is not step %d" % (k, j))

    def against_reference(k, got):
        kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
        for pl, (f64, f32, rows, cols) in enumerate(((sr.map64, sr.map32, r, c), (yr.chroma_map64, yr.chroma_map32, r, c // 2))):
            m64, m32 = f64(g1, A, r, c, t, d, **kw), f32(g1, A, r, c, t, d, **kw)
            cmp_ = wc.near_frame(m64, rows, cols)
            tol = wc.tolerance(m32, m64, cmp_)
            worst = float(np.abs(got[pl].astype(np.float64) - m64)[cmp_].max())
            print("e step %d plane %d against the reference: %.3g px (tolerance %.3g, %d of %d compared)" % (k, pl, worst, tol, cmp_.sum(), cmp_.size))
            assert cmp_.sum() > 0.25 * cmp_.size and worst <= tol, (k, pl)

    step(1, nv12(A, cr.CENTER))
    against_reference(2, step(2, nv16(A, cr.CENTER)))       # the same lens and size: the chroma place must refresh, the luma's not
    np.testing.assert_array_equal(rc.u32(seen[2][0]), rc.u32(seen[1][0]))
    assert seen[2][1].shape == (r, c // 2, 2) and seen[1][1].shape == (r // 2, c // 2, 2)
    step(3, i444(A))                                        # no chroma place
    np.testing.assert_array_equal(rc.u32(seen[3][0]), rc.u32(seen[2][0]))
    step(4, gray(A))
    step(5, zoomed(A))                                      # rays computed in place: the cache untouched
    step(6, nv16(A, cr.CENTER))                             # a reuse of both places
    same(6, 2)
    step(7, nv16(A, cr.LEFT))                               # only the chroma place may change
    np.testing.assert_array_equal(rc.u32(seen[7][0]), rc.u32(seen[6][0]))
    assert (rc.u32(seen[7][1]) != rc.u32(seen[6][1])).any()
    step(8, nv16(A, cr.LEFT, rc.CACHE_OUT))                 # another output size: another ray per sample index
    assert seen[8][0].shape != seen[7][0].shape and seen[8][1].shape != seen[7][1].shape
    step(9, nv16(B, cr.LEFT))                               # both places change
    assert (rc.u32(seen[9][0]) != rc.u32(seen[7][0])).any() and (rc.u32(seen[9][1]) != rc.u32(seen[7][1])).any()
    step(10, nv12(A, cr.CENTER))
    same(10, 1)
    # two calls whose chroma output cameras are the same four numbers (tests/test_yuv_cases_cpu.py): the 4:2:0 call's ray map
    # is the upper half of the 4:2:2 call's, whose lower half a cache keyed without the height would leave as step 11 wrote
    # it.  (The ray maps alone: the two planes' input lenses differ, so their position maps do.)
    step(11, nv16(B, cr.LEFT))
    same(11, 9)
    step(12, nv12(A, cr.CENTER, out_camera=cam_420))
    step(13, nv16(A, cr.CENTER, out_camera=cam_422))
    assert (rc.u32(seen[13][1]) != rc.u32(seen[2][1])).any()
    step(14, nv12(A, cr.CENTER, out_camera=cam_420))        # ... and back: the shorter map after the taller
    same(14, 12)
    step(15, nv12(A, cr.CENTER))
    same(15, 1)
    p.close()
