"""The conditions tests/test_gpu_yuv_lenses.py relies on, proved from the restatements alone (tests/yuv_cases.py): no GPU.
Without them its comparisons could pass for nothing: a NaN check on a chroma plane that has no unimageable sample, a fill
check where nothing is outside, a fit that the luma plane decides in every frame, a map tolerance that a renderer with the
4:2:0 camera, the luma's camera or the other siting would meet as well."""
import numpy as np
import pytest

import color_reference as cr
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
import yuv_cases as yc
import yuv_reference as yr
from rssync_amd import synth


def test_the_size_is_a_tile_and_a_part_in_the_422_chroma_plane():
    assert (yc.C_ROWS, yc.C_COLS) == (94, 85) and 64 < yc.C_COLS < 128 and yc.C_ROWS % 4 and yc.COLS % 4 == 2
    assert rc.OUT[1] % 2 == 0 and yc.OUT444[0] % 2 == 1 and (yc.OUT444[1], yc.OUT444[0]) not in ((yc.ROWS, yc.COLS), rc.OUT)
    L = rc.lens("aniso")            # fx and fy far apart and off-centre: what "halved in x alone" is about
    assert abs(L[1] - L[2]) > 0.2 * L[1] and abs(L[3] - yc.COLS / 2) > 1.0 and abs(L[4] - yc.ROWS / 2) > 1.0
    L = rc.lens("half")
    assert (L[3], L[4]) == (42.5, 23.5)
    assert set(yc.FORMATS) == set(yc.F422) | set(yc.F444) and len(yc.FORMATS) == 7


def test_unimageable_samples_per_plane():
    """the measured table at zoom 1; every case whose NaN rays a GPU section asserts has at least 9 in the luma and in the
    4:2:2 chroma plane with either siting, and the other lenses of the table have none"""
    for name, want in yc.UNIMAGEABLE.items():
        L = rc.lens(name)
        got = (int(yc.plane_masks(L, 0, cr.CENTER, 1.0, sr.LENS, None)[1].sum()),) + tuple(
            int(yc.plane_masks(L, 1, site, 1.0, sr.LENS, None)[1].sum()) for site in (cr.CENTER, cr.LEFT))
        print("%-8s zoom 1.0: luma, chroma centre, chroma left beyond the range: %s" % (name, got))
        assert got == want, name
        assert want[0] == rc.UNIMAGEABLE[1.0].get(name, (0, 0))[0]
    for name in ("aniso", "strong", "synth"):
        assert yc.UNIMAGEABLE[name] == (0, 0, 0)
    # section b: the cases with the LENS camera at zoom 1; section c: the lenses named for their NaN rays
    nan_cases = [c[0] for c in rc.BODY_CASES if c[2] == 1.0 and c[3] == sr.LENS]
    assert nan_cases and {"half", "nonmono"} <= {c[0] for c in rc.PERCAM_CASES if c[2] == 1.0}
    for name in nan_cases + ["half", "nonmono"]:
        assert min(yc.UNIMAGEABLE[name]) >= 9, name
    # a PINHOLE camera gives every sample a ray
    assert not yc.plane_masks(rc.lens("half"), 1, cr.CENTER, 1.0, sr.PINHOLE, None)[1].any()


def test_outside_counts_per_frame_of_every_body_case():
    """section b asserts a fill and both counters: in the float64 map every frame of every case has samples outside and
    samples inside, in the luma and in the 4:2:2 chroma plane with either siting; under roll 'negmild' has three counts"""
    for name, motion, zoom, camera in rc.BODY_CASES:
        for plane, n in ((0, yc.ROWS * yc.COLS), (1, yc.C_ROWS * yc.C_COLS)):
            for site in rc.SITES if plane else (cr.CENTER,):
                got = yc.outside_counts(name, motion, plane, site, camera, zoom)
                print("%-7s %-4s zoom %.1f camera %d plane %d site %d: outside %s of %d" % (name, motion, zoom, camera, plane, site, got, n))
                assert all(0 < g < n for g in got), (name, motion, plane, site)
                if (name, motion) in rc.ROLL_COUNTS_DIFFER and plane == 0:
                    assert len(set(got)) == 3
    # section c: every per-frame case fills samples of the chroma plane, by a NaN ray or by the motion
    for name, motion, zoom in rc.PERCAM_CASES:
        nan = int(yc.plane_masks(rc.lens(name), 1, cr.CENTER, zoom, sr.LENS, None)[1].sum())
        assert nan >= 9 or min(yc.outside_counts(name, motion, 1, cr.CENTER, sr.LENS, zoom)) > 0, (name, motion)


@pytest.mark.parametrize("name", rc.MAP_LENSES)
def test_map_cases_compare_at_least_half_of_their_in_range_samples(name):
    """... and their tolerances are around 1e-4 px: printed per case"""
    for motion in rc.MOTIONS:
        for camera in rc.CAMERAS:
            for out_size in rc.out_sizes() + (yc.OUT444,):
                for plane, site in ((0, cr.CENTER),) + (((1, cr.CENTER), (1, cr.LEFT)) if out_size != yc.OUT444 else ()):
                    c = yc.plane_case(name, motion, plane, site, camera, rc.ZOOM, out_size)
                    share = c["compared"].sum() / max(c["in_range"].sum(), 1)
                    print("%-8s %-5s camera %d out %s plane %d site %d: compared %.3f of %d in range, tolerance %.3g px" %
                          (name, motion, camera, out_size, plane, site, share, c["in_range"].sum(), c["tol"]))
                    assert c["in_range"].sum() > 0.4 * c["in_range"].size
                    assert share >= 0.5, (name, motion, camera, plane)
                    assert 0 < c["tol"] <= 4 * 2.5e-4


def _wrong_chroma_maps(name, site, zoom=rc.ZOOM):
    """the maps of 4:2:2 chroma samples that a renderer with another camera would give, in the case's own coordinates where
    it has any: the output camera with cy halved (the 4:2:0 rule), with fx kept and fy halved, with the siting's offset left
    out of the lens and the camera (the other siting's map), and the luma's positions of the samples' own places"""
    L, g = rc.lens(name), wc.gyro("x1")
    t = float(wc.frame_times()[1])
    q_t = sr.path64(g, np.array([t]), L[0], synth.D_TRUE, rc.SIGMA)[0]
    fx, fy, cx, cy = yr.chroma_camera422(L, yc.ROWS, yc.COLS, yc.ROWS, yc.COLS, site, zoom)
    kw = dict(target=q_t, out_size=(yc.C_COLS, yc.C_ROWS))
    lens_c = yr.chroma_lens422(L, site)
    out = {"cy halved": sr.map64(g, lens_c, yc.C_ROWS, yc.C_COLS, t, synth.D_TRUE, cam=(fx, fy, cx, cy * 0.5), **kw),
           "fx and fy exchanged": sr.map64(g, lens_c, yc.C_ROWS, yc.C_COLS, t, synth.D_TRUE, cam=(fx * 2.0, fy * 0.5, cx, cy), **kw),
           "4:2:0 lens": sr.map64(g, cr.chroma_lens(L, site), yc.C_ROWS, yc.C_COLS, t, synth.D_TRUE, cam=(fx, fy, cx, cy), **kw),
           "other siting": yc.plane_case(name, "x1", 1, cr.LEFT if site == cr.CENTER else cr.CENTER, sr.LENS, zoom)["m64"],
           "luma": yc.plane_case(name, "x1", 0, cr.CENTER, sr.LENS, zoom)["m64"][:, 0:2 * yc.C_COLS:2]}
    return out


@pytest.mark.parametrize("name", ["half", "aniso"])
def test_a_422_chroma_map_from_another_camera_is_far_off(name):
    """a wrong chroma principal point, exchanged fx / fy factors, the 4:2:0 lens or the luma's own map: more than 100
    tolerances off in more than half of the compared samples; the other siting's map (ox left out): more than 20, which at
    zoom 1.1 is a shift of 0.5 (1 - 1 / 1.1) / 2 = 0.023 chroma px.  And the planes of noise and their fills differ, so
    that no plane's bytes pass for another's."""
    for site in rc.SITES:
        c = yc.plane_case(name, "x1", 1, site)
        for how, m in _wrong_chroma_maps(name, site).items():
            assert m.shape == c["m64"].shape, how
            d = np.abs(m - c["m64"]).max(axis=-1)[c["compared"]]
            factor = 20 if how == "other siting" else 100
            share = float((d > factor * c["tol"]).mean())
            print("%-6s site %d %-20s median %.3g px, %.3f of the compared samples beyond %d tolerances (%.3g px)" %
                  (name, site, how, np.median(d), share, factor, factor * c["tol"]))
            assert share > 0.5, (name, site, how)
    # the 4:2:0 chroma map of the same lens is not even of this shape
    assert rc.plane_case(name, "x1", 1, cr.CENTER)["m64"].shape != yc.plane_case(name, "x1", 1, cr.CENTER)["m64"].shape


def test_the_planes_of_noise_and_their_fills_differ():
    for depth in (8, 10, 16):
        d = yc.noise(depth)
        assert d["y"].max() >= (1 << depth) - 2 and d["y"].min() <= 1          # (the whole range)
        for a, b in (("u", "v"), ("u4", "v4"), ("y", "u4"), ("y", "v4")):
            assert (d[a] != d[b]).mean() > 0.9, (depth, a, b)
        assert (d["u"] != d["u4"][:, :, :yc.C_COLS]).mean() > 0.9
        assert len(set(yc.FILLS[depth])) == 3 and max(yc.FILLS[depth]) < (1 << depth)
    for fmt in yc.FORMATS:
        fr = yc.frames(fmt)
        assert len(fr) == (2 if yc.SIBLING.get(fmt, fmt) == yc.NV16 else 3)
        assert fr[0].dtype == (np.uint8 if yc.DEPTH[fmt] == 8 else np.uint16)
        assert fr[1].shape[:3] == (rc.N_FRAMES,) + yc.plane_size(fmt, 1)
    y, uv = yc.frames(yc.P210)
    assert (y & 63).max() == 0 and (uv & 63).max() == 0 and y.max() > 1023 << 5
    # the sampler of a container format works on the values and gives back words: on an identity map the words themselves
    ident = wc.grid(yc.C_ROWS, yc.C_COLS)
    for filter in (0, 1):
        out, n = yc.sample_plane(yc.P210, uv[0], ident, (1, 2), filter)
        assert n == 0
        np.testing.assert_array_equal(out, uv[0])


@pytest.mark.parametrize("case", list(yc.FIT_CASES))
def test_fit_cases_leave_the_device_no_choice(case):
    """plain, liberal and conservative reading give the listed zooms and statuses in every frame, in plane 0 and in the
    4:2:2 chroma plane"""
    name, motion, camera, site, steps, k_l, st_l, k_c, st_c = yc.FIT_CASES[case]
    for plane, k, st in ((0, k_l, st_l), (1, k_c, st_c)):
        readings = yc.fit_readings(name, motion, camera, steps, plane, site)
        print(case, "plane", plane, readings[0][0].tolist(), readings[0][1].tolist())
        for z, s in readings:
            np.testing.assert_array_equal(z, rc.fit_zooms(k, steps))
            np.testing.assert_array_equal(s, st)


def test_the_fit_cases_hold_what_they_must():
    """every lens, motion and camera of rc.FIT_CASES with either siting; the luma columns are rc's own where the step count
    is; a frame decided by the chroma plane, one decided by the luma plane, and a call with both statuses"""
    assert {c[:3] for c in yc.FIT_CASES.values()} == {c[:3] for c in rc.FIT_CASES.values()}
    assert {(c[:3], c[3]) for c in yc.FIT_CASES.values()} == {(c[:3], s) for c in rc.FIT_CASES.values() for s in rc.SITES}
    for c in yc.FIT_CASES.values():
        (theirs,) = [r for r in rc.FIT_CASES.values() if r[:3] == c[:3]]
        if theirs[3] == c[4]:
            assert (c[5], c[6]) == (theirs[4], theirs[5])
    for case in yc.CHROMA_DECIDES:
        c = yc.FIT_CASES[case]
        assert any(kc > kl for kl, kc, sl, sc in zip(c[5], c[7], c[6], c[8]) if not sl and not sc), case
    for case in yc.LUMA_DECIDES:
        c = yc.FIT_CASES[case]
        assert any(kl > kc for kl, kc in zip(c[5], c[7])), case
    for case in yc.MIXED_STATUS:
        c = yc.FIT_CASES[case]
        assert 0 < sum(np.array(c[6]) | np.array(c[8])) < rc.N_FRAMES, case
    assert yc.CHROMA_DECIDES and yc.LUMA_DECIDES and yc.MIXED_STATUS


def test_the_cache_sequence_changes_what_it_must():
    """section e: the 4:2:2 chroma map is not the 4:2:0 map of the same lens; LEFT against CENTER and lens B move it; and
    the trap's two calls have one chroma camera between them, bit for bit, with maps of different heights"""
    A, B = rc.cache_lenses()
    r, c, t, d = rc.CACHE_ROWS, rc.CACHE_COLS, wc.frame_time(), synth.D_TRUE
    g = wc.gyro("x1")
    kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
    m422 = yr.chroma_map64(g, A, r, c, t, d, cr.CENTER, **kw)
    m420 = cr.chroma_map64(g, A, r, c, t, d, cr.CENTER, **kw)
    assert m422.shape == (r, c // 2, 2) and m420.shape == (r // 2, c // 2, 2)
    assert np.abs(m422[:r // 2] - m420).max() > 1.0           # (the upper half of the one against the other)
    assert np.abs(yr.chroma_map64(g, A, r, c, t, d, cr.LEFT, **kw) - m422).max() > 1e-2
    assert np.abs(yr.chroma_map64(g, B, r, c, t, d, cr.CENTER, **kw) - m422).max() > 1e-4
    assert yr.chroma_map64(g, A, r, c, t, d, cr.CENTER, out_size=rc.CACHE_OUT, **kw).shape != m422.shape
    cam_420, cam_422 = yc.cache_trap_cameras()
    for site in rc.SITES:
        a = cr.chroma_camera(A, r, c, r, c, site, rc.ZOOM, cam_420)
        b = yr.chroma_camera422(A, r, c, r, c, site, rc.ZOOM, cam_422)
        assert tuple(a) == tuple(b), (site, a, b)
        # ... which is not lens B's with the other siting, what the call before the trap leaves in the cache
        assert tuple(b) != tuple(yr.chroma_camera422(B, r, c, r, c, cr.LEFT, rc.ZOOM))
