"""The conditions tests/test_gpu_render_lenses.py relies on, proved from the restatements alone (tests/render_cases.py): no GPU.
Without them its comparisons could pass for nothing: a NaN check on a plane that has no unimageable sample, a fill check where
nothing is outside, a fit whose value the tolerance leaves open, an infill that borrows nothing."""
import numpy as np
import pytest

import color_reference as cr
import limit_reference as lr
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
import zoom_reference as zr


def test_the_size_is_a_tile_and_a_part_in_the_chroma_plane():
    assert (rc.C_ROWS, rc.C_COLS) == (47, 85) and 64 < rc.C_COLS < 128 and rc.C_ROWS % 4 and 128 < rc.COLS < 192
    assert rc.OUT[0] % 2 == 0 and rc.OUT[1] % 2 == 0 and rc.OUT != (rc.ROWS, rc.COLS)
    L = rc.lens("half")
    assert (L[3], L[4]) == (42.5, 23.5)
    for name in ("aniso", "half"):      # off-centre by more than a pixel; 'aniso' with fx != fy
        L = rc.lens(name)
        assert max(abs(L[3] - rc.COLS / 2), abs(L[4] - rc.ROWS / 2)) > 1.0, name
    L = rc.lens("aniso")
    assert abs(L[1] - L[2]) > 0.2 * L[1]
    L = rc.lens("synth")            # the lens every other renderer test uses: centred, fx and fy 1.7 % apart at this size
    assert (L[3], L[4]) == (rc.COLS / 2, rc.ROWS / 2) and abs(L[1] - L[2]) < 0.02 * L[1]


@pytest.mark.parametrize("zoom", [1.0, 1.1])
def test_unimageable_samples_per_plane(zoom):
    """the measured table; every plane used for a NaN check (zoom 1: 'half', 'nonmono', 'negmild') has at least 9, either siting"""
    for name, (luma, chroma) in rc.UNIMAGEABLE[zoom].items():
        L = rc.lens(name)
        got_l = int(rc.plane_masks(L, 0, cr.CENTER, zoom, sr.LENS, None)[1].sum())
        got_c = {site: int(rc.plane_masks(L, 1, site, zoom, sr.LENS, None)[1].sum()) for site in rc.SITES}
        print("%-8s zoom %.1f: %d luma pixels, %s chroma samples beyond the range" % (name, zoom, got_l, got_c))
        assert (got_l, got_c[cr.LEFT]) == (luma, chroma), name
        assert (got_c[cr.CENTER] > 0) == (chroma > 0)
    if zoom == 1.0:
        for name in ("half", "nonmono"):
            L = rc.lens(name)
            for site in rc.SITES:
                assert rc.plane_masks(L, 1, site, zoom, sr.LENS, None)[1].sum() >= 9 and rc.plane_masks(L, 0, site, zoom, sr.LENS, None)[1].sum() >= 9


def test_outside_counts_per_frame():
    """the measured table; a roll case has three different counts, and 0 < outside < all wherever a fill is asserted"""
    for key, want in rc.OUTSIDE.items():
        name, motion, camera, plane, site = key
        got = rc.outside_counts(name, motion, plane, site, camera)
        print(key, got)
        assert tuple(got) == want, key
        if motion == "roll":
            assert len(set(got)) == 3, key
    for name, motion, zoom, camera in rc.BODY_CASES:
        for plane, n in ((0, rc.ROWS * rc.COLS), (1, rc.C_ROWS * rc.C_COLS)):
            for site in rc.SITES:
                got = rc.outside_counts(name, motion, plane, site, camera, zoom)
                L = rc.lens(name)
                nan = int(rc.plane_masks(L, plane, site, zoom, camera, None)[1].sum())
                print("%-6s %-4s zoom %.1f camera %d plane %d site %d: outside %s, beyond the range %d of %d" % (name, motion, zoom, camera, plane, site, got,
                                                                                                            nan, n))
                # (the float64 map gives a sample beyond the range some position: the device's count is at least nan)
                assert all(0 < max(g, nan) < n for g in got), (name, motion, plane)
                if (name, motion) in rc.ROLL_COUNTS_DIFFER and plane == 0:
                    assert len(set(got)) == 3
                elif motion == "roll" and plane == 0:       # 'synth' is centred: the same 4805 pixels in every frame
                    assert len(set(got)) == 1
    for name, motion, zoom in rc.PERCAM_CASES:
        L = rc.lens(name)
        nan = int(rc.plane_masks(L, 1, cr.CENTER, zoom, sr.LENS, None)[1].sum())
        out = rc.outside_counts(name, motion, 1, cr.CENTER, sr.LENS, zoom)
        assert nan >= 9 or min(out) > 0, (name, motion)


@pytest.mark.parametrize("name", rc.MAP_LENSES)
def test_plane_cases_compare_nearly_every_in_range_sample(name):
    """... and their tolerances are a few 1e-5 px: printed per case"""
    for motion in rc.MOTIONS:
        for camera in rc.CAMERAS:
            for out_size in rc.out_sizes():
                for plane, site in ((0, cr.CENTER), (1, cr.CENTER), (1, cr.LEFT)):
                    c = rc.plane_case(name, motion, plane, site, camera, rc.ZOOM, out_size)
                    share = c["compared"].sum() / max(c["in_range"].sum(), 1)
                    print("%-8s %-5s camera %d out %s plane %d site %d: compared %.3f of %d in range, tolerance %.3g px" %
                          (name, motion, camera, out_size, plane, site, share, c["in_range"].sum(), c["tol"]))
                    assert c["in_range"].sum() > 0.4 * c["in_range"].size
                    assert share >= (0.25 if motion == "x20" else 0.9), (name, motion, camera, plane)
                    assert 0 < c["tol"] <= 4 * 2.5e-4


@pytest.mark.parametrize("name", ["half", "aniso"])
def test_a_camera_from_the_image_centre_or_with_fx_and_fy_exchanged_is_far_off(name):
    """the output camera of either plane formed from the image centre instead of (cx, cy), or with fx and fy exchanged: more
    than 100 tolerances off in more than half of the compared samples, both planes, both sitings"""
    L, g = rc.lens(name), wc.gyro("x1")
    wrong = {"centre": (L[1], L[2], rc.COLS / 2, rc.ROWS / 2), "swap": (L[2], L[1], L[3], L[4])}
    for how, cam in wrong.items():
        for plane, site in ((0, cr.CENTER), (1, cr.CENTER), (1, cr.LEFT)):
            c = rc.plane_case(name, "x1", plane, site)
            kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM, cam=cam)
            if plane == 0:
                m = sr.map64(g, L, rc.ROWS, rc.COLS, c["time"], c["delay"], **kw)
            else:
                m = cr.chroma_map64(g, L, rc.ROWS, rc.COLS, c["time"], c["delay"], site, **kw)
            d = np.abs(m - c["m64"]).max(axis=-1)[c["compared"]]
            share = float((d > 100 * c["tol"]).mean())
            print("%-6s %-6s plane %d site %d: median %.3g px, %.3f of the compared samples beyond 100 tolerances (%.3g px)" %
                  (name, how, plane, site, np.median(d), share, 100 * c["tol"]))
            assert share > 0.5, (name, how, plane, site)


@pytest.mark.parametrize("case", list(rc.FIT_CASES))
def test_zoom_fit_cases_leave_the_device_no_choice(case):
    """plain, liberal and conservative reading give the listed zooms and statuses in every frame, in plane 0 and in the
    chroma plane"""
    name, motion, camera, steps, k_l, st_l, k_c, st_c = rc.FIT_CASES[case]
    for plane, borders, k, st in ((0, rc.luma_borders(name, motion, camera), k_l, st_l), (1, rc.chroma_borders(name, motion, camera), k_c, st_c)):
        tol = rc.fit_tolerance(name, motion, camera, rc.FIT_LO, plane)
        readings = rc.zoom_readings(borders, rc.FIT_LO, rc.FIT_HI, tol, steps)
        print(case, "plane", plane, "tolerance %.3g" % tol, readings[0][0].tolist(), readings[0][1].tolist())
        for z, s in readings:
            np.testing.assert_array_equal(z, rc.fit_zooms(k, steps))
            np.testing.assert_array_equal(s, st)
    if case in rc.IMAGEABILITY_FITS:
        # one step below the fitted zoom every border pixel that has a position is inside: what is outside has no ray
        for fb, z in zip(rc.luma_borders(name, motion, camera), rc.fit_zooms(k_l, steps)):
            below = z - (rc.FIT_HI - rc.FIT_LO) / (1 << steps)
            beyond, band = fb.range_band(below)
            assert beyond.any() and not fb.clear(below)
            assert sr.inside(fb.map(below), rc.ROWS, rc.COLS)[~beyond & ~band].all()


def test_the_fit_cases_hold_what_they_must():
    """per camera an off-centre lens and a call that mixes clear and not-clear frames; with the LENS camera a case set by
    imageability alone"""
    for cases, cam_at, st_at in ((rc.FIT_CASES, 2, 5), (rc.STRENGTH_CASES, 2, 5)):
        for camera in rc.CAMERAS:
            mine = [c for c in cases.values() if c[cam_at] == camera]
            assert any(c[0] == "half" for c in mine)
            assert any(0 < sum(c[st_at]) < rc.N_FRAMES for c in mine)
    assert all(rc.FIT_CASES[c][2] == sr.LENS and rc.FIT_CASES[c][0] in ("nonmono", "half") for c in rc.IMAGEABILITY_FITS)


@pytest.mark.parametrize("case", list(rc.STRENGTH_CASES))
def test_strength_fit_cases_leave_the_device_no_choice(case):
    name, motion, camera, zoom, k, st = rc.STRENGTH_CASES[case]
    tol = rc.fit_tolerance(name, motion, camera, zoom)
    readings = rc.strength_readings(rc.strength_frames(name, motion, camera, zoom), tol)
    print(case, "tolerance %.3g" % tol, readings[0][0].tolist(), readings[0][1].tolist())
    for a, s in readings:
        np.testing.assert_array_equal(a, rc.fit_strengths(k))
        np.testing.assert_array_equal(s, st)


def test_the_defaults_of_the_fit_restatements_are_unchanged():
    """zoom_reference.frame_border without a margin and limit_reference.limited_frame without gyro, lens and size: the
    scene's first frames still give FITTED and AT_106"""
    for case in ("A", "B"):
        c = zr.CASES[case]
        z, s = zr.fit64(zr.borders(case, times=zr.TIMES[:2]), c["lo"], c["hi"])
        assert tuple(z) == zr.FITTED[case][:2] and not s.any()
        a, s = lr.fit64(lr.frames(case, times=lr.TIMES[:3]))
        assert tuple(a) == lr.FITTED[case][:3] and not s.any()
    a, _ = lr.fit64(lr.frames("A", zoom=1.06, times=lr.TIMES[:3]))
    assert tuple(a) == lr.AT_106[:3]


@pytest.mark.parametrize("name,motion", rc.INFILL_CASES)
def test_infill_cases_borrow_and_leave_filled_in_both_planes(name, motion):
    for plane in (0, 1):
        lent = left = 0
        for f in range(rc.N_FRAMES):
            place, _, _ = rc.infill_hits(name, motion, plane, f)
            print("%s %s plane %d frame %d: own %d borrowed %d filled %d" % (name, motion, plane, f, (place == 0).sum(), (place > 0).sum(), (place < 0).sum()))
            lent += int((place > 0).sum())
            left += int((place < 0).sum())
        assert lent > 0 and left > 0


def test_compose_plane_is_first_hits_rule():
    """on the float64 maps of a frame's candidates compose_plane places every sample where infill_reference.first_hits does"""
    import infill_reference as ir
    from rssync_amd import synth
    name, motion = rc.INFILL_CASES[0]
    L, g, times = rc.lens(name), wc.gyro(motion), wc.frame_times()
    targets = sr.path64(g, times, L[0], synth.D_TRUE, rc.SIGMA)
    frames = rc.noise8()["y"]
    for f in range(rc.N_FRAMES):
        cand = ir.candidates(f, rc.N_FRAMES, rc.INFILL_RADIUS)
        maps = [sr.map64(g, L, rc.ROWS, rc.COLS, times[c], synth.D_TRUE, target=targets[f], zoom=rc.ZOOM) for c in cand]
        got, place = rc.compose_plane([frames[c] for c in cand], maps, rc.ROWS, rc.COLS, 77, lambda fr, m: sr.sample(fr, m)[0])
        want_place, pos, _ = rc.infill_hits(name, motion, 0, f)
        np.testing.assert_array_equal(place, want_place)
        np.testing.assert_array_equal(got, ir.compose(frames, want_place, pos, cand, 77))


def test_the_cache_sequence_changes_what_it_must():
    """section g: LEFT against CENTER moves the chroma map and not the luma map; lens B moves both; x20 moves both"""
    from rssync_amd import synth
    A, B = rc.cache_lenses()
    r, c, t, d = rc.CACHE_ROWS, rc.CACHE_COLS, wc.frame_time(), synth.D_TRUE
    g = wc.gyro("x1")
    kw = dict(sigma=rc.SIGMA, zoom=rc.ZOOM)
    cA = cr.chroma_map64(g, A, r, c, t, d, cr.CENTER, **kw)
    assert np.abs(cr.chroma_map64(g, A, r, c, t, d, cr.LEFT, **kw) - cA).max() > 1e-2
    assert np.abs(cr.chroma_map64(g, B, r, c, t, d, cr.CENTER, **kw) - cA).max() > 1e-4
    assert np.abs(sr.map64(g, B, r, c, t, d, **kw) - sr.map64(g, A, r, c, t, d, **kw)).max() > 1e-4
    assert np.abs(cr.chroma_map64(wc.gyro("x20"), A, r, c, t, d, cr.CENTER, **kw) - cA).max() > 1e-1
    other = cr.chroma_map64(g, A, r, c, t, d, cr.CENTER, out_size=rc.CACHE_OUT, **kw)
    assert other.shape != cA.shape
