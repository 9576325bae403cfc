"""The conditions tests/test_gpu_warp_lenses.py relies on, proved from the reference alone (tests/warp_cases.py): no GPU."""
import numpy as np
import pytest

import pixel_cases as pc
import rectify_reference as rr
import stabilize_reference as sr
import warp_cases as wc


def test_the_margin_band_is_thin_for_every_lens():
    """the pixels within 1e-3 of the model's range, compared with nothing: below 1 % of 95 x 169"""
    for name in wc.LENSES:
        inr, outr = wc.range_masks(wc.lens(name), wc.grid(wc.ROWS, wc.COLS))
        share = 1.0 - inr.mean() - outr.mean()
        print("%-8s in range %.4f, out of range %.4f, margin %.4f" % (name, inr.mean(), outr.mean(), share))
        assert not (inr & outr).any() and share < 0.01, (name, share)
        assert (outr.mean() > 1e-3) == (name in wc.UNIMAGEABLE + ("half",)), name
    # the stabiliser's zoomed lens camera: its own masks
    for name in wc.STAB_LENSES:
        inr, outr = wc.range_masks(wc.stab_camera_lens(wc.lens(name), wc.ROWS, wc.COLS), wc.grid(wc.ROWS, wc.COLS))
        assert 1.0 - inr.mean() - outr.mean() < 0.01, name


def test_the_range_is_the_models_maximum_not_its_value_at_a_right_angle():
    L = wc.lens("nonmono")
    assert wc.model_max(L) > 1.5 * pc.model(L, np.pi / 2)
    for name in pc.LENSES:
        L = wc.lens(name)
        assert wc.model_max(L) == pytest.approx(pc.model(L, np.pi / 2), rel=1e-12), name


@pytest.mark.parametrize("name,motion,extra_delay,ref_row", wc.rect_cases())
def test_rectifier_cases_compare_nearly_every_in_range_pixel(name, motion, extra_delay, ref_row):
    """measured: 100 % for every lens under x1, x20, roll and rest; asserted at the 99 % the comparison needs, and at the
    measured 100 % for roll"""
    c = wc.rect_case(name, motion, extra_delay, ref_row)
    share = c["compared"].sum() / c["in_range"].sum()
    print("%-8s %-5s: compared %.4f of the in-range pixels, tolerance %.3g px" % (name, motion, share, c["tol"]))
    assert share >= 0.99
    assert share >= wc.COMPARED_SHARE[motion]
    # the tolerance is the float32 restatement's spread, a few 1e-5 px: a wrong ray by 1e-3 px cannot hide in it
    assert c["tol"] <= 4 * 6e-5, c["tol"]


@pytest.mark.parametrize("name,motion", wc.stab_cases())
def test_stabiliser_cases_compare_nearly_every_in_range_pixel(name, motion):
    """x1 and roll: 100 %.  Under x20 the path smoothed over 0.1 s lies far from the frame's own orientation and a part of
    the output looks past the frame by more than half an image: measured 63 % (strong) to 100 % (negmild) compared, the
    rest is held to `both say outside`"""
    c = wc.stab_case(name, motion)
    share = c["compared"].sum() / c["in_range"].sum()
    print("%-8s %-5s: compared %.4f of the in-range pixels, tolerance %.3g px" % (name, motion, share, c["tol"]))
    assert share >= (0.6 if motion == "x20" else 0.99)
    assert c["tol"] <= 4 * 1e-4, c["tol"]


def test_roll_fills_between_a_quarter_and_a_half_and_every_frame_differently():
    c = wc.rect_case("synth", "roll")
    x = 1.0 - rr.inside(c["m64"]).mean()
    print("roll: %.3f of the pixels are filled" % x)
    assert wc.ROLL_BAND[0] < x < wc.ROLL_BAND[1]
    for name in wc.EDGE_LENSES:
        outside, inside = wc.reference_counts(name, "roll", wc.ROWS, wc.COLS)
        print(name, outside)
        assert len(set(outside)) == 3 and min(outside) > 0.15 * wc.ROWS * wc.COLS, (name, outside)


@pytest.mark.parametrize("rows,cols", wc.EDGE_SIZES)
def test_every_edge_size_has_inside_and_outside_pixels(rows, cols):
    for name in wc.EDGE_LENSES:
        outside, inside = wc.reference_counts(name, "x1", rows, cols)
        print("%s %d x %d: outside %s inside %s" % (name, rows, cols, outside, inside))
        assert min(inside) >= 1 and min(outside) >= 1, (name, outside, inside)


def test_the_float64_reference_is_the_identity_at_rest():
    """in range, to 1e-9 px, all eight lenses -- and so is the stabiliser's at zoom 1 without smoothing"""
    g = wc.gyro("rest")
    for name in wc.LENSES:
        c = wc.rect_case(name, "rest")
        worst = np.abs(c["m64"] - wc.grid(wc.ROWS, wc.COLS))[c["in_range"]].max()
        print("%-8s rectifier at rest: %.3g px from the identity" % (name, worst))
        assert worst <= 1e-9, (name, worst)
        m = sr.map64(g, c["lens"], wc.ROWS, wc.COLS, c["time"], c["delay"])
        assert np.abs(m - wc.grid(wc.ROWS, wc.COLS))[c["in_range"]].max() <= 1e-9, name


def test_points_cases_lie_where_they_should():
    for name in wc.LENSES:
        L, p = wc.full_size_points(name)
        assert wc.N_POINTS <= len(p) <= wc.N_POINTS + 4 and wc.range_masks(L, p)[0].all(), name
        # forward_points o the true inverse is the identity at rest: the reference the device is held to is sound
        back = rr.forward_points(wc.gyro("rest"), L, wc.FULL_ROWS, wc.frame_time(), 0.037, p)
        assert np.abs(back - p).max() <= 1e-9, name
    for name in wc.UNIMAGEABLE:
        L, p = wc.out_of_range_points(name)
        assert wc.range_masks(L, p)[1].all() and len(p) >= 8, name


def test_the_cache_sequence_changes_the_map_at_every_step_that_must():
    """a stale ray map or row table shows: each change of the sequence moves the float64 map by far more than a float32 ulp (1.9e-6 px at 16 .. 32)"""
    from rssync_amd import synth
    A, B, C = wc.cache_lenses()
    g, t, r, c = wc.gyro("x1"), wc.frame_time(), wc.CACHE_ROWS, wc.CACHE_COLS
    mA = rr.map64(g, A, r, c, t, synth.D_TRUE)
    assert A[:8] == B[:8] and A[1:] == C[1:] and len(set(A)) == 9
    assert np.abs(rr.map64(g, B, r, c, t, synth.D_TRUE) - mA).max() > 1e-4
    assert np.abs(rr.map64(g, C, r, c, t, synth.D_TRUE) - mA).max() > 1e-4
    assert np.abs(rr.map64(wc.gyro("x20"), A, r, c, t, synth.D_TRUE) - mA).max() > 1e-1
    # the same nine numbers on the transposed frame: another ray per pixel index
    rays, rays_t = rr.pixel_rays(A, r, c).reshape(-1, 3), rr.pixel_rays(A, c, r).reshape(-1, 3)
    assert np.abs(rays - rays_t).max() > 1e-2
    zoomed = wc.stab_camera_lens(A, r, c)
    assert np.abs(rr.pixel_rays(zoomed, r, c).reshape(-1, 3) - rays).max() > 1e-2
