"""The conditions tests/test_gpu_infill_lenses.py relies on, proved from the restatements alone (tests/infill_cases.py): no GPU.
Without them its comparisons could pass for nothing: an infill that borrows from one place only or leaves nothing filled, a
NaN check on a plane in which every sample has a ray, a composition that places samples by another rule than the
restatement's, a map check that compares a handful of samples."""
import numpy as np
import pytest

import infill_cases as ic
import infill_reference as ir
import render_cases as rc
import stabilize_reference as sr
import warp_cases as wc
from rssync_amd import synth

PLANES = [(name, kind) for name in ic.CASES for kind in ic.kinds(name)]


def test_radius_2_on_three_frames_gives_the_three_orders_with_skipped_steps():
    for f, order in enumerate(ic.ORDERS):
        assert ir.candidates(f, ic.N_FRAMES, ic.RADIUS) == order
    # frame 0 has no f - 1 and no f - 2, frame 2 no f + 1 and no f + 2: two of the five steps are skipped in each
    steps = lambda f: [f] + [g for d in (1, 2) for g in (f - d, f + d)]  # noqa: E731
    assert [k for k, g in enumerate(steps(0)) if not 0 <= g < 3] == [1, 3]
    assert [k for k, g in enumerate(steps(2)) if not 0 <= g < 3] == [2, 4]
    assert len(ic.pairs()) == 9


@pytest.mark.parametrize("name,kind", PLANES)
def test_every_plane_borrows_from_both_later_places_and_leaves_samples_filled(name, kind):
    """counted over the samples in the lens model's range: the restatement extrapolates where the device has NaN"""
    not_in_range, rows = ic.counts(name, kind)
    print("%s %s: %d not in range, per frame [own, 2nd, 3rd, filled] %s" % (name, kind, not_in_range, list(rows)))
    assert (not_in_range, rows) == ic.COUNTS[(name, kind)]
    total = np.array(rows).sum(0)
    assert total[1] > 0 and total[2] > 0 and total[3] > 0
    inr = ic.masks(ic.case(name), kind)[0]
    assert all(sum(r) == inr.sum() for r in rows) and not_in_range + inr.sum() == inr.size
    assert inr.shape == ic.out_shape(ic.case(name), kind)


@pytest.mark.parametrize("name", ic.HALF_CASES)
def test_half_has_samples_without_a_ray_in_every_plane(name):
    c = ic.case(name)
    for kind in ic.kinds(name):
        outr = ic.masks(c, kind)[1]
        print("%s %s: %d of %d samples beyond the model's range" % (name, kind, outr.sum(), outr.size))
        assert outr.sum() >= ic.MIN_NAN
    for other in ic.CASES.values():          # a PINHOLE camera gives every sample a ray
        if other.camera == sr.PINHOLE:
            assert all(ic.masks(other, kind)[1].sum() == 0 for kind in ic.kinds(other.name))


@pytest.mark.parametrize("name", list(ic.CASES))
def test_compose_plane_is_first_hits_rule_with_all_three_orders(name):
    """on the float64 maps of a frame's candidates rc.compose_plane places every sample where infill_reference.first_hits
    does, in every plane's camera; the luma picture is infill_reference.compose's"""
    c = ic.case(name)
    L, g, times, targets = ic.lens(c), wc.gyro(c.motion), wc.frame_times(), ic.targets64(c)
    frames = wc.noise(ic.N_FRAMES, rc.ROWS, rc.COLS)
    for kind in ic.kinds(name):
        rows, cols = ic.source_size(kind)
        maps = {(f, k): ic.reference_map(c, kind, f, k, targets) for f, k in ic.pairs()}
        for f in range(ic.N_FRAMES):
            cand = ir.candidates(f, ic.N_FRAMES, ic.RADIUS)
            got, place = rc.compose_plane([frames[k][:rows, :cols] for k in cand], [maps[(f, k)] for k in cand], rows, cols, 77,
                                          lambda fr, m: sr.sample(fr, m)[0])
            np.testing.assert_array_equal(place, ic.hits(name, kind, f), err_msg="%s frame %d" % (kind, f))
            assert place.shape == ic.out_shape(c, kind)
            if kind == ic.LUMA:
                want_place, pos, _ = ir.first_hits(g, L, rc.ROWS, rc.COLS, times, synth.D_TRUE, targets, ic.RADIUS, f, zoom=c.zoom, camera=c.camera,
                                                   out_size=c.out_size)
                np.testing.assert_array_equal(got, ir.compose(frames, want_place, pos, cand, 77))


@pytest.mark.parametrize("name", list(ic.CASES))
def test_every_donor_map_compares_at_least_a_quarter_of_its_samples(name):
    """section a of the device tests holds the compared samples of every (f, g) to float64: the reference alone must give it
    enough of them, with a tolerance that is a rounding's size and not a sample's"""
    c = ic.case(name)
    targets = ic.targets64(c)
    for kind in ic.kinds(name):
        for f, g in ic.pairs():
            m = ic.map_case(c, kind, f, g, targets)
            share = m["compared"].sum() / m["compared"].size
            print("%s %s f %d g %d: %d of %d compared (%.2f), tolerance %.3g px" % (name, kind, f, g, m["compared"].sum(), m["compared"].size, share, m["tol"]))
            assert share >= ic.MIN_COMPARED_SHARE, (kind, f, g)
            # compared positions lie within 1.5 images of the origin, below 256 px, where a float32 rounding is 1.5e-5 px: a
            # tolerance of a hundredth of a sample would be several hundred roundings and hold the map to nothing fine
            assert 0 < m["tol"] < 1e-2, (kind, f, g)
            assert m["m64"].shape[:2] == ic.out_shape(c, kind)


def test_every_format_has_planes_fills_and_cameras_that_fit():
    for name in ic.FORMATS:
        src, fills = ic.frames(name), ic.fills(name)
        assert len(set(fills)) == len(fills)                      # distinct fills per plane
        for k, a in enumerate(src):
            assert a.shape[:3] == (ic.N_FRAMES,) + ic.source_size(ic.kind_of(name, k)), (name, k)
            stored = ic.stored_fill(name, k)
            assert stored.shape == a.shape[3:], (name, k)
            if ic.shift(name):
                assert (a & 63).max() == 0 and (stored & 63).max() == 0 and a.max() >= 1000 << 6
    assert set(ic.YUV_FORMATS) | set(ic.COLOR_FORMATS) == set(ic.FORMATS)
