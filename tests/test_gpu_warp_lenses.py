"""The rectifier and the stabiliser on the device across lenses, motions, frame sizes and reuses of the ray-map cache
(tests/warp_cases.py; the conditions these comparisons rest on are proved in tests/test_warp_cases_cpu.py).

  a  map against the float64 reference, every lens x motion at 95 x 169, rectifier and stabiliser (lens camera)
  b  a camera at rest is the identity, every lens
  c  points against the reference at 1520 x 2704, and as the inverse of the map
  d  pixels and points the lens cannot image: NaN position, `fill`, counted
  e  sampler and counts from the device's own map at the edge sizes and under roll, three frames per call
  f  one problem through a sequence of calls that reuse or must refresh the cached ray map, against fresh problems
"""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import rectify_reference as rr
import stabilize_reference as sr
import warp_cases as wc

pytestmark = pytest.mark.gpu


def _problem(gyro):
    import rssync_amd
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    return p


@pytest.fixture(scope="module")
def problems(built):
    """one problem per motion"""
    return {m: _problem(wc.gyro(m)) for m in wc.MOTIONS}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_map(what, got, c, rows=wc.ROWS, cols=wc.COLS):
    """section a for one map: compared pixels within the case's tolerance, the other in-range pixels outside on both
    sides, out-of-range pixels NaN -> the device's distance"""
    assert got.shape == c["m64"].shape and got.dtype == np.float32
    cmp_, inr, outr = c["compared"], c["in_range"], c["out_of_range"]
    assert np.isfinite(got[inr]).all()
    worst = float(np.abs(got.astype(np.float64) - c["m64"])[cmp_].max())
    print("%s: %.3g px (tolerance %.3g, %d compared of %d in range, %d out of range)" % (what, worst, c["tol"], cmp_.sum(), inr.sum(),
                                                                                        outr.sum()))
    assert worst <= c["tol"], what
    far = inr & ~cmp_
    assert not sr.inside(got, rows, cols)[far].any() and not sr.inside(c["m64"], rows, cols)[far].any(), what
    assert np.isnan(got[outr]).all(), what
    return worst


# a -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,motion,extra_delay,ref_row", wc.rect_cases())
def test_a_rectifier_map_against_the_float64_reference(problems, name, motion, extra_delay, ref_row):
    c = wc.rect_case(name, motion, extra_delay, ref_row)
    got = problems[motion].rectify_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"], ref_row=ref_row)
    _check_map("%s %s delay +%.2f ref_row %s" % (name, motion, extra_delay, ref_row), got, c)


@pytest.mark.parametrize("name,motion", wc.stab_cases())
def test_a_stabiliser_map_with_the_lens_camera_against_the_float64_reference(problems, name, motion):
    c = wc.stab_case(name, motion)
    got = problems[motion].stabilize_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"], sigma=wc.STAB_SIGMA, zoom=wc.STAB_ZOOM,
                                         camera=sr.LENS)
    _check_map("stabiliser %s %s" % (name, motion), got, c)


# b -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.LENSES)
def test_b_a_camera_at_rest_is_the_identity(problems, name):
    c = wc.rect_case(name, "rest")
    p, inr = problems["rest"], c["in_range"]
    got = p.rectify_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"])
    worst = float(np.abs(got.astype(np.float64) - wc.grid(wc.ROWS, wc.COLS))[inr].max())
    print("%s at rest: %.3g px from the identity (tolerance %.3g)" % (name, worst, c["tol"]))
    assert worst <= c["tol"]
    frames = wc.noise(2, wc.ROWS, wc.COLS)
    out, _ = p.rectify_frames(frames, wc.frame_times()[:2], c["lens"], c["delay"])
    sel = inr[1:-1, 1:-1]
    assert sel.sum() > 0.2 * inr.size
    for k in range(2):
        np.testing.assert_array_equal(out[k][1:-1, 1:-1][sel], frames[k][1:-1, 1:-1][sel])


# c -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.LENSES)
def test_c_points_against_the_reference_at_full_size(problems, name):
    L, pts = wc.full_size_points(name)
    for motion in ("x1", "x20"):
        for ref_row in (None, 0):
            got = problems[motion].rectify_points(pts, wc.FULL_COLS, wc.FULL_ROWS, L, wc.frame_time(), wc.delays()[0], ref_row=ref_row)
            want = rr.forward_points(wc.gyro(motion), L, wc.FULL_ROWS, wc.frame_time(), wc.delays()[0], pts, ref_row=ref_row)
            worst = float(np.abs(got - want).max())
            print("%s %s ref_row %s: %d points against the reference %.3g px" % (name, motion, ref_row, len(pts), worst))
            assert worst <= 1e-9, (name, motion, ref_row)


@pytest.mark.parametrize("name", wc.LENSES)
def test_c_points_are_the_inverse_of_the_map(problems, name):
    """under the scene's motion and at rest: three iterations have converged there (at 2 rad/s the third moves the map by
    2e-5 px; under x20 they have not, and the closed-form points are no inverse of that map)"""
    for motion in ("x1", "rest"):
        c = wc.rect_case(name, motion)
        p = problems[motion]
        m = p.rectify_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"])
        back = p.rectify_points(m.astype(np.float64), wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"])
        # Sources inside the frame: beyond its first and last row the map holds the table's end entries where the points
        # take the orientation of their own row time.  A source position is itself a position of the frame, and only those
        # the lens can image come back (taken from the reference's map: the margin of the range is far wider than the
        # tolerance).
        ok = c["in_range"] & rr.inside(m) & wc.range_masks(c["lens"], c["m64"])[0]
        assert ok.sum() >= 0.9 * c["compared"].sum()
        worst = float(np.abs(back - wc.grid(wc.ROWS, wc.COLS))[ok].max())
        print("%s %s: points o map %.3g px (tolerance %.3g, %d of %d compared)" % (name, motion, worst, c["tol"], ok.sum(),
                                                                                  c["compared"].sum()))
        assert worst <= c["tol"], (name, motion)


# d -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.UNIMAGEABLE)
def test_d_pixels_the_lens_cannot_image_are_filled_counted_and_nan(problems, name):
    for motion in ("x1", "rest"):
        c = wc.rect_case(name, motion)
        p, outr, inr = problems[motion], c["out_of_range"], c["in_range"]
        assert outr.sum() >= 24
        m = p.rectify_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"])
        assert np.isnan(m[outr]).all() and np.isfinite(m[inr]).all()
        frames = np.full((3, wc.ROWS, wc.COLS), 200, np.uint8)
        out, n_out = p.rectify_frames(frames, np.repeat(c["time"], 3), c["lens"], c["delay"], fill=wc.FILL)
        want, want_n = rr.sample(frames[0], m, fill=wc.FILL)
        for k in range(3):
            assert (out[k][outr] == wc.FILL).all()
            np.testing.assert_array_equal(out[k], want)
            assert int(n_out[k]) == want_n >= outr.sum()
        assert (out[0][inr & rr.inside(m)] == 200).all()
        sm = p.stabilize_map(wc.COLS, wc.ROWS, c["lens"], c["time"], c["delay"], sigma=wc.STAB_SIGMA, zoom=1.0, camera=sr.LENS)
        assert np.isnan(sm[outr]).all() and np.isfinite(sm[inr]).all()
        sout, sn = p.stabilize_frames(frames[:1], [c["time"]], c["lens"], c["delay"], sigma=wc.STAB_SIGMA, zoom=1.0, camera=sr.LENS,
                                      fill=wc.FILL)
        assert (sout[0][outr] == wc.FILL).all() and int(sn[0]) == int((~sr.inside(sm, wc.ROWS, wc.COLS)).sum()) >= outr.sum()
    L, pts = wc.out_of_range_points(name)
    _, good = wc.full_size_points(name)
    both = np.concatenate([pts, good[:16]])
    got = problems["x1"].rectify_points(both, wc.FULL_COLS, wc.FULL_ROWS, L, wc.frame_time(), wc.delays()[0])
    assert np.isnan(got[:len(pts)]).all() and np.isfinite(got[len(pts):]).all()


@pytest.mark.parametrize("name", wc.UNIMAGEABLE)
def test_d_the_coverage_sweep_counts_unimageable_border_pixels_at_every_zoom(problems, name):
    """at rest, without smoothing, an in-range border pixel of the output looks at (c + (u - c) / zoom): inside the frame
    for every zoom above 1, so the count is that of the border pixels the zoomed camera cannot image -- those within the
    margin of its range may fall either way"""
    L, zooms = wc.lens(name), (1.02, 1.1, 1.3, 2.0)
    counts = problems["rest"].stabilize_coverage(wc.COLS, wc.ROWS, L, wc.frame_times(), wc.delays()[0], zooms, sigma=0.0, camera=sr.LENS)
    assert counts.shape == (3, len(zooms))
    border = sr.border(wc.ROWS, wc.COLS)
    seen = 0
    for z, zoom in enumerate(zooms):
        inr, outr = wc.range_masks(wc.stab_camera_lens(L, wc.ROWS, wc.COLS, zoom), border)
        lo, hi = int(outr.sum()), int((~inr).sum())
        print("%s zoom %.2f: %s border pixels outside, %d .. %d cannot be imaged" % (name, zoom, counts[:, z].tolist(), lo, hi))
        assert ((counts[:, z] >= lo) & (counts[:, z] <= hi)).all(), (name, zoom)
        seen += lo
    assert seen > 0


# e -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,motion,rows,cols", wc.sampler_cases())
def test_e_sampler_and_counts_from_the_devices_own_map(problems, name, motion, rows, cols):
    """three frames with three times per call, pitched input and output, padding untouched; then the same through the
    launcher with a budget of one and a half frames per slot (three chunks through both slots)"""
    from rssync_amd import rectify, synth
    p, L, times = problems[motion], wc.lens(name, rows, cols), wc.frame_times()
    frames = wc.noise(3, rows, cols)
    maps = [p.rectify_map(cols, rows, L, t, synth.D_TRUE) for t in times]
    want = [rr.sample(frames[k], maps[k], fill=wc.FILL) for k in range(3)]
    src = np.zeros((3, rows + 2, cols + 45), np.uint8)
    src[:, 1:1 + rows, 7:7 + cols] = frames
    dst = np.full((3, rows + 3, cols + 21), 201, np.uint8)
    view = dst[:, 1:1 + rows, 5:5 + cols]
    got, got_n = p.rectify_frames(src[:, 1:1 + rows, 7:7 + cols], times, L, synth.D_TRUE, fill=wc.FILL, out=view)
    assert got is view
    print("%s %s %d x %d: filled %s of %d" % (name, motion, rows, cols, [int(n) for n in got_n], rows * cols))
    for k in range(3):
        np.testing.assert_array_equal(view[k], want[k][0], err_msg="frame %d" % k)
        assert int(got_n[k]) == want[k][1], (k, got_n, [w[1] for w in want])
        assert 0 < want[k][1] < rows * cols
    if motion == "roll":
        assert len(set(int(n) for n in got_n)) == 3
    pad = np.ones(dst.shape, bool)
    pad[:, 1:1 + rows, 5:5 + cols] = False
    assert (dst[pad] == 201).all()
    out, out_n = rectify.rectify_frames_budget(p, frames, times, L, synth.D_TRUE, wc.budget_bytes(rows, cols), fill=wc.FILL)
    for k in range(3):
        np.testing.assert_array_equal(out[k], want[k][0], err_msg="budget, frame %d" % k)
        assert int(out_n[k]) == want[k][1]


# f -----------------------------------------------------------------------------------------------------------------------
def test_f_the_ray_map_cache_through_a_sequence_of_calls(built):
    """after every step the long-lived problem gives the bits of a freshly constructed one (at most two contexts alive)"""
    from rssync_amd import synth
    A, B, C = wc.cache_lenses()
    r, c, t, d = wc.CACHE_ROWS, wc.CACHE_COLS, wc.frame_time(), synth.D_TRUE
    frame = wc.noise(1, r, c)
    frame_t = wc.noise(1, c, r)
    g1, g20 = wc.gyro("x1"), wc.gyro("x20")

    def rect(L, rows=r, cols=c, f=frame):
        def run(p):
            m = p.rectify_map(cols, rows, L, t, d)
            out, n = p.rectify_frames(f, [t], L, d, fill=wc.FILL)
            return m, out, n
        return run

    def stab(**kw):
        def run(p):
            m = p.stabilize_map(c, r, A, t, d, sigma=wc.STAB_SIGMA, **kw)
            out, n = p.stabilize_frames(frame, [t], A, d, sigma=wc.STAB_SIGMA, fill=wc.FILL, **kw)
            return m, out, n
        return run

    p = _problem(g1)
    seen = {}

    def step(k, run, gyro=g1):
        got = run(p)
        fresh = _problem(gyro)
        want = run(fresh)
        fresh.close()
        np.testing.assert_array_equal(_u32(got[0]), _u32(want[0]), err_msg="step %d: map" % k)
        np.testing.assert_array_equal(got[1], want[1], err_msg="step %d: frame" % k)
        np.testing.assert_array_equal(got[2], want[2], err_msg="step %d: count" % k)
        seen[k] = got
        return got

    def against_reference(k, got, L, gyro):
        m64, m32 = rr.map64(gyro, L, r, c, t, d), rr.map32(gyro, L, r, c, t, d)
        tol = wc.tolerance(m32, m64, np.ones((r, c), bool))
        worst = float(np.abs(got[0].astype(np.float64) - m64).max())
        print("step %d against the reference: %.3g px (tolerance %.3g)" % (k, worst, tol))
        assert worst <= tol, k

    step(1, rect(A))
    step(2, rect(B))
    assert (_u32(seen[2][0]) != _u32(seen[1][0])).any()
    step(3, rect(A))
    np.testing.assert_array_equal(_u32(seen[3][0]), _u32(seen[1][0]))
    against_reference(4, step(4, rect(C)), C, g1)           # the cache hits; the row table is the call's own
    assert (_u32(seen[4][0]) != _u32(seen[1][0])).any()
    step(5, rect(A, c, r, frame_t))                         # the same nine numbers, 29 x 37: equal area
    step(6, stab(zoom=wc.STAB_ZOOM, camera=sr.LENS))
    step(7, rect(A))
    np.testing.assert_array_equal(_u32(seen[7][0]), _u32(seen[1][0]))
    step(8, stab(zoom=wc.STAB_ZOOM, camera=sr.PINHOLE))
    step(9, rect(A))
    np.testing.assert_array_equal(_u32(seen[9][0]), _u32(seen[1][0]))
    p.SetGyroQuaternions(g20.quats, g20.fs, g20.t0)         # step 10
    against_reference(11, step(11, rect(A), g20), A, g20)
    assert (_u32(seen[11][0]) != _u32(seen[1][0])).any()
    # ... and the lens camera at another zoom BETWEEN two calls with one key: the map it left is not A's
    step(12, stab(zoom=1.3, camera=sr.LENS), g20)
    step(13, rect(A), g20)
    np.testing.assert_array_equal(_u32(seen[13][0]), _u32(seen[11][0]))
    step(14, stab(zoom=1.3, camera=sr.LENS), g20)
    np.testing.assert_array_equal(_u32(seen[14][0]), _u32(seen[12][0]))
    p.close()
