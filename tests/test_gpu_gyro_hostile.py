"""The gyro front end on the device, on what a real log does and synth.make_gyro does not: a camera that stands still,
a saturated or spinning sensor, repeated timestamps, dropouts, bursts, a time base days from 0, and the lengths at which
the scan's chunks and segments change shape.  The streams are tests/gyro_cases.py's; tests/test_gyro_cases_cpu.py proves
on the CPU that each reaches the branch named here and that the fp64 oracle alone stays inside the bounds used here.

    test                                   compared with                                  kernel / branch reached
    a  rates_route_against_long_double     gyro_hostile_reference (long double): info     gyro_rates_kernel (gyro_delta's else-branch
                                           equal, knots within SCAN_ATOL + 1e-15;         in still / deadband / tiny / repeats),
                                           table == thomas_table(own knots), bit for bit  gyro_scan_kernel, gyro_resample_kernel
                                                                                          (slerp: lerp on dot >= 1 and NaN, sign flip
                                                                                          in `flip`), both spline kernels
    b  still_is_exactly_the_identity       [1, 0, 0, 0] and zeros, exactly                the same, with nothing to round
       spline_table_beside_a_still_...     thomas_table, bit for bit                      both spline kernels: the long warm-up of
                                                                                          a run that meets values below 1e-14
    c  scan_edges                          as (a), and the oracle pair within SCAN_ATOL   gyro_scan_kernel: chunk = ceil(n / 1024) at
                                                                                          1024 k +- 1, idle threads, 1 / 2 / 3 / 4
                                                                                          segments, a last segment of ONE sample;
                                                                                          the totals' scan; gyro_scan_fixup_kernel
    d  timestamped_route_...               the oracle: info equal, knots within 2e-15;    gyro_order_kernel (equal is in order),
                                           the long-double slerp within SCAN_ATOL         gyro_resample_kernel: equal neighbours,
                                                                                          q then -q, dot < 0 on every pair
    e  conditioning_...                    check_conditioned of test_gpu_gyro_            gyro_cond_check_kernel, gyro_grid_kernel
                                           conditioning.py (grid equal, rates bit-equal   (interp_rate on duplicates, across gaps, on
                                           or within CHUNKED_R x e_seq, knots)            a sample), gyro_lowpass_kernel + carry,
                                                                                          gyro_decimate_kernel, gyro_rates_uniform_kernel
    f  a_shifted_time_base_gives_...       the same scene 65 536 s earlier                the whole chain into PreSync and Sync
    g  complaints_...                      the wording                                    rs::grid_of's time-base refusal, on both
                                                                                          routes, before any launch

Measured on an MI355X, largest knot error against the long-double reference over time bases and orientations, device / the
fp64 oracle alone: still 0 / 0, deadband 5.0e-16 / 5.0e-15, tiny 4.9e-16 / 8.5e-16, saturated 4.5e-15 / 5.9e-15, spin
8.5e-15 / 1.1e-14, flip 2.5e-14 / 2.3e-14, repeats 5.2e-16 / 3.8e-15, dropouts 7.1e-16 / 1.0e-14, bursts 4.3e-16 / 4.2e-15;
saturated at the edge lengths 2.6e-14 / 2.8e-14 (98 305 samples).  Every test here runs in under a second.

SCAN_ATOL (2e-13, tests/test_gpu_gyro.py:107) bounds the scan's rounding over up to 1e5 products; 1e-15 is that file's bound
for slerp on the device's math library against the host's.  Neither is changed here."""
import numpy as np
import pytest

import rssync_amd
from rssync_amd import synth
from oracle import oracle

import gyro_cases as cases
import gyro_hostile_reference as hostile
import gyro_signal_reference as ref
from test_gpu_gyro import thomas_table
from test_gpu_gyro_conditioning import check_conditioned, SCAN_ATOL

pytestmark = pytest.mark.gpu

SLERP_ATOL = 1e-15       # tests/test_gpu_gyro.py:89
LD = np.longdouble
TIME_BASE = "time base"


def check_rates_route(run, with_oracle=False):
    """-> the device's largest knot error against the long-double reference"""
    name, n, t0, orientation = run
    info, knots, q, us = hostile.case_route(*run)
    t, r = cases.make(name, n, t0)
    h = rssync_amd.SyncProblem(verbose=False)
    h.set_gyro_rates(t, r, orientation)
    assert h.gyro_info() == info, cases.run_id(run)
    got = h.gyro_knots()
    err = float(np.max(np.abs(got - knots)))
    line = "%s: device knot error %.3g" % (cases.run_id(run), err)
    if with_oracle:
        oq, ous = oracle.integrate_gyro(t, r, orientation)
        assert np.array_equal(ous, us)
        assert hostile.last_grid_sample(ous, info[0]) < 2 ** 31      # the oracle's grid loop counts in `int`
        o = oracle.OracleProblem()
        o.SetGyroQuaternionsTimestamped(ous, oq)
        assert h.gyro_info() == o.gyro_info()
        ok = o.gyro_knots()
        line += ", oracle's own %.3g, device against oracle %.3g" % (float(np.max(np.abs(ok - knots))), float(np.max(np.abs(got - ok))))
    print(line)
    assert err <= SCAN_ATOL + SLERP_ATOL, cases.run_id(run)
    if with_oracle:
        np.testing.assert_allclose(got, ok, rtol=0, atol=SCAN_ATOL)
    assert np.array_equal(h.gyro_table(), thomas_table(got)), cases.run_id(run)
    return h, got


# ---- a, b: every case, every time base -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_rates_route_against_long_double(name):
    for run in cases.runs():
        if run[0] == name and run[1] == cases.N_DEFAULT:
            check_rates_route(run)


def test_still_is_exactly_the_identity():
    for t0 in cases.T0S:
        for orientation in cases.ORIENTATIONS:
            t, r = cases.make("still", cases.N_DEFAULT, t0)
            h = rssync_amd.SyncProblem(verbose=False)
            h.set_gyro_rates(t, r, orientation)                     # no complaint
            knots, table = h.gyro_knots(), h.gyro_table()
            assert np.array_equal(knots, np.tile([1.0, 0.0, 0.0, 0.0], (knots.shape[0], 1)))
            assert np.array_equal(table[:, 0], knots) and not table[:, 1:].any()


def test_spline_table_beside_a_still_stretch_is_the_sequential_solve():
    """Equal knots give right-hand sides of exactly 0; there the sequential solve is the decaying tail of the motion beside
    the stretch, 0.268 per row down through 1e-40 and the subnormals to 0, and a run's warm-up start is all there is to
    see of it.  Found by `deadband` above (first 2 s at rest: 491 rows of c differed by up to 5e-43 from the sequential
    solve with the 64-row warm-up alone).  Stretches shorter and longer than both warm-ups, at either end and inside."""
    rng = np.random.default_rng(8)
    for n, stretches in [(700, [(0, 300)]), (700, [(400, 700)]), (1500, [(200, 1300)]), (4099, [(0, 1000), (1700, 3300), (3500, 4099)]),
                         (1300, [(0, 650), (652, 1300)]), (2000, [(100, 164), (300, 940), (1000, 1609)])]:
        q = rng.standard_normal((n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        for lo, hi in stretches:
            q[lo:hi] = q[lo]
        h = rssync_amd.SyncProblem(verbose=False)
        h.SetGyroQuaternions(q, 400.0, 0.0)
        got, want = h.gyro_table(), thomas_table(q)
        tiny = np.abs(want[:, 2]) < 1e-30
        assert tiny.any() and (want[:, 2][tiny] != 0).any()          # the tail is there to be got wrong
        assert np.array_equal(got, want), (n, stretches, int(np.count_nonzero(got != want)), float(np.max(np.abs(got - want))))


# ---- c: the scan's edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.EDGES)
def test_scan_edges(n):
    (run,) = [r for r in cases.runs() if r[0] == "saturated" and r[1] == n]
    check_rates_route(run, with_oracle=True)


# ---- d: the timestamped route ------------------------------------------------------------------------------------------
def timestamped_inputs():
    """-> [(label, ts_us, quats)]: identical neighbours, q followed by -q, and `flip`'s orientations, on the timestamps of
    `repeats` (every 7th equal to the one before it) and of `bursts`"""
    out = []
    rng = np.random.default_rng(41)
    for stamps in ("repeats", "bursts"):
        for t0 in (0, 200000):
            t, _ = cases.make(stamps, cases.N_DEFAULT, t0)
            us = cases.timestamps_us(t)
            n = us.size
            q = rng.standard_normal((n, 4))
            q /= np.linalg.norm(q, axis=1, keepdims=True)
            same = q.copy()
            same[1::2] = same[0::2][:same[1::2].shape[0]]           # pairs of identical neighbours (dot = |q|^2: 1 -+ 1 ulp)
            out.append(("identical-%s-t%d" % (stamps, t0), us, same))
            anti = same.copy()
            anti[1::2] = -anti[1::2]                                # q, -q: dot = -|q|^2, flipped to the case above
            out.append(("negated-%s-t%d" % (stamps, t0), us, anti))
            fq = hostile.case_route("flip", cases.N_DEFAULT, 0, None)[2].astype(np.float64)
            out.append(("flip-%s-t%d" % (stamps, t0), us, fq))
    return out


def test_timestamped_route_on_equal_negated_and_flipping_neighbours():
    for label, us, q in timestamped_inputs():
        info, want = hostile.knots_of(us, q)
        assert hostile.last_grid_sample(us, info[0]) < 2 ** 31      # the oracle's grid loop counts in `int`
        h, o = rssync_amd.SyncProblem(verbose=False), oracle.OracleProblem()
        h.SetGyroQuaternionsTimestamped(us, q)
        o.SetGyroQuaternionsTimestamped(us, q)
        assert h.gyro_info() == o.gyro_info() == info, label
        got, ok = h.gyro_knots(), o.gyro_knots()
        print("%s: device against oracle %.3g, against long double %.3g" %
              (label, float(np.max(np.abs(got - ok))), float(np.max(np.abs(got - want)))))
        np.testing.assert_allclose(got, ok, rtol=0, atol=2e-15, err_msg=label)
        assert float(np.max(np.abs(got - want))) <= SCAN_ATOL, label
        assert np.array_equal(h.gyro_table(), thomas_table(got)), label


# ---- e: conditioning ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deadband", "saturated", "repeats", "dropouts", "bursts"])
def test_conditioning_on_the_hostile_streams(name):
    t, r = cases.make(name)
    check_conditioned(("hostile", name), t, r, knots_too=True)


def test_conditioning_of_a_saturated_stream_over_more_than_one_segment():
    t, r = cases.make("saturated", 70001)
    check_conditioned(("hostile", "saturated", 70001), t, r, knots_too=False)


def test_conditioning_of_a_camera_that_stands_still():
    t, r = cases.make("still")
    for divider, k in [(d, k) for d in (0, 3, 32, 256) for k in (1, 2, 8) if k == 1 or d >= 2 * k]:
        h = rssync_amd.SyncProblem(verbose=False)
        h.set_gyro_conditioning(divider, k)
        h.set_gyro_rates(t, r)
        got, fs, t0 = h.gyro_conditioned()
        assert got.shape[0] >= 5003 // k - 2 and not got.any(), (divider, k)
        knots = h.gyro_knots()
        assert np.array_equal(knots, np.tile([1.0, 0.0, 0.0, 0.0], (knots.shape[0], 1))), (divider, k)


@pytest.mark.parametrize("divider", [3, 32, 256])
def test_conditioning_hands_a_constant_stream_through(divider):
    """rates (0.3, -0.2, 0.1) throughout: away from the ends (4 x divider samples, the filter's start from its input) the
    output is the long-double filter's to CHUNKED_R x e_seq"""
    t, r = cases.constant()
    sr, t_new, grid = ref.gyro_interpolate(t, r)
    truth = ref.gyro_lowpass(grid, divider, LD, coef=ref.lowpass_coef(divider))
    e_seq = float(np.max(np.abs(ref.gyro_lowpass(grid, divider) - truth)))
    h = rssync_amd.SyncProblem(verbose=False)
    h.set_gyro_conditioning(divider, 1)
    h.set_gyro_rates(t, r)
    got, fs, t0 = h.gyro_conditioned()
    assert got.shape == grid.shape and fs == sr
    cut = 4 * divider
    err = float(np.max(np.abs(got[cut:-cut] - truth[cut:-cut])))
    print("constant stream, divider %d: e_seq %.3g, device error %.3g away from the ends" % (divider, e_seq, err))
    assert e_seq > 0 and err <= ref.CHUNKED_R * e_seq


# ---- f: one end to end --------------------------------------------------------------------------------------------------
def test_a_shifted_time_base_gives_the_same_delay():
    """tests/test_gpu_gyro.py's scene (rates -> device -> PreSync / Sync) with 65 536 s added to the gyro's and the frames'
    times, against the unshifted run: the same PreSync grid value, the Sync delays within that test's 1e-8.  The gyro's
    times sit half a microsecond above a whole one: (int64)(t * 1e6) of a time that IS a whole microsecond lands on
    either side of it in fp64, differently at the two time bases, and a sample moved by 1 us is a knot moved by 2e-6 rad."""
    F, N, shift = 32, 128, 65536.0
    g = synth.make_gyro(1.0, 1.0 + (F + 2) / synth.FPS, seed=77)
    times = (np.round(g.times * 1e6) + 0.5) / 1e6
    assert np.array_equal(cases.timestamps_us(times) + 65536000000, cases.timestamps_us(times + shift))
    a, b = rssync_amd.SyncProblem(seed=5, verbose=False), rssync_amd.SyncProblem(seed=5, verbose=False)
    a.set_gyro_rates(times, g.rates)
    b.set_gyro_rates(times + shift, g.rates)
    assert b.gyro_info() == (a.gyro_info()[0], a.gyro_info()[1] + shift, a.gyro_info()[2])
    print("knots differ by %.3g between the time bases" % float(np.max(np.abs(a.gyro_knots() - b.gyro_knots()))))
    for fr, ta, tb, ra, rb in synth.make_frames(g, 30, 30 + F, N, seed=9, noise=0.0, outliers=0.0):
        a.SetTrackResult(fr, ta, tb, ra, rb)
        b.SetTrackResult(fr, ta + shift, tb + shift, ra, rb)
    ca, da = a.PreSync(0.0, 30, 30 + F, 0.001, 0.05)
    cb, db = b.PreSync(0.0, 30, 30 + F, 0.001, 0.05)
    sa, sb = a.Sync(da, 30, 30 + F, 0.0, 0.1), b.Sync(db, 30, 30 + F, 0.0, 0.1)
    print("PreSync delay %r / %r (cost %.6g / %.6g); Sync delay %.10f at 0 s, %.10f at %d s" % (da, db, ca, cb, sa[1], sb[1], shift))
    assert da == db
    assert abs(sa[1] - sb[1]) < 1e-8


# ---- g: complaints ------------------------------------------------------------------------------------------------------
def test_complaints_name_the_time_base_and_leave_the_object_usable():
    n = 4000
    rng = np.random.default_rng(4)
    r = 0.3 * rng.standard_normal((n, 3))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rel = np.arange(n) / 8000.0
    h = rssync_amd.SyncProblem(verbose=False)
    # a repeated timestamp is accepted, not reported as out of order
    us = (np.arange(n) * 125).astype(np.int64)
    us[7::9] = us[6::9][:us[7::9].size]
    h.SetGyroQuaternionsTimestamped(us, q)
    assert h.gyro_info()[0] == 8000.0
    t_rep = 1.0 + rel
    t_rep[7::9] = t_rep[6::9][:t_rep[7::9].size]
    h.set_gyro_rates(t_rep, r)
    assert h.gyro_info()[:2] == (8000.0, 1.0)
    # 8 kHz: the first grid sample passes 2^31 at 268 435.456 s; 2^50 us = 1.126e9 s
    h.set_gyro_rates(268435.0 + rel, r)
    assert h.gyro_info()[:2] == (8000.0, 268435.0)
    for t0 in (268436.0, 3.0e5, 6.0e5, 1.2e9):
        with pytest.raises(rssync_amd.RsSyncError, match=TIME_BASE):
            h.set_gyro_rates(t0 + rel, r)
        with pytest.raises(rssync_amd.RsSyncError, match="gyro data was not set"):
            h.gyro_table()
        with pytest.raises(rssync_amd.RsSyncError, match=TIME_BASE):
            h.SetGyroQuaternionsTimestamped(((t0 + rel) * 1e6).astype(np.int64), q)
    with pytest.raises(rssync_amd.RsSyncError, match=TIME_BASE):     # first x rate leaves int64 here; the division does not
        h.SetGyroQuaternionsTimestamped((1 << 50) - 400 + np.arange(6) * 62, q[:6])
    h.set_gyro_rates(1.0 + rel, r)                                   # and the object is usable afterwards
    assert h.gyro_info()[:2] == (8000.0, 1.0)
    h.SetGyroQuaternionsTimestamped((np.arange(n) * 125).astype(np.int64), q)
    assert h.gyro_info()[:2] == (8000.0, 0.0)
