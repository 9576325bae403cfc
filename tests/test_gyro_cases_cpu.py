"""The streams of tests/gyro_cases.py, proved on the CPU before the device sees them (tests/test_gpu_gyro_hostile.py):

    the long-double reference (tests/gyro_hostile_reference.py) against a closed form in mpmath, to 1e-17;
    the fp64 oracle pair (integrate_gyro, then SetGyroQuaternionsTimestamped) within the device tests' bound of that
        reference on every run the device tests make -- so a device failure there is the device's;
    no slerp sign decision is close (|dot| > 1e-3 on every consecutive pair): fp64 and long double cannot flip differently;
    the screens: each stream reaches the branch it is there for, in fp64;
    the host stand-in (tests/cpu_device/rship_cpu.cpp, which shares gyro_math.hpp with the kernels) within the same bound,
        and its complaint about a time base past the integer grid;
    interp_rate (gyro_signal_math.hpp) on duplicated timestamps, across gaps and on grid points that sit on a sample.

WHAT BITES (tried on the CPU stand-in, each edit on its own):
    gyro_delta without its th2 > 0 guard          test_host_stand_in_stays_within_the_scan_bound[still-...] (and deadband,
                                                  tiny, repeats): 0 / 0, "non-finite sample after interpolation"
    quat_slerp without the lerp for a NaN theta   test_host_stand_in_stays_within_the_scan_bound[tiny-...] (all 8; and 7
                                                  of deadband's 8): the pairs that
                                                  test_screens_tiny_has_pairs_whose_dot_exceeds_one counts
    interp_rate taking the last of equal stamps   test_interpolation_on_the_hostile_streams_is_bit_equal[repeats] and
                                                  test_interpolation_takes_the_first_of_two_equal_timestamps
    quat_slerp without the sign flip              test_host_stand_in_stays_within_the_scan_bound[flip-...]"""
import mpmath
import numpy as np
import pytest

import gyro_cases as cases
import gyro_hostile_reference as hostile
import gyro_signal_reference as ref
from test_gyro_conditioning_cpu import shim, shim_grid, _pd   # noqa: F401  (shim: a fixture)

SCAN_ATOL = 2e-13        # tests/test_gpu_gyro.py:107, the bound of the device tests; not to be touched here
RUNS = cases.runs()
LD = np.longdouble


def dot64(p, q):
    """the four products summed from the left in fp64, as rs::quat_slerp sums them"""
    return ((p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]) + p[:, 3] * q[:, 3]


def th2_64(t, rates):
    """-> (th2 in fp64 as rs::gyro_delta computes it, w) for samples 1 .. n-1"""
    w = rates[1:] * np.diff(t)[:, None]
    return (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2], w


_oracle = {}


def oracle_pair(run):
    """the fp64 oracle, one sample after the other -> (info, knots, orientations)"""
    from oracle import oracle
    if run not in _oracle:
        name, n, t0, orientation = run
        t, r = cases.make(name, n, t0)
        q, us = oracle.integrate_gyro(t, r, orientation)
        info = hostile.case_route(*run)[0]
        # the oracle's grid loop counts in `int`, as the reference's does, and does not end past 2^31
        assert hostile.last_grid_sample(us, info[0]) < 2 ** 31
        o = oracle.OracleProblem()
        o.SetGyroQuaternionsTimestamped(us, q)
        _oracle[run] = (o.gyro_info(), o.gyro_knots(), q)
    return _oracle[run]


# ---- the reference against a closed form ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,t0", [("spin", 0), ("spin", 200000), ("flip", 0), ("flip", 65536)])
def test_reference_agrees_with_the_closed_form(name, t0):
    """Rotation about a fixed axis: the orientation at sample i is the rotation by the sum of |w| dt, between two samples
    slerp is that rotation at the linearly interpolated angle -- for `flip` the short way round after the sign change."""
    mpmath.mp.prec = 200
    t, r = cases.make(name, cases.N_DEFAULT, t0)
    info, knots, q, us = hostile.case_route(name, cases.N_DEFAULT, t0, None)
    assert np.all(r == r[0])
    rate = [mpmath.mpf(float(v)) for v in r[0]]
    speed = mpmath.sqrt(sum(v * v for v in rate))
    axis = [v / speed for v in rate]
    half = [mpmath.mpf(0)]                       # half the angle at every sample; dt is the fp64 difference, as the kernel's
    for dt in np.diff(t):
        half.append(half[-1] + speed * mpmath.mpf(float(dt)) / 2)
    sr, first_sample, times = hostile.grid(us)
    us_list = [int(v) for v in us]
    hi = knots.astype(np.float64)                # a long double is the sum of two doubles, exactly
    lo = (knots - hi.astype(LD)).astype(np.float64)
    assert np.array_equal(hi.astype(LD) + lo.astype(LD), knots)
    worst, flips = mpmath.mpf(0), 0
    for j, tg in enumerate(times):
        i = int(np.searchsorted(us, tg, side="left"))
        if i == 0:
            h = half[0]
        else:
            a, b = half[i - 1], half[i]
            turns = mpmath.nint((b - a) / mpmath.pi)          # q and -q are the rotation by b and by b - pi
            flips += int(turns) % 2
            b = b - turns * mpmath.pi
            u = mpmath.mpf(tg - us_list[i - 1]) / mpmath.mpf(us_list[i] - us_list[i - 1])
            h = a + u * (b - a)
        want = [mpmath.cos(h)] + [x * mpmath.sin(h) for x in axis]
        for c in range(4):
            worst = max(worst, abs(want[c] - (mpmath.mpf(float(hi[j, c])) + mpmath.mpf(float(lo[j, c])))))
    print("%s t0 %d: %d knots, %d of them across a sign flip, largest difference to the closed form %.3g" %
          (name, t0, len(times), flips, float(worst)))
    assert (flips > len(times) // 2) == (name == "flip")
    assert worst <= 1e-17


# ---- the oracle alone, and the sign decisions -------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=cases.run_id)
def test_fp64_oracle_stays_inside_the_gpu_bound(built, run):
    info, knots, q, us = hostile.case_route(*run)
    o_info, o_knots, o_q = oracle_pair(run)
    assert o_info == info
    err = float(np.max(np.abs(o_knots - knots)))
    print("%s: oracle knot error %.3g (orientations %.3g)" % (cases.run_id(run), err, float(np.max(np.abs(o_q - q)))))
    assert err <= SCAN_ATOL


@pytest.mark.parametrize("run", RUNS, ids=cases.run_id)
def test_no_slerp_sign_decision_is_close(built, run):
    q = hostile.case_route(*run)[2]
    o_q = oracle_pair(run)[2]
    d = np.sum(q[1:] * q[:-1], axis=1)
    d64 = dot64(o_q[:-1], o_q[1:])
    assert float(np.min(np.abs(d))) > 1e-3 and float(np.min(np.abs(d64))) > 1e-3
    assert np.array_equal(d < 0, d64 < 0)


# ---- the screens: each stream reaches what it is there to reach ---------------------------------------------------------
@pytest.mark.parametrize("name", ["still", "deadband", "tiny", "repeats"])
def test_screens_th2_is_zero_in_fp64(name):
    for t0 in cases.T0S:
        t, r = cases.make(name, cases.N_DEFAULT, t0)
        th2, w = th2_64(t, r)
        zero = th2 == 0
        assert zero.any()
        if name == "tiny":      # the underflow: th2 == 0 while w != 0
            assert (zero & np.any(w != 0, axis=1)).sum() > 100
        if name == "repeats":   # dt == 0
            assert np.array_equal(zero, np.diff(t) == 0) and zero.sum() >= cases.N_DEFAULT // 7 - 1


@pytest.mark.parametrize("name", ["still", "deadband"])
def test_screens_equal_neighbours_have_a_dot_of_one_or_more(built, name):
    for o in cases.ORIENTATIONS:
        o_q = oracle_pair((name, cases.N_DEFAULT, 0, o))[2]
        d = dot64(o_q[:-1], o_q[1:])
        assert (d >= 1).sum() > 100


def pairs_above_one(run):
    """the grid knots of a run that interpolate between two orientations whose fp64 dot is ABOVE 1: acos gives NaN"""
    info, knots, q, us = hostile.case_route(*run)
    o_q = oracle_pair(run)[2]
    sr, first_sample, times = hostile.grid(us)
    idx = np.searchsorted(us, np.array(times, np.int64), side="left")
    idx = idx[idx > 0]
    return int((dot64(o_q[idx - 1], o_q[idx]) > 1).sum())


def test_screens_tiny_has_pairs_whose_dot_exceeds_one(built):
    """a unit quaternion in fp64 has |q|^2 = 1 + 2.2e-16 about as often as not, and `tiny` repeats one in five"""
    for t0 in cases.T0S:
        for o in cases.ORIENTATIONS:
            assert pairs_above_one(("tiny", cases.N_DEFAULT, t0, o)) > 10


def test_screens_flip_has_a_negative_dot_on_every_pair(built):
    for t0 in cases.T0S:
        q = hostile.case_route("flip", cases.N_DEFAULT, t0, None)[2]
        o_q = oracle_pair(("flip", cases.N_DEFAULT, t0, None))[2]
        assert np.all(np.sum(q[1:] * q[:-1], axis=1) < 0) and np.all(dot64(o_q[:-1], o_q[1:]) < 0)


def test_screens_dropouts_round_to_another_rate():
    n, seed = cases.N_DEFAULT, 1000 * cases.NAMES.index("dropouts") + cases.N_DEFAULT % 997
    t, _ = cases.make("dropouts", n)
    t_whole, _ = cases.without_dropouts(n, seed)
    assert not np.array_equal(t, t_whole)
    sr = hostile.grid(hostile.timestamps_us(t))[0]
    sr_whole = hostile.grid(hostile.timestamps_us(t_whole))[0]
    assert (sr, sr_whole) == (350, 400)
    assert ref.uniform_grid(t)[0] == 350 and ref.uniform_grid(t_whole)[0] == 400     # and the conditioning grid's


def test_screens_conditioning_grid_meets_duplicates_gaps_and_samples():
    t, r = cases.make("repeats")
    sr, t_new = ref.uniform_grid(t)
    b = np.minimum(np.searchsorted(t, t_new, side="left"), t.size - 2)
    inside = (b > 0) & (t[b] > t_new)
    dup = inside & (t[b + 1] == t[b])                  # the upper neighbour is the first of two equal timestamps ...
    assert dup.sum() > 100
    assert np.all(np.any(r[b[dup] + 1] != r[b[dup]], axis=1))    # ... which carry different rates
    t, r = cases.make("dropouts")
    sr, t_new = ref.uniform_grid(t)
    b = np.searchsorted(t, t_new, side="left")
    gap = t[np.minimum(b, t.size - 1)] - t[np.maximum(b - 1, 0)]
    assert (gap > 1.9).sum() > 600 and ((gap > 0.4) & (gap < 0.6)).sum() > 150      # 2 s and 0.5 s at 350 Hz
    on_sample = 0
    for name in cases.NAMES:                           # some grid point in some case sits exactly on a sample
        for t0 in cases.T0S:
            t, r = cases.make(name, cases.N_DEFAULT, t0)
            on_sample += int(np.isin(ref.uniform_grid(t)[1], t).sum())
    assert on_sample > 0


def test_screens_microsecond_grid_sits_on_samples(built):
    """the integer grid of the rates route: knots that ARE a sample (u = 1) in some case, beside the first knot (idx 0)"""
    hits = 0
    for run in RUNS:
        info, knots, q, us = hostile.case_route(*run)
        hits += int(np.isin(np.array(hostile.grid(us)[2], np.int64), us).sum())
    assert hits > 0


# ---- the host stand-in: gyro_math.hpp one sample after the other --------------------------------------------------------
def host_problem(hosttest_lib):
    import rssync_amd
    return rssync_amd.SyncProblem(seed=1, verbose=False, _lib=hosttest_lib)


@pytest.mark.parametrize("run", RUNS, ids=cases.run_id)
def test_host_stand_in_stays_within_the_scan_bound(hosttest_lib, run):
    name, n, t0, orientation = run
    info, knots, q, us = hostile.case_route(*run)
    t, r = cases.make(name, n, t0)
    h = host_problem(hosttest_lib)
    h.set_gyro_rates(t, r, orientation)
    assert h.gyro_info() == info
    err = float(np.max(np.abs(h.gyro_knots() - knots)))
    print("%s: host stand-in knot error %.3g" % (cases.run_id(run), err))
    assert err <= SCAN_ATOL
    if name == "still":
        assert np.array_equal(h.gyro_knots(), np.tile([1.0, 0, 0, 0], (info[2], 1)))
        assert not h.gyro_table()[:, 1:].any()


TIME_BASE = "time base"


def test_host_stand_in_names_the_time_base(hosttest_lib):
    """8 kHz for 10 s: the first grid sample, first timestamp x rate, passes 2^31 at 268 435 s (3.1 days of uptime)"""
    import rssync_amd
    n = 80000
    rng = np.random.default_rng(4)
    r = 0.3 * rng.standard_normal((n, 3))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rel = np.arange(n) / 8000.0
    h = host_problem(hosttest_lib)
    for t0 in (2.0e5, 268435.0):                            # 2^31 / 8000 = 268 435.456
        h.set_gyro_rates(t0 + rel, r)
        assert h.gyro_info()[0] == 8000.0 and h.gyro_info()[1] == t0
        h.SetGyroQuaternionsTimestamped(((t0 + rel) * 1e6).astype(np.int64), q)
        assert h.gyro_info()[:2] == (8000.0, t0)
    for t0 in (268436.0, 3.0e5, 6.0e5, 2.0e9, 1.2e9):       # (2^50 us = 1.126e9 s: the last is past that too)
        with pytest.raises(rssync_amd.RsSyncError, match=TIME_BASE):
            h.set_gyro_rates(t0 + rel, r)
        with pytest.raises(rssync_amd.RsSyncError, match="subtract a common offset"):
            h.SetGyroQuaternionsTimestamped(((t0 + rel) * 1e6).astype(np.int64), q)
        with pytest.raises(rssync_amd.RsSyncError, match="gyro data was not set"):
            h.gyro_table()
    # first timestamp 2^50 us, 16 kHz: the product first x rate leaves int64, the division does not
    big = (1 << 50) - 400 + np.arange(6) * 62
    with pytest.raises(rssync_amd.RsSyncError, match=TIME_BASE):
        h.SetGyroQuaternionsTimestamped(big, q[:6])
    # out of order AND past the grid: the time base is told first, it needs nothing but the end timestamps
    ts = ((3.0e5 + rel[:6]) * 1e6).astype(np.int64)
    ts[2], ts[3] = ts[3], ts[2]
    with pytest.raises(rssync_amd.RsSyncError, match=TIME_BASE):
        h.SetGyroQuaternionsTimestamped(ts, q[:6])
    h.set_gyro_rates(1.0 + rel, r)                          # and the object is usable afterwards
    assert h.gyro_info()[:2] == (8000.0, 1.0)


def test_host_stand_in_accepts_a_repeated_timestamp(hosttest_lib):
    t, r = cases.make("repeats", 50)
    us = cases.timestamps_us(t)
    assert (np.diff(us) == 0).sum() == 7
    q = hostile.orientations(t, r).astype(np.float64)
    h = host_problem(hosttest_lib)
    h.SetGyroQuaternionsTimestamped(us, q)                  # equal is not out of order
    assert h.gyro_info()[2] >= 48
    np.testing.assert_allclose(h.gyro_knots(), hostile.knots_of(us, q)[1].astype(np.float64), rtol=0, atol=2e-15)


# ---- interp_rate on what a real log does to the conditioning grid ---------------------------------------------------------
@pytest.mark.parametrize("name", ["repeats", "dropouts", "bursts", "deadband", "saturated"])
def test_interpolation_on_the_hostile_streams_is_bit_equal(shim, name):
    for t0 in (0, 65536):
        t, r = cases.make(name, cases.N_DEFAULT, t0)
        sr, t_new, want = ref.gyro_interpolate(t, r)
        rc, sr_c, first, count = shim_grid(shim, t)
        assert rc == 0 and sr_c == sr and count == t_new.size
        got = np.empty((count, 3))
        shim.interp(_pd(t), _pd(np.ascontiguousarray(r)), t.size, first, sr_c, count, _pd(got))
        np.testing.assert_array_equal(got, want)


def test_interpolation_takes_the_first_of_two_equal_timestamps(shim):
    """known answers: a grid point below a pair of equal timestamps weighs the pair's FIRST sample; one that sits on the
    pair takes the first as it is"""
    t = np.array([1.0, 1.003, 1.003, 1.0075, 1.01])            # 5 / 0.01 -> 500 Hz: grid 1.0, 1.002, .. 1.008
    r = np.array([[0.0, 0, 0], [10.0, 20, 30], [-50.0, -60, -70], [1.0, 1, 1], [2.0, 2, 2]])
    rc, sr_c, first, count = shim_grid(shim, t)
    assert (rc, sr_c, count) == (0, 500, 5)
    got = np.empty((count, 3))
    shim.interp(_pd(t), _pd(r), 5, first, sr_c, count, _pd(got))
    w = (1.002 - 1.0) / ((1.002 - 1.0) + (1.003 - 1.002))
    np.testing.assert_array_equal(got[1], (1.0 - w) * r[0] + w * r[1])
    t2 = np.array([1.0, 1.002, 1.002, 1.0075, 1.01])
    shim.interp(_pd(t2), _pd(r), 5, first, sr_c, count, _pd(got))
    np.testing.assert_array_equal(got[1], r[1])
    w = (1.004 - 1.002) / ((1.004 - 1.002) + (1.0075 - 1.004))
    np.testing.assert_array_equal(got[2], (1.0 - w) * r[2] + w * r[3])   # and ABOVE the pair the lower neighbour is its last
