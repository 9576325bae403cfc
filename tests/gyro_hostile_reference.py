"""The rates route (angular rates -> orientations -> integer-microsecond grid -> knots) in numpy long double (a 64-bit
significand on x86 hosts, as tests/gyro_signal_reference.py already relies on): the yardstick the device, the host
stand-in and the fp64 oracle are measured against in tests/test_gyro_cases_cpu.py and tests/test_gpu_gyro_hostile.py.

    deltas       core_support/quat.cpp:5-17 via core_testcode.cpp:41-46   rotation by rate * dt, dt = t_i - t_{i-1} taken
                                                                           in fp64 as gyro_rates_kernel takes it
    orientations core_testcode.cpp:36-47                                   q_0 = 1, q_i = dq_i q_{i-1}: a vectorised prefix scan
    timestamps   core_testcode.cpp:48-50                                   (int64)(t * 1e6) in fp64, as the reference does it
    grid         core_private.cpp:147-160                                  Python integers: no width to overflow
    slerp        core_support/quat.cpp:55-74, core_private.cpp:162-176     flip on a negative dot; lerp when theta <= 1e-9
                                                                           or theta is not a number

THE PER-STEP NORMALISATION (core_testcode.cpp:45) IS DROPPED from the product.  It is there to stop fp64 drift; here the
deltas are unit quaternions to beyond long-double precision -- cos^2 + sin^2 in the branch th2 > 0, and the else-branch
[1, w / 2] only runs where th2 == 0 IN LONG DOUBLE, whose exponent range reaches 1e-4932: for the streams of
tests/gyro_cases.py that is w == 0 exactly (fp64 takes the else-branch for |w| < 1e-154 already, where 1 + |w|^2 / 4 is 1
to 300 digits) -- so the product of n of them is a unit quaternion to n x 1e-19, and one normalisation at the end
removes that.  Nothing here touches the library."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "this reference needs a long double wider than fp64"


def orient(rates, orientation):
    """telemetry-parser's three-letter axis string: position = output axis, letter = input axis, lower case = minus"""
    if orientation is None:
        return np.asarray(rates, np.float64)
    out = np.empty_like(rates)
    for i, ch in enumerate(orientation):
        out[:, i] = rates[:, "xyz".index(ch.lower())] * (1.0 if ch.isupper() else -1.0)
    return out


def quat_mul(p, q):
    """Hamilton product, [w,x,y,z] (core_support/quat.cpp:33-38), over leading dimensions, in the arrays' type"""
    pw, px, py, pz = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    qw, qx, qy, qz = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([pw * qw - px * qx - py * qy - pz * qz,
                     pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw], axis=-1)


def _split(a):
    c = a * LD(4294967297.0)                                           # Veltkamp: 2^32 + 1 halves a 64-bit significand
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """-> (p, e) with p = round(a b) and p + e = a b exactly (Dekker)"""
    p = a * b
    a1, a2 = _split(a)
    b1, b2 = _split(b)
    return p, ((a1 * b1 - p) + a1 * b2 + a2 * b1) + a2 * b2


def two_sum(a, b):
    """-> (s, e) with s = round(a + b) and s + e = a + b exactly (Knuth)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def deltas(t, rates, orientation=None):
    """dq[n][4] in long double: identity at 0, then the rotation by rate_i * (t_i - t_{i-1}); the difference in fp64
    (what the stream IS: the kernel's dt), the product and everything after it in long double.

    THE ANGLE is carried in two long doubles (w = rate * dt as an exact product, |w|^2 as a compensated sum, the root
    with one correction step): a relative error of 5e-20 in an angle of 3.5 rad per sample (`flip`) is 2e-19 per step and,
    as a random walk over 5000 steps, 1.4e-17 at the end -- above the 1e-17 to which tests/test_gyro_cases_cpu.py holds
    this file against a closed form.  What is left is the rounding of the four components, once per step."""
    t = np.asarray(t, np.float64)
    r = orient(rates, orientation).astype(LD)
    dt = np.concatenate([[0.0], np.diff(t)]).astype(LD)[:, None]
    wh, wl = two_prod(r, np.broadcast_to(dt, r.shape).copy())          # w = wh + wl
    p, e = two_prod(wh, wh)
    e = e + 2 * wh * wl
    s, e1 = two_sum(p[:, 0], p[:, 1])
    s, e2 = two_sum(s, p[:, 2])
    th2, th2_lo = two_sum(s, (e1 + e2) + (e[:, 0] + e[:, 1] + e[:, 2]))
    pos = th2 > 0                                                      # quat.cpp:7
    th = np.sqrt(np.where(pos, th2, LD(1)))
    p, e = two_prod(th, th)
    th_lo = (((th2 - p) - e) + th2_lo) / (2 * th)                      # th + th_lo = sqrt(th2 + th2_lo)
    th_lo = np.where(pos, th_lo, LD(0))
    hh, hl = th * LD(0.5), th_lo * LD(0.5)
    sn = np.sin(hh) + hl * np.cos(hh)
    cs = np.cos(hh) - hl * np.sin(hh)
    kk = np.where(pos, sn / th, LD(0.5))[:, None]                      # :8-12 / :14-15
    xyz = wh * kk + (wl - wh * (th_lo / th)[:, None]) * kk
    return np.concatenate([np.where(pos, cs, LD(1))[:, None], xyz], axis=1)


def orientations(t, rates, orientation=None):
    """q[n][4] in long double: the running product, the later factor on the left, as a Hillis-Steele scan"""
    q = deltas(t, rates, orientation)
    shift = 1
    while shift < q.shape[0]:
        q[shift:] = quat_mul(q[shift:], q[:-shift].copy())
        shift *= 2
    return q / np.sqrt(np.sum(q * q, axis=1, keepdims=True))


def timestamps_us(t):
    return (np.asarray(t, np.float64) * 1000000).astype(np.int64)       # core_testcode.cpp:48-50


def grid(ts_us):
    """core_private.cpp:147-160 -> (rate in Hz, first grid sample, grid times in us as a list of Python integers)"""
    first, last, count = int(ts_us[0]), int(ts_us[-1]), len(ts_us)
    assert 0 <= first < last
    actual_sr_uhz = 1000000 * 1000000 * count // (last - first)
    v = float(actual_sr_uhz) / 50.0 / 1000000.0                        # :149: two double divisions ...
    sr = (int(np.floor(v)) + (1 if v - np.floor(v) >= 0.5 else 0)) * 50   # ... and C's round(): halves away from zero
    assert sr > 0
    sample = first * sr // 1000000
    times = []
    while 1000000 * sample // sr < last:
        times.append(1000000 * sample // sr)
        sample += 1
    return sr, first * sr // 1000000, times


def last_grid_sample(ts_us, sr):
    """ceil(last_us * sr / 1e6): where the oracle's `int` loop counter ends.  It must stay below 2^31."""
    return -((-int(ts_us[-1]) * int(sr)) // 1000000)


def slerp(p, q, u):
    """core_support/quat.cpp:55-74 over rows, in long double"""
    dot = np.sum(p * q, axis=1)
    neg = dot < 0
    q = np.where(neg[:, None], -q, q)
    dot = np.where(neg, np.sum(p * q, axis=1), dot)
    with np.errstate(invalid="ignore"):
        theta = np.arccos(dot)                                         # not a number above 1
        curved = theta > LD(1e-9)                                      # False for NaN: the lerp
        th = np.where(curved, theta, LD(1))
        st = np.sin(th)
        m1 = np.where(curved, np.sin((1 - u) * th) / st, 1 - u)
        m2 = np.where(curved, np.sin(u * th) / st, u)
    return m1[:, None] * p + m2[:, None] * q


def knots_of(ts_us, quats):
    """core_private.cpp:147-176 -> (info, knots): info = (rate, time of the first knot in s, knot count) as the
    library's gyro_info() reports it; knots [m][4] in long double"""
    ts_us = np.asarray(ts_us, np.int64)
    sr, first_sample, times = grid(ts_us)
    tg = np.array(times, np.int64)
    idx = np.searchsorted(ts_us, tg, side="left")                      # std::lower_bound
    assert idx.max() < ts_us.size
    lo = np.maximum(idx - 1, 0)
    num = (tg - ts_us[lo]).astype(LD)
    den = (ts_us[idx] - ts_us[lo]).astype(LD)
    assert np.all(den[idx > 0] > 0)                                    # lower_bound never lands on the second of two equals
    u = num / np.where(idx > 0, den, LD(1))
    quats = np.asarray(quats, LD)
    out = slerp(quats[lo], quats[idx], u)
    out[idx == 0] = quats[0]
    start = float(np.float64(1000000 * first_sample // sr) / np.float64(1000000))
    return (float(sr), start, len(times)), out


def rates_route(t, rates, orientation=None):
    """-> (info, knots in long double, orientations in long double, timestamps in us)"""
    q = orientations(t, rates, orientation)
    us = timestamps_us(t)
    info, knots = knots_of(us, q)
    return info, knots, q, us


_routes = {}


def case_route(name, n, t0_s, orientation):
    """rates_route of a stream of tests/gyro_cases.py, computed once per session and left unchanged"""
    import gyro_cases
    key = (name, n, t0_s, orientation)
    if key not in _routes:
        t, r = gyro_cases.make(name, n, t0_s)
        _routes[key] = rates_route(t, r, orientation)
    return _routes[key]
