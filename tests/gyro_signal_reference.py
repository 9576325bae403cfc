"""The reference's second gyro route, restated line by line in numpy: sequential, one sample after the other.

    gyro_lowpass      core_support/signal.cpp:3-31
    gyro_decimate     core_support/signal.cpp:53-60
    gyro_interpolate  core_support/signal.cpp:62-85
    integrate         core_testcode.cpp:26-34 (the `#if 0` driver: fixed-rate integration)

What the tests of gyro conditioning compare the product with (tests/test_gyro_conditioning_cpu.py,
tests/test_gpu_gyro_conditioning.py).  Every function takes ``dtype``: ``np.float64`` gives the operations of the
reference in its own precision and order, ``np.longdouble`` the same operations with a 64-bit significand, the yardstick
for rounding.  Nothing here touches the library."""
import numpy as np

# How far the library's CHUNKED filter may be from the long-double filter, in units of the sequential fp64 filter's own
# error against it (e_seq): twice the largest ratio measured for the carry scheme that ships.  The measurement and its
# table: tests/test_gyro_conditioning_cpu.py (header).
CHUNKED_R = 4.4
# The same for the streams of tests/gyro_cases.py (saturated, deadband, dropouts, bursts), a constant of their own: their
# largest measured ratio, 2.70 (`deadband`, 5003 samples, divider 256, chunks of 32), is above CHUNKED_R / 2, so they get
# twice THEIR largest ratio; CHUNKED_R and the tests that use it stay.  In the device's own layout (lowpass_chunk_for)
# the largest is 1.36.  The table: tests/test_gyro_conditioning_cpu.py (header).
CHUNKED_R_HOSTILE = 5.4


def uniform_grid(ts, dtype=np.float64):
    """signal.cpp:63-69 -> (rounded_sr, new_timestamps).  The rate and the grid are computed in fp64 whatever `dtype`
    is (they are the reference's own: the long-double yardstick is about the arithmetic ON the grid)."""
    ts = np.asarray(ts, np.float64)
    actual_sr = ts.size / (ts[-1] - ts[0])                            # :63
    rounded_sr = int(np.round(actual_sr / 50) * 50)                   # :64
    sample = np.ceil(ts[0] * rounded_sr)                              # :67
    # :67-69, the push-back loop, in blocks: every candidate passes through the same division and comparison
    n_est = int(np.ceil((ts[-1] - ts[0]) * rounded_sr)) + 4
    cand = sample + np.arange(n_est, dtype=np.float64)
    keep = cand / rounded_sr < ts[-1]                                 # :68
    n = int(np.argmin(keep)) if not keep.all() else n_est
    assert not keep[n:].any()
    return rounded_sr, (cand[:n] / rounded_sr).astype(dtype)         # :69


def uniform_grid_loop(ts):
    """signal.cpp:66-69 as written, a push-back loop (small inputs: the closed form is checked against it)."""
    ts = np.asarray(ts, np.float64)
    actual_sr = ts.size / (ts[-1] - ts[0])
    rounded_sr = int(np.round(actual_sr / 50) * 50)
    out = []
    sample = np.ceil(ts[0] * rounded_sr)
    while sample / rounded_sr < ts[-1]:
        out.append(sample / rounded_sr)
        sample += 1
    return rounded_sr, np.array(out)


def interp1_linear(ts, y, t_new, dtype=np.float64):
    """signal.cpp:74-79: arma::interp1, linear (its default).  Between the neighbours a (below) and b (at or above):
    weight = (t - ts[a]) / ((t - ts[a]) + (ts[b] - t)), value = (1 - weight) y[a] + weight y[b]; a sample that sits on t
    is taken as it is.  A grid point outside the timestamps (the first can fall below ts[0] by the rounding of
    ceil(t0 sr) / sr; arma answers NaN there) takes the nearest sample: the library's stated rule."""
    ts = np.asarray(ts, dtype)
    y = np.asarray(y, dtype)
    t_new = np.asarray(t_new, dtype)
    b = np.searchsorted(ts, t_new, side="left")                       # std::lower_bound
    b = np.minimum(b, ts.size - 1)
    a = np.maximum(b - 1, 0)
    ea = t_new - ts[a]
    eb = ts[b] - t_new
    den = ea + eb
    w = np.where(ea > 0, ea / np.where(den > 0, den, 1), 0).astype(dtype)
    out = (1 - w)[:, None] * y[a] + w[:, None] * y[b]
    exact = (b == 0) | (ts[b] == t_new) | ~(ts[b] > t_new)
    return np.where(exact[:, None], y[b], out).astype(dtype)


def gyro_interpolate(ts, rates, dtype=np.float64):
    """signal.cpp:62-85 -> (rounded_sr, new_timestamps, new_gyro [m][3])"""
    sr, t_new = uniform_grid(ts, dtype)
    return sr, t_new, interp1_linear(ts, rates, t_new, dtype)


def lowpass_coef(divider, dtype=np.float64):
    """signal.cpp:5-8"""
    one, two = dtype(1.0), dtype(2.0)
    ita = one / np.tan(dtype(np.pi) / dtype(divider))                 # (M_PI is a double)
    q = np.sqrt(two)
    b0 = one / (one + q * ita + ita * ita)
    b1 = 2 * b0
    b2 = b0
    a1 = two * (ita * ita - one) * b0
    a2 = -(one - q * ita + ita * ita) * b0
    return b0, b1, b2, a1, a2


def _pass(x, coef):
    """signal.cpp:10-18 for ONE axis, x a list of scalars (Python floats are IEEE doubles; np.longdouble scalars keep
    their precision); the backward pass (:20-30) is this over the reversed list"""
    b0, b1, b2, a1, a2 = coef
    s = list(x)
    o0, o1 = x[0], x[1]                                               # :10
    for i in range(2, len(x)):                                        # :11
        o2 = b0 * x[i] + b1 * x[i - 1] + b2 * x[i - 2] + a1 * o1 + a2 * o0   # :12-13
        s[i - 2] = o0                                                 # :14
        o0 = o1                                                       # :16
        o1 = o2                                                       # :17
    return s                                                          # (the last two samples are never written back)


def gyro_lowpass(samples, divider, dtype=np.float64, coef=None):
    """signal.cpp:3-31 on samples[n][3] (the reference holds them as 3 x n columns).  `coef`: filter with these
    coefficients (the fp64 ones) instead of computing them in `dtype`: the rounding yardstick runs THE SAME filter."""
    x = np.array(samples, dtype)
    if divider < 2 or x.shape[0] < 3:                                 # :4 (fewer than 3 columns: :10 would read past the end)
        return x
    k = coef if coef is not None else lowpass_coef(divider, dtype)
    k = tuple(float(c) for c in k) if dtype is np.float64 else tuple(dtype(c) for c in k)
    out = np.empty_like(x)
    for ax in range(3):
        col = x[:, ax].tolist() if dtype is np.float64 else list(x[:, ax])
        fwd = _pass(col, k)                                           # :10-18
        out[:, ax] = _pass(fwd[::-1], k)[::-1]                        # :20-30
    return out


def gyro_decimate(samples, divider):
    """signal.cpp:53-60"""
    if divider < 2:
        return samples
    n = samples.shape[0] // divider                                   # :56
    return samples[np.arange(n) * divider].copy()                     # :58


def quat_from_aa(aa):
    """core_support/quat.cpp:5-17"""
    th2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]
    if th2 > 0:
        th = np.sqrt(th2)
        half = th * aa.dtype.type(0.5)
        kk = np.sin(half) / th
        return np.array([np.cos(half), aa[0] * kk, aa[1] * kk, aa[2] * kk], aa.dtype)
    return np.array([1, aa[0] * 0.5, aa[1] * 0.5, aa[2] * 0.5], aa.dtype)


def quat_prod(d, p):
    """core_support/quat.cpp:33-38"""
    return np.array([d[0] * p[0] - d[1] * p[1] - d[2] * p[2] - d[3] * p[3],
                     d[0] * p[1] + d[1] * p[0] + d[2] * p[3] - d[3] * p[2],
                     d[0] * p[2] - d[1] * p[3] + d[2] * p[0] + d[3] * p[1],
                     d[0] * p[3] + d[1] * p[2] - d[2] * p[1] + d[3] * p[0]], d.dtype)


def integrate(rates, k, sr, dtype=np.float64):
    """core_testcode.cpp:28-33 with a sample standing for k / sr seconds (k = 1: the reference to the letter)"""
    r = np.asarray(rates, dtype)
    q = np.empty((r.shape[0], 4), dtype)
    q[0] = [1, 0, 0, 0]                                               # :29
    for i in range(1, r.shape[0]):                                    # :30
        v = quat_prod(quat_from_aa(r[i] * dtype(k) / dtype(sr)), q[i - 1])   # :32
        q[i] = v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3])
    return q


def integrate_fast(rates, k, sr):
    """integrate() for long streams: the same products as a vectorised prefix scan (fp64; association differs from
    the sequential loop as the device's scan does -- the tests' bound for it is that of tests/test_gpu_gyro.py)."""
    from rssync_amd import synth
    r = np.asarray(rates, np.float64)
    dq = synth.quat_from_aa(r * float(k) / float(sr))
    dq[0] = [1.0, 0.0, 0.0, 0.0]
    q = dq.copy()
    shift = 1
    while shift < r.shape[0]:
        q[shift:] = synth.quat_mul(q[shift:], q[:-shift].copy())
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        shift *= 2
    return q


def orient(rates, orientation):
    """telemetry-parser's three-letter axis string: position = output axis, letter = input axis, lower case = minus"""
    out = np.empty_like(rates)
    for i, ch in enumerate(orientation):
        out[:, i] = rates[:, "xyz".index(ch.lower())] * (1.0 if ch.isupper() else -1.0)
    return out


def conditioned(ts, rates, divider, k, dtype=np.float64, coef=None):
    """The conditioned route up to the integration -> (rates [m // k][3], sample rate after decimation,
    first_timestamp).  first_timestamp = grid time 0 + (k - 1) / (2 sr): a decimated sample integrated over k / sr
    stands for the mean of the k samples that end at it, whose centre lies (k - 1) / (2 sr) before the sample."""
    sr, t_new, g = gyro_interpolate(ts, rates, dtype)
    g = gyro_lowpass(g, divider, dtype, coef)
    g = gyro_decimate(g, k)
    k = max(int(k), 1)
    return g, sr / k, float(np.float64(t_new[0])) + (k - 1) / (2.0 * sr)
