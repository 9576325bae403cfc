"""Gyro conditioning without a GPU (DESIGN.md section 3 "Gyro conditioning"): the arithmetic the kernels inline
(rs-sync_amd/csrc/gyro_signal_math.hpp, HIP-free) compiled with g++ behind a C shim, against the sequential numpy
restatement of the reference (tests/gyro_signal_reference.py: core_support/signal.cpp:3-31, :53-85); the host's setting
through the CPU test double of the device ABI; and a known-answer check of the time alignment with the oracle.

THE CHUNKED FILTER'S ROUNDING.  The yardstick is the sequential fp64 restatement's own largest error against the same
filter in long double, e_seq; the chunked form (a thread runs a chunk from the state zero, the chunk ends are carried
with tabulated powers of the companion matrix, the chunk is run again from its true state) must stay within R x e_seq.
R = twice the largest ratio measured for the carry scheme that ships (powers by long-double squarings rounded once, plain
fp64 carry).  Measured: err_chunked / e_seq on synth.make_gyro(fs=8000) rates (2 rad/s sinusoids plus noise), seeds
0 .. 5, lengths 5000 / 40 003 / 200 001, the four layouts of LAYOUTS plus the device's own (lowpass_chunk_for) --
the worst of the 90 runs per divider (4 and 8: this file's one signal):

    divider      3      4      8      32     64     256
    e_seq        1e-15  4e-16  7e-16  7e-15  2e-14  1.4e-13
    worst ratio  1.18   1.00   1.01   1.39   1.55   2.19

R = 2 x 2.19 = 4.4 (gyro_signal_reference.CHUNKED_R; the condition R <= 32 is part of the test).  A naive carry
(numpy.linalg.matrix_power in fp64) measured 4-11 at divider 256.

THE STREAMS OF tests/gyro_cases.py (plateaus with step edges, exact zeros, gaps, bursts), gridded as the device grids them,
5003 and 70 001 samples, the same five layouts -- the worst of the 40 runs per divider, and where it was met:

    divider      3                    32                 256
    e_seq        6e-16 .. 3e-14       3e-15 .. 2e-13     4e-14 .. 3e-12     (the largest: `saturated`, 35 rad/s steps)
    worst ratio  1.23                 1.62               2.70
    met on       saturated, 70 001    bursts, 70 001     deadband, 5003, chunks of 32 x 1024 threads
    per stream   saturated 1.32, deadband 2.70, dropouts 2.12, bursts 2.38 (all at divider 256); the device's own layout: 1.36

2.70 is above CHUNKED_R / 2, so these streams are held to a constant of their own, twice their largest ratio:
gyro_signal_reference.CHUNKED_R_HOSTILE = 5.4.  CHUNKED_R stays, and so does every test that uses it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gyro_signal_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_BOUND = ref.CHUNKED_R   # 2 x the largest ratio measured (table above); must not exceed 32
DIVIDERS = (3, 4, 8, 32, 64, 256)
# (chunk, threads per segment): 32 x 1024 is the device's layout for long streams (40 000 samples: two segments, the
# second level); 157: an odd length, one segment; 8 threads: many segments, every level of the scan and the segment carry
LAYOUTS = ((32, 1024), (157, 1024), (32, 8), (157, 8))

SHIM = r'''
#include <vector>
#include <array>
#include "gyro_signal_math.hpp"
extern "C" {
int grid(double t_first, double t_last, unsigned long n, int* sr, long* first, unsigned long* count) {
    rs::UniformGrid g;
    const int rc = rs::uniform_grid_of(t_first, t_last, n, &g);
    *sr = g.sr; *first = g.first_sample; *count = g.count;
    return rc;
}
void interp(const double* ts, const double* rates, unsigned n, long first, int sr, unsigned m, double* out) {
    for (unsigned i = 0; i < m; ++i) rs::interp_rate(ts, rates, n, rs::ugrid_time(first + i, sr), out + 3 * (size_t)i);
}
void coef(int divider, double* out) {
    const rs::LowpassCoef k = rs::lowpass_coef(divider);
    out[0] = k.b0; out[1] = k.b1; out[2] = k.b2; out[3] = k.a1; out[4] = k.a2;
}
unsigned chunk_for(unsigned long n, unsigned threads) { return rs::lowpass_chunk_for(n, threads); }

// one pass in the layout of gyro_lowpass_kernel: `threads` (= 2^levels) chunks per segment, a host loop per barrier interval
static void pass(const double* in, double* out, unsigned n, bool reverse, const rs::LowpassCoef& k, const rs::CarryTable& tab, unsigned chunk,
                 unsigned threads, int levels) {
    typedef std::array<double, 6> St;
    const unsigned long seg = (unsigned long)chunk * threads;
    const unsigned n_seg = (unsigned)((n + seg - 1) / seg);
    std::vector<St> seg_state(n_seg);
    auto segment = [&](unsigned b, double* o) {
        std::vector<St> s(threads), start(threads, St{0, 0, 0, 0, 0, 0});
        std::vector<unsigned> lo(threads), hi(threads);
        const unsigned long first = b * seg, seg_end = first + seg < n ? first + seg : n;
        if (b > 0 && o) start[0] = seg_state[b - 1];
        for (unsigned t = 0; t < threads; ++t) {
            const unsigned long l = first + (unsigned long)t * chunk < seg_end ? first + (unsigned long)t * chunk : seg_end;
            lo[t] = (unsigned)l;
            hi[t] = (unsigned)(l + chunk < seg_end ? l + chunk : seg_end);
            double st[3][2];
            for (int c = 0; c < 6; ++c) st[c >> 1][c & 1] = start[t][c];
            rs::lowpass_run(k, in, nullptr, n, reverse, lo[t], hi[t], st);
            for (int c = 0; c < 6; ++c) s[t][c] = st[c >> 1][c & 1];
        }
        for (int lvl = 0; lvl < levels; ++lvl) {
            const unsigned off = 1u << lvl;
            const std::vector<St> before = s;
            for (unsigned t = off; t < threads; ++t) {
                double from[3][2], v[3][2];
                for (int c = 0; c < 6; ++c) { from[c >> 1][c & 1] = before[t - off][c]; v[c >> 1][c & 1] = before[t][c]; }
                rs::carry_step(tab.p[lvl], from, v);
                for (int c = 0; c < 6; ++c) s[t][c] = v[c >> 1][c & 1];
            }
        }
        if (!o) { seg_state[b] = s[threads - 1]; return; }
        for (unsigned t = 0; t < threads; ++t) {
            double st[3][2];
            for (int c = 0; c < 6; ++c) st[c >> 1][c & 1] = t ? s[t - 1][c] : start[0][c];
            rs::lowpass_run(k, in, o, n, reverse, lo[t], hi[t], st);
        }
    };
    if (n_seg > 1) {
        for (unsigned b = 0; b < n_seg; ++b) segment(b, nullptr);
        for (unsigned b = 1; b < n_seg; ++b) { // gyro_lowpass_carry_kernel
            double prev[3][2], v[3][2];
            for (int c = 0; c < 6; ++c) { prev[c >> 1][c & 1] = seg_state[b - 1][c]; v[c >> 1][c & 1] = seg_state[b][c]; }
            rs::carry_step(tab.p[levels], prev, v);
            for (int c = 0; c < 6; ++c) seg_state[b][c] = v[c >> 1][c & 1];
        }
    }
    for (unsigned b = 0; b < n_seg; ++b) segment(b, out);
}
// forward then backward over x[n][3] -> y[n][3]
void lowpass(const double* x, double* y, unsigned n, int divider, unsigned chunk, unsigned threads) {
    int levels = 0;
    while ((1u << levels) < threads) ++levels;
    const rs::LowpassCoef k = rs::lowpass_coef(divider);
    const rs::CarryTable tab = rs::carry_table(k, chunk);
    std::vector<double> tmp(3 * (size_t)n);
    pass(x, tmp.data(), n, false, k, tab, chunk, threads, levels);
    pass(tmp.data(), y, n, true, k, tab, chunk, threads, levels);
}
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("gyro_signal")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    out = d / "libgyrosignal.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "rs-sync_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(out), str(src)])
    L = ctypes.CDLL(str(out))
    PD = ctypes.POINTER(ctypes.c_double)
    L.grid.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_ulong, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_long),
                       ctypes.POINTER(ctypes.c_ulong)]
    L.interp.argtypes = [PD, PD, ctypes.c_uint, ctypes.c_long, ctypes.c_int, ctypes.c_uint, PD]
    L.coef.argtypes = [ctypes.c_int, PD]
    L.chunk_for.argtypes = [ctypes.c_ulong, ctypes.c_uint]
    L.chunk_for.restype = ctypes.c_uint
    L.lowpass.argtypes = [PD, PD, ctypes.c_uint, ctypes.c_int, ctypes.c_uint, ctypes.c_uint]
    return L


def _pd(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def shim_grid(L, ts):
    sr, first, count = ctypes.c_int(), ctypes.c_long(), ctypes.c_ulong()
    rc = L.grid(float(ts[0]), float(ts[-1]), ts.size, ctypes.byref(sr), ctypes.byref(first), ctypes.byref(count))
    return rc, sr.value, first.value, count.value


def shim_lowpass(L, x, divider, chunk, threads=1024):
    x = np.ascontiguousarray(x, np.float64)
    y = np.empty_like(x)
    L.lowpass(_pd(x), _pd(y), x.shape[0], divider, chunk, threads)
    return y


def jittered(n, fs, seed, t0=0.37):
    rng = np.random.default_rng(seed)
    t = t0 + np.arange(n) / fs + rng.uniform(-0.2, 0.2, size=n) / fs
    return np.sort(t)


# ---- the grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fs,seed,t0", [(400, 400.0, 0, 0.37), (1000, 8000.0, 1, -1.0), (777, 421.0, 2, 12.5),   # 421 -> 400
                                          (900, 426.0, 3, 0.0), (300, 1975.0, 4, 3.0), (50, 99.0, 5, 100.0)])      # 426 -> 450, 1975 -> 2000
def test_grid_count_and_first_sample_equal_the_push_back_loop(shim, n, fs, seed, t0):
    ts = jittered(n, fs, seed, t0)
    sr, grid = ref.uniform_grid_loop(ts)
    rc, sr_c, first, count = shim_grid(shim, ts)
    assert rc == 0 and sr_c == sr and count == grid.size
    assert first == int(np.ceil(ts[0] * sr)) and first / sr == grid[0]
    sr_v, grid_v = ref.uniform_grid(ts)                 # the restatement's block form, which the GPU tests use
    assert sr_v == sr
    np.testing.assert_array_equal(grid_v, grid)


def test_grid_when_the_span_ends_exactly_on_a_grid_point(shim):
    # 400 samples from 1.0 to 2.0 s: 400 / 1.0 -> 400 Hz, grid 400 .. while s / 400 < 2.0: 400 points, 2.0 itself excluded
    ts = np.linspace(1.0, 2.0, 400)
    sr, grid = ref.uniform_grid_loop(ts)
    rc, sr_c, first, count = shim_grid(shim, ts)
    assert (rc, sr_c, first, count) == (0, 400, 400, 400) and sr == 400 and grid.size == 400 and grid[-1] < 2.0
    # and one that ends a hair above a grid point keeps it
    ts2 = ts.copy()
    ts2[-1] = np.nextafter(2.0, 3.0)
    assert shim_grid(shim, ts2)[3] == ref.uniform_grid_loop(ts2)[1].size == 401


def test_grid_refuses_an_empty_span(shim):
    assert shim_grid(shim, np.array([1.0, 1.0]))[0] != 0
    assert shim_grid(shim, np.array([2.0, 1.0]))[0] != 0


@pytest.mark.parametrize("n,fs,seed", [(400, 400.0, 0), (3000, 8000.0, 1)])
def test_interpolation_is_bit_equal(shim, n, fs, seed):
    ts = jittered(n, fs, seed)
    rates = np.random.default_rng(seed).normal(size=(n, 3))
    sr, t_new, want = ref.gyro_interpolate(ts, rates)
    rc, sr_c, first, count = shim_grid(shim, ts)
    got = np.empty((count, 3))
    shim.interp(_pd(ts), _pd(np.ascontiguousarray(rates)), n, first, sr_c, count, _pd(got))
    np.testing.assert_array_equal(got, want)


def test_interpolation_takes_a_sample_that_sits_on_the_grid(shim):
    ts = np.array([1.0, 1.0025, 1.004, 1.0075, 1.01])        # 5 / 0.01 = 500 Hz; grid 1.0, 1.002, .. 1.008
    rates = np.arange(15.0).reshape(5, 3)
    sr, t_new, want = ref.gyro_interpolate(ts, rates)
    rc, sr_c, first, count = shim_grid(shim, ts)
    assert (sr_c, count) == (500, 5)
    got = np.empty((count, 3))
    shim.interp(_pd(ts), _pd(rates), 5, first, sr_c, count, _pd(got))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0], rates[0])
    np.testing.assert_array_equal(got[2], rates[2])         # 1.004 is a timestamp


# ---- the filter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("divider", DIVIDERS)
def test_coefficients_equal_the_restatement(shim, divider):
    c = np.empty(5)
    shim.coef(divider, _pd(c))
    np.testing.assert_array_equal(c, np.array(ref.lowpass_coef(divider), np.float64))


@pytest.mark.parametrize("n", [3, 4, 5, 1000])
@pytest.mark.parametrize("divider", [3, 32, 256])
def test_one_chunk_is_bit_equal_to_the_sequential_filter(shim, n, divider):
    x = np.random.default_rng(n).normal(size=(n, 3))
    want = ref.gyro_lowpass(x, divider)
    got = shim_lowpass(shim, x, divider, chunk=n, threads=1)
    np.testing.assert_array_equal(got, want)
    if n == 3:   # edges: nothing is written back by either pass
        np.testing.assert_array_equal(got, x)
    if n == 4:   # the forward pass writes samples 0, 1 (its inputs); the backward pass 3, 2 (ITS inputs): unchanged as well
        np.testing.assert_array_equal(got, x)


def test_edges_of_a_pass():
    # n = 5: forward writes y[2] only (0, 1 are inputs; 3, 4 never written back); backward then rewrites sample 2 from (4, 3, 2)
    x = np.random.default_rng(0).normal(size=(5, 3))
    y = ref.gyro_lowpass(x, 8)
    np.testing.assert_array_equal(y[[0, 1, 3, 4]], x[[0, 1, 3, 4]])
    assert np.all(y[2] != x[2])


def filter_signal(n=40003, fs=8000.0, seed=3):
    from rssync_amd import synth
    g = synth.make_gyro(0.0, n / fs - 2.0, fs=fs, seed=seed)   # 2 rad/s sinusoids plus noise
    return np.ascontiguousarray(g.rates[:n])


def chunked_ratios(L, x, divider, layouts=LAYOUTS):
    """-> e_seq, [err_chunked / e_seq per layout]: both against the long-double run of THE SAME (fp64) coefficients"""
    coef = ref.lowpass_coef(divider)
    truth = ref.gyro_lowpass(x, divider, np.longdouble, coef=coef)
    seq = ref.gyro_lowpass(x, divider)
    e_seq = float(np.max(np.abs(seq - truth)))
    out = []
    for chunk, threads in layouts:
        got = shim_lowpass(L, x, divider, chunk, threads)
        out.append(float(np.max(np.abs(got - truth))) / e_seq)
    return e_seq, out


@pytest.mark.parametrize("divider", DIVIDERS)
def test_chunked_filter_stays_within_R_times_the_sequential_error(shim, divider):
    assert R_BOUND <= 32
    x = filter_signal()
    assert x.shape[0] % 32 and x.shape[0] % 157            # an uneven last chunk in every layout
    e_seq, ratios = chunked_ratios(shim, x, divider)
    print("divider %d: e_seq %.3g, err_chunked / e_seq %s" % (divider, e_seq, ["%.2f" % r for r in ratios]))
    assert e_seq > 0
    assert max(ratios) <= R_BOUND, (divider, e_seq, ratios)


@pytest.mark.parametrize("n", [5003, 70001])
@pytest.mark.parametrize("name", ["saturated", "deadband", "dropouts", "bursts"])
def test_chunked_filter_on_the_hostile_streams(shim, name, n):
    import gyro_cases
    t, r = gyro_cases.make(name, n)
    grid = ref.gyro_interpolate(t, r)[2]
    layouts = list(LAYOUTS) + [(shim.chunk_for(grid.shape[0], 1024), 1024)]     # ... and the device's own
    for divider in (3, 32, 256):
        e_seq, ratios = chunked_ratios(shim, grid, divider, layouts)
        print("%s, %d samples, divider %d: e_seq %.3g, err_chunked / e_seq %s" % (name, n, divider, e_seq, ["%.2f" % x for x in ratios]))
        assert e_seq > 0
        assert max(ratios) <= ref.CHUNKED_R_HOSTILE, (name, n, divider, e_seq, ratios)
        assert ratios[-1] <= R_BOUND, (name, n, divider, e_seq, ratios)      # what the device tests hold the device to


def test_the_device_layout_for_short_and_long_streams(shim):
    assert shim.chunk_for(3, 1024) == 2 and shim.chunk_for(5000, 1024) == 5 and shim.chunk_for(32768, 1024) == 32
    assert shim.chunk_for(10 ** 7, 1024) == 32
    # a short stream in the device's layout (chunks of 2: the smallest a chunk may be) is still the sequential filter's
    x = filter_signal()[:1501]
    for divider in (3, 256):
        e_seq, ratios = chunked_ratios(shim, x, divider, [(2, 1024)])
        assert ratios[0] <= R_BOUND


# ---- the host, through the CPU test double of the device ABI ----------------------------------------------------------
def host_problem(hosttest_lib):
    import rssync_amd
    return rssync_amd.SyncProblem(seed=1, _lib=hosttest_lib)


def test_the_setting_exists_in_the_public_interface(hosttest_lib):
    assert hasattr(hosttest_lib, "rssync_ext_set_gyro_conditioning") and hasattr(hosttest_lib, "rssync_ext_gyro_conditioned")
    header = open(os.path.join(ROOT, "include", "rssync_c.h")).read()
    assert "rssync_gyro_conditioning" in header and "rssync_ext_gyro_conditioned" in header


def test_the_cpu_double_refuses_the_setting_and_stays_usable(hosttest_lib):
    import rssync_amd
    from rssync_amd import synth
    gyro = synth.make_gyro(1.0, 1.5, seed=4)    # (from t = 0: the timestamped grid takes no negative times)
    p = host_problem(hosttest_lib)
    with pytest.raises(rssync_amd.RsSyncError, match="gyro conditioning: not available in this device layer"):
        p.set_gyro_conditioning(32, 8)
    with pytest.raises(rssync_amd.RsSyncError, match="gyro conditioning: not available in this device layer"):
        p.set_gyro_conditioning(0, 0)
    with pytest.raises(rssync_amd.RsSyncError, match="gyro conditioning: not available in this device layer"):
        p.gyro_conditioned()
    p.set_gyro_conditioning(None)
    fresh = host_problem(hosttest_lib)
    for q in (p, fresh):
        q.set_gyro_rates(gyro.times, gyro.rates, "XYZ")
    np.testing.assert_array_equal(p.gyro_knots(), fresh.gyro_knots())
    assert p.gyro_info() == fresh.gyro_info()
    for q in (p, fresh):
        q.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    np.testing.assert_array_equal(p.gyro_knots(), fresh.gyro_knots())
    ts_us, quats = synth.make_timestamped(gyro, seed=4)
    for q in (p, fresh):
        q.SetGyroQuaternionsTimestamped(ts_us, quats)
    np.testing.assert_array_equal(p.gyro_knots(), fresh.gyro_knots())


@pytest.mark.parametrize("divider,k,message", [
    (2, 0, "lowpass_divider 2"), (-1, 0, "lowpass_divider must be"), (257, 0, "lowpass_divider must be"),
    (0, -1, "decimate must be"), (256, 65, "decimate must be"), (0, 2, "needs lowpass_divider >= 4"),
    (15, 8, "needs lowpass_divider >= 16"), (3, 2, "needs lowpass_divider >= 4")])
def test_parameter_errors_have_their_own_messages(hosttest_lib, divider, k, message):
    import rssync_amd
    p = host_problem(hosttest_lib)
    with pytest.raises(rssync_amd.RsSyncError, match=message):
        p.set_gyro_conditioning(divider, k)     # (checked before the device layer is asked for anything)


# ---- time alignment, with the oracle -----------------------------------------------------------------------------------
def test_decimation_does_not_move_the_delay(built):
    """An 8 kHz gyro, noise-free frames.  (a) raw: every sample a knot; (b) the conditioned route's restatement
    (divider 32, k = 8) through the oracle's uniform setter with first_timestamp = grid time 0 + (k - 1) / (2 sr);
    (c) the same with the shift left out.  |b - a| <= 1e-4 s (the project's north star); |c - a| > 3e-4 s: the shift
    is needed (predicted (k - 1) / (2 sr) = 4.375e-4 s)."""
    from rssync_amd import synth
    from oracle.oracle import OracleProblem
    F, N, k, divider = 32, 128, 8, 32
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, fs=8000.0, seed=2)
    frames = list(synth.make_frames(gyro, 0, F, N, seed=2, noise=0.0, outliers=0.0))
    rates, fs, t0 = ref.conditioned(gyro.times, gyro.rates, divider, k)
    assert fs == 1000.0
    quats = ref.integrate(rates, k, 8000)
    shift = (k - 1) / (2 * 8000.0)

    def delay(q, rate, start):
        o = OracleProblem(seed=2, max_outer_iters=150, threads=os.cpu_count() or 1, faithful=False)
        o.SetGyroQuaternions(q, rate, start)
        for fr, ta, tb, ra, rb in frames:
            o.SetTrackResult(fr, ta, tb, ra, rb)
        _, d0 = o.PreSync(0.0, 0, F, 0.001, 0.08)
        return o.Sync(d0, 0, F, 0.0, 0.08)[1]

    a = delay(gyro.quats, gyro.fs, gyro.t0)
    b = delay(quats, fs, t0)
    c = delay(quats, fs, t0 - shift)
    print("Sync delay: raw %.7f, conditioned %.7f (diff %.3g), without the shift %.7f (diff %.3g)" % (a, b, b - a, c, c - a))
    assert abs(a - synth.D_TRUE) <= 1e-4
    assert abs(b - a) <= 1e-4
    assert abs(c - a) > 3e-4
