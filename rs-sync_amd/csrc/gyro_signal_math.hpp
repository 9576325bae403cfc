// gyro_signal_math.hpp -- the arithmetic of gyro CONDITIONING (raw rates -> uniform grid -> zero-phase low-pass ->
// decimation), shared by the device kernels (kernels/gyro.hpp) and by tests/test_gyro_conditioning_cpu.py, which
// compiles this file with g++ and runs the chunked filter over an array with a host loop in the kernels' thread layout.
// HIP-free; fp64, contraction off: the restated operations must round as the reference's do.
//
// What each function restates (reference = VladimirP1/rs-sync, src/):
//   uniform_grid_of     core_support/signal.cpp:62-69 (rate rounded to 50 Hz, samples ceil(t0 sr) .. while s / sr < t1),
//                       count in closed form instead of the push-back loop
//   interp_rate         signal.cpp:74-79 (arma::interp1, linear: weight = distance to the lower neighbour / both distances)
//   lowpass_coef        signal.cpp:5-8
//   lowpass_step        signal.cpp:12-13, in its order of operations
//   lowpass_run         signal.cpp:11-18 for a contiguous chunk of one pass (either direction), all three axes
//   carry_*             NOT in the reference: how a chunk's true start state is obtained without running the samples before
//                       it one after the other (below)
//
// The recurrence y_i = u_i + a1 y_{i-1} + a2 y_{i-2}, u_i = b0 x_i + b1 x_{i-1} + b2 x_{i-2}, is linear in its state
// s_i = (y_i, y_{i-1}): s_i = A s_{i-1} + (u_i, 0), A = [[a1, a2], [1, 0]].  A chunk run from the state ZERO therefore ends
// in p with  true end state = A^len (true start state) + p.  With chunks of one length the true states at the chunk ends
// follow from a scan in which the step over `off` chunks multiplies by the CONSTANT matrix A^(len off): these powers are
// tabulated once per (divider, chunk length) on the host (carry_table; long double squarings, rounded once).  Each chunk is
// then run again from its true state with lowpass_step -- the only difference to the sequential filter is the rounding of
// that carried state.
#pragma once

#include <stdint.h>
#include <math.h>

#include "device_math.hpp"

namespace rs {

// ---- uniform grid ---------------------------------------------------------------------------------------------
struct UniformGrid {
    int32_t sr;            // grid rate, Hz (a multiple of 50)
    int64_t first_sample;  // grid sample s stands at time s / sr
    uint64_t count;
};
#define RS_UGRID_OK 0
#define RS_UGRID_BAD_RATE 1 /* span <= 0, or the rate rounds to <= 0 Hz or beyond int32 */

RS_HD double ugrid_time(int64_t sample, int32_t sr) {
#pragma clang fp contract(off)
    return (double)sample / (double)sr; // signal.cpp:68-69: `sample` is a double there, exact below 2^53
}

// signal.cpp:63-69 without the loop: the count is ceil(t_last sr) - first up to the rounding of one product and one
// division, so the estimate is corrected by testing the reference's own loop condition next to it (a few steps at most).
inline int uniform_grid_of(double t_first, double t_last, uint64_t n_samples, UniformGrid* g) {
#pragma clang fp contract(off)
    g->sr = 0; g->first_sample = 0; g->count = 0;
    if (!(t_last > t_first)) return RS_UGRID_BAD_RATE;
    const double actual_sr = (double)n_samples / (t_last - t_first);
    const double rounded = round(actual_sr / 50) * 50;
    if (!(rounded >= 50.0 && rounded <= 2.0e9)) return RS_UGRID_BAD_RATE;
    const int32_t sr = (int32_t)rounded;
    const double first = ceil(t_first * sr);
    if (!(fabs(first) < 4.0e15) || !(fabs(t_last * sr) < 4.0e15)) return RS_UGRID_BAD_RATE;
    int64_t end = (int64_t)ceil(t_last * sr); // first sample NOT below t_last, give or take
    while (ugrid_time(end - 1, sr) >= t_last) --end;
    while (ugrid_time(end, sr) < t_last) ++end;
    g->sr = sr;
    g->first_sample = (int64_t)first;
    g->count = end > g->first_sample ? (uint64_t)(end - g->first_sample) : 0;
    return RS_UGRID_OK;
}

// first index in ts[0..count) with ts[i] >= t
RS_HD uint32_t lower_bound_s(const double* ts, uint32_t count, double t) {
    uint32_t lo = 0, n = count;
    while (n > 0) {
        const uint32_t half = n >> 1;
        if (ts[lo + half] < t) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    return lo;
}

// the three rates at time t.  arma::interp1's linear rule: between the neighbours a (below) and b (at or above),
// weight = (t - ts[a]) / ((t - ts[a]) + (ts[b] - t)), value = (1 - weight) y[a] + weight y[b]; a sample that sits on t is
// taken as it is.  A grid point outside the timestamps (the first one can fall below ts[0] by the rounding of
// ceil(t0 sr) / sr; arma would answer NaN there) takes the nearest sample.
RS_HD void interp_rate(const double* ts, const double* rates, uint32_t count, double t, double out[3]) {
#pragma clang fp contract(off)
    uint32_t b = lower_bound_s(ts, count, t);
    if (b >= count) b = count - 1;
    if (b == 0 || ts[b] == t || !(ts[b] > t)) {
        for (int c = 0; c < 3; ++c) out[c] = rates[3 * (size_t)b + c];
        return;
    }
    const uint32_t a = b - 1;
    const double ea = t - ts[a], eb = ts[b] - t;
    const double w = ea > 0 ? ea / (ea + eb) : 0.0;
    for (int c = 0; c < 3; ++c) out[c] = (1.0 - w) * rates[3 * (size_t)a + c] + w * rates[3 * (size_t)b + c];
}

// ---- the Butterworth low-pass -----------------------------------------------------------------------------------
struct LowpassCoef { double b0, b1, b2, a1, a2; };

inline LowpassCoef lowpass_coef(int divider) { // signal.cpp:5-8
#pragma clang fp contract(off)
    const double ita = 1.0 / tan(M_PI / divider);
    const double q = sqrt(2.0);
    LowpassCoef k;
    k.b0 = 1.0 / (1.0 + q * ita + ita * ita);
    k.b1 = 2 * k.b0;
    k.b2 = k.b0;
    k.a1 = 2.0 * (ita * ita - 1.0) * k.b0;
    k.a2 = -(1.0 - q * ita + ita * ita) * k.b0;
    return k;
}

// signal.cpp:12-13: b0 x_i + b1 x_{i-1} + b2 x_{i-2} + a1 y_{i-1} + a2 y_{i-2}, summed from the left
RS_HD double lowpass_step(const LowpassCoef& k, double x0, double x1, double x2, double y1, double y2) {
#pragma clang fp contract(off)
    return k.b0 * x0 + k.b1 * x1 + k.b2 * x2 + k.a1 * y1 + k.a2 * y2;
}

// where sample i OF A PASS lives: the backward pass (signal.cpp:20-30) is the forward one over the reversed array
RS_HD size_t pass_index(uint32_t i, uint32_t n, bool reverse) { return reverse ? (size_t)(n - 1 - i) : (size_t)i; }

// Samples lo .. hi-1 of one pass over in[n][3].  st[axis] = {y[lo-1], y[lo-2]} on entry (ignored for lo == 0: the first
// two outputs of a pass are its inputs, signal.cpp:10), {y[hi-1], y[hi-2]} on return.  With `out`, sample i is written
// as the pass leaves it: y[i] up to n-3, the INPUT for the last two (:14 writes sample i-2; the loop ends before the last
// two are written back).  lo is 0 or >= 2.
RS_HD void lowpass_run(const LowpassCoef& k, const double* in, double* out, uint32_t n, bool reverse, uint32_t lo, uint32_t hi,
                       double st[3][2]) {
    double x1[3] = {0., 0., 0.}, x2[3] = {0., 0., 0.};
    if (lo >= 2)
        for (int c = 0; c < 3; ++c) {
            x1[c] = in[3 * pass_index(lo - 1, n, reverse) + c];
            x2[c] = in[3 * pass_index(lo - 2, n, reverse) + c];
        }
    for (uint32_t i = lo; i < hi; ++i) {
        const size_t at = 3 * pass_index(i, n, reverse);
        for (int c = 0; c < 3; ++c) {
            const double x0 = in[at + c];
            const double y = i < 2 ? x0 : lowpass_step(k, x0, x1[c], x2[c], st[c][0], st[c][1]);
            st[c][1] = st[c][0];
            st[c][0] = y;
            x2[c] = x1[c];
            x1[c] = x0;
            if (out) out[at + c] = i + 2 < n ? y : x0;
        }
    }
}

// ---- carrying the state over chunks -----------------------------------------------------------------------------
constexpr int kCarryLevels = 10;                 // a workgroup scans 2^10 chunks
struct CarryTable { double p[kCarryLevels + 1][4]; }; // p[j] = A^(chunk 2^j), row-major; p[kCarryLevels]: over one whole segment

// A^(chunk 2^j) by squarings in long double (64-bit significand on x86 hosts), rounded to double once per entry
inline CarryTable carry_table(const LowpassCoef& k, uint32_t chunk) {
    typedef long double L;
    auto mul = [](const L a[4], const L b[4], L o[4]) {
        const L r0 = a[0] * b[0] + a[1] * b[2], r1 = a[0] * b[1] + a[1] * b[3];
        const L r2 = a[2] * b[0] + a[3] * b[2], r3 = a[2] * b[1] + a[3] * b[3];
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    };
    L base[4] = {(L)k.a1, (L)k.a2, 1, 0}, acc[4] = {1, 0, 0, 1};
    for (uint32_t e = chunk; e; e >>= 1) { // A^chunk, binary
        if (e & 1u) mul(acc, base, acc);
        mul(base, base, base);
    }
    CarryTable t;
    for (int j = 0; j <= kCarryLevels; ++j) {
        for (int c = 0; c < 4; ++c) t.p[j][c] = (double)acc[c];
        mul(acc, acc, acc);
    }
    return t;
}

// v <- v + P from: one step of the scan over chunk end states, three axes
RS_HD void carry_step(const double P[4], const double from[3][2], double v[3][2]) {
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c) {
        const double f0 = from[c][0], f1 = from[c][1];
        v[c][0] = v[c][0] + (P[0] * f0 + P[1] * f1);
        v[c][1] = v[c][1] + (P[2] * f0 + P[3] * f1);
    }
}

// chunk length for a stream of n samples on `threads` threads per segment: one segment while chunks of up to 32 samples
// cover it, else segments of 32 threads samples; never below 2 (a chunk starts at sample 0 or holds two earlier ones)
RS_HD uint32_t lowpass_chunk_for(uint64_t n, uint32_t threads) {
    const uint64_t c = (n + threads - 1) / threads;
    return c < 2 ? 2u : c > 32 ? 32u : (uint32_t)c;
}

} // namespace rs
