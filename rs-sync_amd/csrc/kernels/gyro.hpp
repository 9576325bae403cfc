// gyro.hpp -- the gyro side of the problem on the device: angular rates -> orientations (a scan of
// quaternion products), orientations -> the uniform integer-microsecond grid, grid -> natural-spline table.
// Part of the single HIP translation unit rssync_kernels.hip (included there, in order).
//
// Reference: core_testcode.cpp:36-52 (optdata_fill_gyro), core_private.cpp:142-190 (the timestamped
// setter), minispline.cpp:3-46 (spline coefficients).  The arithmetic per sample is gyro_math.hpp's; what is
// specific to the device is how the two sequential recurrences are cut:
//   * integration q_i = normalise(dq_i q_{i-1}) is a scan under the quaternion product: a workgroup takes a
//     segment of kScanSegment samples, every thread a contiguous chunk of it (sequential inside the chunk, with the
//     reference's normalisation per step), a 1024-wide scan of the chunk products in LDS, then the chunk again
//     from its prefix; with more than one segment the segment totals are scanned the same way by one workgroup
//     and a last pass multiplies every later segment by the product of the segments before it;
//   * the spline's tridiagonal solve has data-independent pivots (tabulated, gyro_math.hpp) and a
//     recurrence factor of 2 - sqrt(3) = 0.268 per row in both sweeps: what a row sees of a row k places away
//     is below 0.268^k, so every thread solves a short run of rows after a warm-up of kSplineWarm rows started
//     from zero, all runs in parallel.  0.268^64 = 2.5e-37 cannot be seen in fp64 BESIDE A VALUE OF ORDINARY SIZE.  Where
//     the data stands still (a camera at rest: equal knots, right-hand sides exactly 0) the sequential solve decays
//     through 1e-40 .. 1e-300 down to 0, and there the warm-up's start is all there is to see: a run that meets a value
//     below kSplineCertain is solved again after kSplineWarmLong rows, where 0.268^576 times any coefficient of unit
//     quaternions is below half the smallest subnormal.  The table is the sequential solve's bit for bit on both paths.
#pragma once

namespace {

constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

struct GyroStatus {
    uint32_t out_of_order; // smallest i with ts[i-1] > ts[i], kNoIndex if none
    uint32_t bad_input;    // a non-finite timestamp or rate
    uint32_t bad_knot;     // a non-finite knot after interpolation
    uint32_t pad;
};

__global__ void gyro_status_reset_kernel(GyroStatus* st) {
    st->out_of_order = kNoIndex;
    st->bad_input = 0;
    st->bad_knot = 0;
    st->pad = 0;
}

struct GyroRatesParams {
    const double* ts;    // [n] seconds
    const double* rates; // [n][3] rad/s
    int64_t* us;         // [n] out: whole microseconds (core_testcode.cpp:48-50)
    double* dq;          // [n][4] out: rotation over (t_i - t_{i-1}); identity at 0
    GyroStatus* st;
    uint32_t n;
    int32_t axis[3];     // output axis c reads input axis axis[c] ...
    double sign[3];      // ... times sign[c] (telemetry-parser's orientation string)
};

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.79769313486231570e308; }

__global__ __launch_bounds__(256) void gyro_rates_kernel(GyroRatesParams p) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const double t = p.ts[i];
    const double r[3] = {p.rates[3 * (size_t)i], p.rates[3 * (size_t)i + 1], p.rates[3 * (size_t)i + 2]};
    if (!(finite64(t) && finite64(r[0]) && finite64(r[1]) && finite64(r[2]))) atomicOr(&p.st->bad_input, 1u);
    const int64_t us = (int64_t)(t * 1000000);
    p.us[i] = us;
    double d[4] = {1., 0., 0., 0.};
    if (i > 0) {
        const double tp = p.ts[i - 1];
        if ((int64_t)(tp * 1000000) > us) atomicMin(&p.st->out_of_order, i);
        const double dt = t - tp;
        const double w[3] = {r[p.axis[0]] * p.sign[0] * dt, r[p.axis[1]] * p.sign[1] * dt, r[p.axis[2]] * p.sign[2] * dt};
        rs::gyro_delta(w, d);
    }
    for (int c = 0; c < 4; ++c) p.dq[4 * (size_t)i + c] = d[c];
}

__global__ __launch_bounds__(256) void gyro_order_kernel(const int64_t* ts, const double* quats, uint32_t n, GyroStatus* st) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i > 0 && ts[i - 1] > ts[i]) atomicMin(&st->out_of_order, i);
}

// q_0 = dq_0 (identity), q_i = normalise(dq_i * q_{i-1}) within each segment of `seg` samples (one workgroup of
// kScanThreads per segment); total[b] = the product over segment b (may be null)
constexpr int kScanThreads = 1024;
constexpr uint32_t kScanSegment = 32 * kScanThreads;

__global__ __launch_bounds__(kScanThreads) void gyro_scan_kernel(const double* __restrict__ dq_all, double* __restrict__ q_all, uint32_t n_all,
                                                                 uint32_t seg, double* __restrict__ total) {
    __shared__ double s[kScanThreads][4];
    const uint32_t t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * seg;
    const uint32_t n = n_all - first < seg ? (uint32_t)(n_all - first) : seg;
    const double* dq = dq_all + 4 * first;
    double* q = q_all + 4 * first;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    double acc[4] = {1., 0., 0., 0.};
    for (uint32_t i = lo; i < hi; ++i) {
        const double d[4] = {dq[4 * (size_t)i], dq[4 * (size_t)i + 1], dq[4 * (size_t)i + 2], dq[4 * (size_t)i + 3]};
        rs::quat_mul_norm(d, acc);
    }
    for (int c = 0; c < 4; ++c) s[t][c] = acc[c];
    __syncthreads();
    // inclusive scan of the chunk products; the later chunk multiplies from the left
    for (uint32_t off = 1; off < (uint32_t)kScanThreads; off <<= 1) {
        double a[4] = {1., 0., 0., 0.};
        if (t >= off)
            for (int c = 0; c < 4; ++c) a[c] = s[t - off][c];
        __syncthreads();
        if (t >= off) {
            rs::quat_mul_norm(acc, a); // a <- normalise(acc * a)
            for (int c = 0; c < 4; ++c) { acc[c] = a[c]; s[t][c] = a[c]; }
        }
        __syncthreads();
    }
    double cur[4] = {1., 0., 0., 0.};
    if (t > 0)
        for (int c = 0; c < 4; ++c) cur[c] = s[t - 1][c];
    for (uint32_t i = lo; i < hi; ++i) {
        const double d[4] = {dq[4 * (size_t)i], dq[4 * (size_t)i + 1], dq[4 * (size_t)i + 2], dq[4 * (size_t)i + 3]};
        rs::quat_mul_norm(d, cur);
        for (int c = 0; c < 4; ++c) q[4 * (size_t)i + c] = cur[c];
    }
    if (total && t == kScanThreads - 1)
        for (int c = 0; c < 4; ++c) total[4 * (size_t)blockIdx.x + c] = s[t][c];
}

// q_i <- normalise(q_i * P) for the samples of segment b >= 1, P = product of the segments before it
__global__ __launch_bounds__(256) void gyro_scan_fixup_kernel(double* __restrict__ q, uint32_t n, uint32_t seg, const double* __restrict__ prefix) {
    const uint32_t i = seg + blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* p = prefix + 4 * (size_t)(i / seg - 1);
    double local[4] = {q[4 * (size_t)i], q[4 * (size_t)i + 1], q[4 * (size_t)i + 2], q[4 * (size_t)i + 3]};
    double acc[4] = {p[0], p[1], p[2], p[3]};
    rs::quat_mul_norm(local, acc); // acc <- normalise(local * acc)
    for (int c = 0; c < 4; ++c) q[4 * (size_t)i + c] = acc[c];
}

// ---- conditioning: raw rates -> uniform grid -> zero-phase low-pass -> decimation (gyro_signal_math.hpp) -------------
// Reference: core_support/signal.cpp:3-31 (gyro_lowpass), :53-60 (gyro_decimate), :62-85 (gyro_interpolate) and the
// fixed-rate integration of core_testcode.cpp:26-34.  Runs once per upload; what it leaves ([m / k][3] rates) is what
// every orientation integrates.

// the raw stream's own faults: a non-finite number, a timestamp below the one before it
__global__ __launch_bounds__(256) void gyro_cond_check_kernel(const double* __restrict__ ts, const double* __restrict__ rates, uint32_t n, GyroStatus* st) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double t = ts[i];
    if (!(finite64(t) && finite64(rates[3 * (size_t)i]) && finite64(rates[3 * (size_t)i + 1]) && finite64(rates[3 * (size_t)i + 2])))
        atomicOr(&st->bad_input, 1u);
    if (i > 0 && ts[i - 1] > t) atomicMin(&st->out_of_order, i);
}

// one thread per grid point: the rates at time (first_sample + i) / sr
__global__ __launch_bounds__(256) void gyro_grid_kernel(const double* __restrict__ ts, const double* __restrict__ rates, uint32_t n, double* __restrict__ grid,
                                                        uint32_t m, int64_t first_sample, int32_t sr) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double r[3];
    rs::interp_rate(ts, rates, n, rs::ugrid_time(first_sample + (int64_t)i, sr), r);
    for (int c = 0; c < 3; ++c) grid[3 * (size_t)i + c] = r[c];
}

// One pass of the low-pass (forward, or backward = forward over the reversed array) over in[n][3] -> out[n][3], in != out.
// A workgroup takes a segment of kScanThreads chunks, a thread one chunk of `chunk` samples and all three axes: the chunk
// from the state zero, a scan of the chunk end states with the tabulated powers of the companion matrix, the chunk again
// from its true state in the reference's order of operations.  More than one segment: a first launch with out == nullptr
// leaves every segment's end state from a zero start in seg_state, gyro_lowpass_carry_kernel turns them into the true
// ones, and the launch that writes starts segment b's first chunk from seg_state[b - 1].
struct GyroLowpassParams {
    const double* in;
    double* out;
    double* seg_state; // [segments][3][2]
    uint32_t n, chunk;
    int32_t reverse;
    rs::LowpassCoef k;
    rs::CarryTable tab;
};

__global__ __launch_bounds__(kScanThreads) void gyro_lowpass_kernel(GyroLowpassParams p) {
    __shared__ double s[kScanThreads][6];
    const uint32_t t = threadIdx.x;
    const uint64_t seg = (uint64_t)p.chunk * kScanThreads, first = (uint64_t)blockIdx.x * seg;
    const uint64_t seg_end = first + seg < p.n ? first + seg : p.n;
    const uint64_t lo64 = first + (uint64_t)t * p.chunk < seg_end ? first + (uint64_t)t * p.chunk : seg_end;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + p.chunk < seg_end ? lo64 + p.chunk : seg_end);
    const bool reverse = p.reverse != 0;
    double start[3][2] = {{0., 0.}, {0., 0.}, {0., 0.}};
    if (t == 0 && blockIdx.x > 0 && p.out)
        for (int c = 0; c < 6; ++c) start[c >> 1][c & 1] = p.seg_state[6 * (size_t)(blockIdx.x - 1) + c];
    double st[3][2];
    for (int c = 0; c < 6; ++c) st[c >> 1][c & 1] = start[c >> 1][c & 1];
    rs::lowpass_run(p.k, p.in, nullptr, p.n, reverse, lo, hi, st);
    for (int c = 0; c < 6; ++c) s[t][c] = st[c >> 1][c & 1];
    __syncthreads();
    for (int lvl = 0; lvl < rs::kCarryLevels; ++lvl) {
        const uint32_t off = 1u << lvl;
        double from[3][2] = {{0., 0.}, {0., 0.}, {0., 0.}};
        if (t >= off)
            for (int c = 0; c < 6; ++c) from[c >> 1][c & 1] = s[t - off][c];
        __syncthreads();
        if (t >= off) {
            rs::carry_step(p.tab.p[lvl], from, st);
            for (int c = 0; c < 6; ++c) s[t][c] = st[c >> 1][c & 1];
        }
        __syncthreads();
    }
    if (!p.out) {
        if (t == kScanThreads - 1)
            for (int c = 0; c < 6; ++c) p.seg_state[6 * (size_t)blockIdx.x + c] = s[t][c];
        return;
    }
    if (t > 0)
        for (int c = 0; c < 6; ++c) start[c >> 1][c & 1] = s[t - 1][c];
    rs::lowpass_run(p.k, p.in, p.out, p.n, reverse, lo, hi, start);
}

// seg_state[b] <- seg_state[b] + A^segment seg_state[b - 1], b = 1 .. n_seg-1: a few thousand steps at most, one thread
struct CarryMatrix { double m[4]; };
__global__ void gyro_lowpass_carry_kernel(double* seg_state, uint32_t n_seg, CarryMatrix P) {
    double prev[3][2];
    for (int c = 0; c < 6; ++c) prev[c >> 1][c & 1] = seg_state[c];
    for (uint32_t b = 1; b < n_seg; ++b) {
        double v[3][2];
        for (int c = 0; c < 6; ++c) v[c >> 1][c & 1] = seg_state[6 * (size_t)b + c];
        rs::carry_step(P.m, prev, v);
        for (int c = 0; c < 6; ++c) { seg_state[6 * (size_t)b + c] = v[c >> 1][c & 1]; prev[c >> 1][c & 1] = v[c >> 1][c & 1]; }
    }
}

// signal.cpp:53-60: sample j = sample j k
__global__ __launch_bounds__(256) void gyro_decimate_kernel(const double* __restrict__ in, double* __restrict__ out, uint32_t m_out, uint32_t k) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m_out) return;
    for (int c = 0; c < 3; ++c) out[3 * (size_t)j + c] = in[3 * ((size_t)j * k) + c];
}

// gyro_rates_kernel for the conditioned stream (core_testcode.cpp:28-33): every sample stands for k / sr seconds
struct GyroUniformRatesParams {
    const double* rates; // [n][3] conditioned
    double* dq;          // [n][4] out; identity at 0
    uint32_t n;
    double k, sr;
    int32_t axis[3];
    double sign[3];
};

__global__ __launch_bounds__(256) void gyro_rates_uniform_kernel(GyroUniformRatesParams p) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    double d[4] = {1., 0., 0., 0.};
    if (i > 0) {
        const double r[3] = {p.rates[3 * (size_t)i], p.rates[3 * (size_t)i + 1], p.rates[3 * (size_t)i + 2]};
        const double w[3] = {r[p.axis[0]] * p.sign[0] * p.k / p.sr, r[p.axis[1]] * p.sign[1] * p.k / p.sr, r[p.axis[2]] * p.sign[2] * p.k / p.sr};
        rs::gyro_delta(w, d);
    }
    for (int c = 0; c < 4; ++c) p.dq[4 * (size_t)i + c] = d[c];
}

struct GyroResampleParams {
    const int64_t* ts;   // [n] microseconds
    const double* quats; // [n][4]
    double* knots;       // [m][4] out
    GyroStatus* st;
    uint32_t n, m;
    uint64_t first_sample, sr_hz;
};

__global__ __launch_bounds__(256) void gyro_resample_kernel(GyroResampleParams p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.m) return;
    double out[4];
    if (!rs::resample_knot(p.ts, p.quats, p.n, rs::grid_time_us(p.first_sample + i, p.sr_hz), out)) atomicOr(&p.st->bad_knot, 1u);
    for (int c = 0; c < 4; ++c) p.knots[4 * (size_t)i + c] = out[c];
}

// ---- spline table ---------------------------------------------------------------------------------------
constexpr uint32_t kSplineRun = 32, kSplineWarm = 64, kSplineWarmLong = 576;
// |c'| and |c| are below 8 for knots in [-1, 1]; after kSplineWarm rows the start's share is below 8 x 2.5e-37, which is
// 2e-6 of an ulp of 1e-14 and less of anything larger
constexpr double kSplineCertain = 1e-14;

struct SplineParams {
    const double* knots; // [n][4]
    double* cf;          // [n][4]: forward-sweep values c'
    double* coef64;      // [n][16] out: y[4] b[4] c[4] d[4]
    float* coef32;       // [n][16] out: the same rounded once (PreSync's table)
    uint32_t n;
    rs::SplinePivots piv;
};

// thread = (run of kSplineRun rows, quaternion component)
__global__ __launch_bounds__(256) void spline_forward_kernel(SplineParams p) {
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x;
    const uint32_t comp = tid & 3u, s = (tid >> 2) * kSplineRun;
    if (s >= p.n) return;
    const uint32_t e = s + kSplineRun < p.n ? s + kSplineRun : p.n;
    const double* y = p.knots + comp;
    if (s == 0) p.cf[comp] = 0.0;
    if (e == p.n) p.cf[4 * (size_t)(p.n - 1) + comp] = 0.0;
    const uint32_t last = e < p.n - 1 ? e : p.n - 1; // exclusive
    if ((s > 1 ? s : 1) >= last) return;             // rows 1 .. n-2 carry an equation
    for (uint32_t warm = kSplineWarm;; warm = kSplineWarmLong) {
        uint32_t i = s > warm + 1 ? s - warm : 1;
        const bool from_the_top = i == 1;
        double c_prev = 0.0;                         // c'[0] = 0; elsewhere the warm-up start
        double smallest = 1.0;
        double ym = y[4 * (size_t)(i - 1)], y0 = y[4 * (size_t)i];
        for (; i < last; ++i) {
            const double yp = y[4 * (size_t)(i + 1)];
            c_prev = rs::spline_forward(ym, y0, yp, rs::spline_pivot(p.piv, i - 1), c_prev);
            if (i >= s) {
                p.cf[4 * (size_t)i + comp] = c_prev;
                smallest = fmin(smallest, fabs(c_prev));
            }
            ym = y0;
            y0 = yp;
        }
        if (from_the_top || warm == kSplineWarmLong || smallest >= kSplineCertain) break;
    }
}

__global__ __launch_bounds__(256) void spline_finish_kernel(SplineParams p) {
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x;
    const uint32_t comp = tid & 3u, s = (tid >> 2) * kSplineRun;
    if (s >= p.n) return;
    const uint32_t e = s + kSplineRun < p.n ? s + kSplineRun : p.n;
    const double* y = p.knots + comp;
    const double* cf = p.cf + comp;
    auto put = [&](uint32_t i, double yv, double b, double c, double d) {
        double* r64 = p.coef64 + 16 * (size_t)i + comp;
        float* r32 = p.coef32 + 16 * (size_t)i + comp;
        r64[0] = yv; r64[4] = b; r64[8] = c; r64[12] = d;
        r32[0] = (float)yv; r32[4] = (float)b; r32[8] = (float)c; r32[12] = (float)d;
    };
    if (e == p.n) { // this run owns the last knot: its coefficients continue the segment before it
        const uint32_t l = p.n - 1;
        const double c_lm = l >= 1 ? (l - 1 >= 1 ? rs::spline_backward(cf[4 * (size_t)(l - 1)], rs::spline_pivot(p.piv, l - 1), 0.0) : 0.0) : 0.0;
        double b_prev, d_prev, b, d;
        rs::spline_segment(y[4 * (size_t)(l - 1)], y[4 * (size_t)l], c_lm, 0.0, &b_prev, &d_prev);
        rs::spline_tail(b_prev, d_prev, c_lm, &b, &d);
        put(l, y[4 * (size_t)l], b, 0.0, d);
    }
    for (uint32_t warm = kSplineWarm;; warm = kSplineWarmLong) {
        // c at the row the backward sweep starts from: the last row (zero), or a forward value far enough away
        const uint32_t j = e + warm < p.n - 1 ? e + warm : p.n - 1;
        double c_next = j == p.n - 1 ? 0.0 : cf[4 * (size_t)j];
        double smallest = 1.0;
        // rows j-1 .. s; row 0 is pinned to zero
        for (uint32_t i = j; i-- > s;) {
            const double c_i = i >= 1 ? rs::spline_backward(cf[4 * (size_t)i], rs::spline_pivot(p.piv, i), c_next) : 0.0;
            if (i <= e && i >= 1) smallest = fmin(smallest, fabs(c_i)); // (row e: the c_next of this run's last segment)
            if (i < e && i + 1 < p.n) {
                double b, d;
                rs::spline_segment(y[4 * (size_t)i], y[4 * (size_t)(i + 1)], c_i, c_next, &b, &d);
                put(i, y[4 * (size_t)i], b, c_i, d);
            }
            c_next = c_i;
        }
        if (j == p.n - 1 || warm == kSplineWarmLong || smallest >= kSplineCertain) break;
    }
}

} // namespace
