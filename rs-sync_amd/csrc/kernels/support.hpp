// support.hpp -- segment sums, packing kernels (raw records -> packed streams), the re-timing kernel, debug kernels
// Part of the single HIP translation unit rssync_kernels.hip (included there, in order).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// Sums over the frames of a window, in ONE association that does not depend on how many devices
// share the frames: slots are grouped into CHUNKS (the slots of the window whose frame-table index
// falls into the same block of 64; the host builds the plan), a chunk is summed sequentially in
// slot order, and a window is the sequential sum of its chunks in order.  A device that holds only
// part of a window contributes its chunk sums, and whoever adds the chunks in order -- this kernel
// on a single device, the host across several -- gets bit-identical totals.
//   in[r][slot]                 per-slot values of row r (a candidate delay, a line-search trial)
//   idx[j]                      slot of plan position j (NULL = j itself)
//   chunk_off[c] .. [c+1]       plan positions of chunk c
//   win_chunk_off[w] .. [w+1]   chunks of window w
//   chunk_out[r][c], win_out[r][w]
__global__ __launch_bounds__(64) void plan_sum_kernel(const double* __restrict__ in, uint32_t n_cols,
                                                         const uint32_t* __restrict__ idx,
                                                         const uint32_t* __restrict__ chunk_off, uint32_t n_chunks,
                                                         const uint32_t* __restrict__ win_chunk_off, uint32_t n_win,
                                                         double* __restrict__ chunk_out, double* __restrict__ win_out) {
    const uint32_t r = blockIdx.x / n_win, w = blockIdx.x % n_win;
    const uint32_t c0 = win_chunk_off[w], c1 = win_chunk_off[w + 1];
    const double* row = in + (size_t)r * n_cols;
    double* cout = chunk_out + (size_t)r * n_chunks;
    for (uint32_t c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
        double acc = 0.0;
        uint32_t j = chunk_off[c];
        const uint32_t j1 = chunk_off[c + 1];
        for (; j + 8 <= j1; j += 8) { // eight loads in flight, the additions still in slot order
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = row[idx ? idx[j + q] : j + q];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += v[q];
        }
        for (; j < j1; ++j) acc += row[idx ? idx[j] : j];
        cout[c] = acc;
    }
    __syncthreads(); // the chunk sums of this block are visible to its thread 0
    if (threadIdx.x == 0) {
        double acc = 0.0;
        uint32_t c = c0;
        for (; c + 16 <= c1; c += 16) { // sixteen loads in flight, the additions still in chunk order
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = cout[c + q];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc += v[q];
        }
        for (; c < c1; ++c) acc += cout[c];
        win_out[blockIdx.x] = acc;
    }
}

// debug: P (and dP/dd) rows of one frame
struct DebugParams {
    const f4* rays_a;
    const f4* rays_b;
    const FrameRec* frames;
    uint32_t fi;
    const f4* coef;
    int n_knots;
    float fs;
    int32_t kd;
    float fd;
    float* P;
    float* dP;
};

__global__ __launch_bounds__(kBlock) void debug_problem_kernel(DebugParams p) {
    __shared__ f4 s_win[4 * kWinMax];
    const FrameRec fr = p.frames[p.fi];
    Spline sp;
    sp.g = p.coef;
    sp.n = p.n_knots;
    stage_window(sp, s_win, fr.base_knot + (int)floorf(fr.tmin) + p.kd, fr.base_knot + (int)floorf(fr.tmax) + p.kd + 1);
    __syncthreads();
    for (uint32_t row = blockIdx.x * kBlock + threadIdx.x; row < fr.n; row += gridDim.x * kBlock) {
        f3 P, dP;
        if (sp.path == kPathInterior) residual_row<true, kPathInterior>(sp, p.rays_a[fr.off + row], p.rays_b[fr.off + row], fr.base_knot + p.kd, p.fd, P, dP);
        else residual_row<true, kPathGlobal>(sp, p.rays_a[fr.off + row], p.rays_b[fr.off + row], fr.base_knot + p.kd, p.fd, P, dP);
        p.P[3 * row] = P.x; p.P[3 * row + 1] = P.y; p.P[3 * row + 2] = P.z;
        if (p.dP) { p.dP[3 * row] = dP.x * p.fs; p.dP[3 * row + 1] = dP.y * p.fs; p.dP[3 * row + 2] = dP.z * p.fs; }
    }
}

// ---------------------------------------------------------------------------
// Packing kernels: raw records (what SetTrackResult / set_track_pixels staged, fp64) -> the packed
// streams.  One thread per ray pair; the spline parameter offset (ts - start) * fs - base is
// evaluated in fp64 here (core_private.cpp:19-20 without the delay, relative to the frame's base
// knot), written as fp64 for the Sync kernels and rounded once to fp32 for the PreSync kernel.
// Pixel frames run the driver's undistortion first (core_testcode.cpp:63-95,
// 135-158; fp64 = the reference's arithmetic).  HBM: 64 B read + 96 B written per pair.
struct PackParams {
    const double* raw;
    const rship_pack_frame* frames;
    f4* rays_a;
    f4* rays_b;
    double2* q0; // {ax,bx}
    double2* q1; // {ay,by}
    double2* q2; // {az,bz}
    double2* q3; // {ta,tb}
    double start, fs;
    uint32_t* bad;
};

// spline parameter of a pixel's row time relative to the frame's base knot: row_time (core_testcode.cpp:144-145), then
// knot_offset (core_private.cpp:19-20 without the delay).  pack_frames_kernel and retime_pixels_kernel both take a pixel
// frame's ta / tb from here, so that re-timing gives the bits a full repack with the same readout would.
__device__ __forceinline__ double pixel_knot_offset(double ro, double py, double frame_time, double rows, double start, double fs,
                                                   double base) {
    return rs::knot_offset(rs::row_time(ro, py, frame_time, rows), start, fs, base);
}

__global__ __launch_bounds__(kBlock) void pack_frames_kernel(PackParams p) {
    const rship_pack_frame& fr = p.frames[blockIdx.x];
    const uint32_t n = fr.n_rays;
    for (uint32_t row = blockIdx.y * kBlock + threadIdx.x; row < n; row += gridDim.y * kBlock) {
        double ra[3], rb[3], tsa, tsb, ta, tb;
        const double* rec = p.raw + fr.raw_offset;
        if (fr.is_pixels) {
            const double2* src = (const double2*)(rec + 4 * (size_t)row);
            const double2 a = src[0], b = src[1];
            const rs::Lens lens{fr.lens[0], fr.lens[1], fr.lens[2], fr.lens[3], fr.lens[4], fr.lens[5], fr.lens[6], fr.lens[7], fr.lens[8]};
            rs::pixel_to_ray(lens, a.x, a.y, fr.time_a, fr.rows, ra, &tsa);
            rs::pixel_to_ray(lens, b.x, b.y, fr.time_b, fr.rows, rb, &tsb);
            ta = pixel_knot_offset(lens.ro, a.y, fr.time_a, fr.rows, p.start, p.fs, fr.base);
            tb = pixel_knot_offset(lens.ro, b.y, fr.time_b, fr.rows, p.start, p.fs, fr.base);
        } else {
            tsa = rec[row];
            tsb = rec[(size_t)n + row];
            const double* pa = rec + 2 * (size_t)n + 3 * (size_t)row;
            const double* pb = rec + 5 * (size_t)n + 3 * (size_t)row;
            ra[0] = pa[0]; ra[1] = pa[1]; ra[2] = pa[2];
            rb[0] = pb[0]; rb[1] = pb[1]; rb[2] = pb[2];
            ta = rs::knot_offset(tsa, p.start, p.fs, fr.base);
            tb = rs::knot_offset(tsb, p.start, p.fs, fr.base);
        }
        f4 o0, o1;
        o0.x = (float)ra[0]; o0.y = (float)rb[0]; o0.z = (float)ra[1]; o0.w = (float)rb[1];
        o1.x = (float)ra[2]; o1.y = (float)rb[2]; o1.z = (float)ta; o1.w = (float)tb;
        const bool ok = finite_f(o0.x) && finite_f(o0.y) && finite_f(o0.z) && finite_f(o0.w) && finite_f(o1.x) &&
                        finite_f(o1.y) && finite_f(o1.z) && finite_f(o1.w);
        if (!ok) atomicAdd(p.bad, 1u);
        const size_t o = (size_t)fr.ray_offset + row;
        p.rays_a[o] = o0;
        p.rays_b[o] = o1;
        p.q0[o] = double2{ra[0], rb[0]};
        p.q1[o] = double2{ra[1], rb[1]};
        p.q2[o] = double2{ra[2], rb[2]};
        p.q3[o] = double2{ta, tb};
    }
}

// Re-timing kernel: a new readout for the pixel frames without repacking them.  The ray directions do not depend on the
// readout (core_testcode.cpp:147-152); only the row times do (:144-145).  Per pair it reads the two pixel rows y_a, y_b of
// the raw record and rewrites the time parts of the packed streams -- rays_b[o].z / .w (fp32 ta, tb) and q3[o] (fp64
// {ta, tb}) -- with pixel_knot_offset against the base knot of the frame table the launcher has just installed.  One
// thread per pair, as pack_frames_kernel; 16 B read and 24 B written per pair.  Frames set as rays leave at once.
struct RetimeParams {
    const double* raw;
    const rship_pack_frame* pack; // the records of the last rship_pack_frames (raw offset, times, rows)
    const FrameRec* frames;       // the new frame table (base_knot)
    const double* ro;             // [n_frames] readout of each frame
    f4* rays_b;
    double2* q3;
    double start, fs;
};

__global__ __launch_bounds__(kBlock) void retime_pixels_kernel(RetimeParams p) {
    const rship_pack_frame& fr = p.pack[blockIdx.x];
    if (!fr.is_pixels) return;
    const uint32_t n = fr.n_rays;
    const double ro = p.ro[blockIdx.x], base = (double)p.frames[blockIdx.x].base_knot;
    const double* rec = p.raw + fr.raw_offset;
    for (uint32_t row = blockIdx.y * kBlock + threadIdx.x; row < n; row += gridDim.y * kBlock) {
        const double ya = rec[4 * (size_t)row + 1], yb = rec[4 * (size_t)row + 3];
        const double ta = pixel_knot_offset(ro, ya, fr.time_a, fr.rows, p.start, p.fs, base);
        const double tb = pixel_knot_offset(ro, yb, fr.time_b, fr.rows, p.start, p.fs, base);
        const size_t o = (size_t)fr.ray_offset + row;
        ((float2*)(p.rays_b + o))[1] = make_float2((float)ta, (float)tb); // (.x / .y, the z components, stay)
        p.q3[o] = double2{ta, tb};
    }
}

// Re-lens kernel: a new lens for the pixel frames without repacking them (the lens sweep, rssync_c.h: rssync_ext_lens_sweep).
// A lens changes the ray directions as well as the row times, so per pair it reads the whole raw pixel record (32 B, two
// double2) and rewrites ALL packed streams of the pair (96 B) with the arithmetic of pack_frames_kernel's pixel branch --
// rs::pixel_to_ray and pixel_knot_offset, the same text -- against the base knot of the frame table the launcher has just
// installed.  The lens of a frame comes from a device table (9 doubles per frame, uniform across a block).  One thread per
// pair; rays with a non-finite packed value are counted as the packing kernel counts them, reduced within the wave first
// (one atomic per wave that met any).  Frames set as rays leave at once.
struct RelensParams {
    const double* raw;
    const rship_pack_frame* pack; // the records of the last rship_pack_frames (raw offset, times, rows)
    const FrameRec* frames;       // the new frame table (base_knot)
    const double* lens;           // [n_frames][9]: ro, fx, fy, cx, cy, k1 .. k4
    f4* rays_a;
    f4* rays_b;
    double2* q0;
    double2* q1;
    double2* q2;
    double2* q3;
    double start, fs;
    uint32_t* bad; // this launch's counter
};

__global__ __launch_bounds__(kBlock) void relens_pixels_kernel(RelensParams p) {
    const rship_pack_frame& fr = p.pack[blockIdx.x];
    if (!fr.is_pixels) return;
    const uint32_t n = fr.n_rays;
    const double* L = p.lens + 9 * (size_t)blockIdx.x;
    const rs::Lens lens{L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7], L[8]};
    const double base = (double)p.frames[blockIdx.x].base_knot;
    const double* rec = p.raw + fr.raw_offset;
    uint32_t n_bad = 0;
    for (uint32_t row = blockIdx.y * kBlock + threadIdx.x; row < n; row += gridDim.y * kBlock) {
        double ra[3], rb[3], tsa, tsb;
        const double2* src = (const double2*)(rec + 4 * (size_t)row);
        const double2 a = src[0], b = src[1];
        rs::pixel_to_ray(lens, a.x, a.y, fr.time_a, fr.rows, ra, &tsa);
        rs::pixel_to_ray(lens, b.x, b.y, fr.time_b, fr.rows, rb, &tsb);
        const double ta = pixel_knot_offset(lens.ro, a.y, fr.time_a, fr.rows, p.start, p.fs, base);
        const double tb = pixel_knot_offset(lens.ro, b.y, fr.time_b, fr.rows, p.start, p.fs, base);
        f4 o0, o1;
        o0.x = (float)ra[0]; o0.y = (float)rb[0]; o0.z = (float)ra[1]; o0.w = (float)rb[1];
        o1.x = (float)ra[2]; o1.y = (float)rb[2]; o1.z = (float)ta; o1.w = (float)tb;
        const bool ok = finite_f(o0.x) && finite_f(o0.y) && finite_f(o0.z) && finite_f(o0.w) && finite_f(o1.x) &&
                        finite_f(o1.y) && finite_f(o1.z) && finite_f(o1.w);
        n_bad += ok ? 0u : 1u;
        const size_t o = (size_t)fr.ray_offset + row;
        p.rays_a[o] = o0;
        p.rays_b[o] = o1;
        p.q0[o] = double2{ra[0], rb[0]};
        p.q1[o] = double2{ra[1], rb[1]};
        p.q2[o] = double2{ra[2], rb[2]};
        p.q3[o] = double2{ta, tb};
    }
    // (every thread of the block gets here: the early return above is uniform across it)
    n_bad = wave_sum_u32(n_bad);
    if (n_bad && (threadIdx.x & 63) == 0) atomicAdd(p.bad, n_bad);
}

// debug: the wave-level exact selection on caller-provided residuals (one wave per problem,
// 2048 slots, NaN-padded), exactly as the LMedS kernel drives it
__global__ __launch_bounds__(64) void debug_select_kernel(const float* __restrict__ vals, uint32_t n, uint32_t kq,
                                                          const float* __restrict__ upper, uint32_t* out) {
    constexpr int NR = 32;
    const int lane = threadIdx.x;
    const float* v = vals + (size_t)blockIdx.x * n;
    uint32_t r2[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
        uint32_t i = m * 64 + lane;
        r2[m] = (i < n) ? __float_as_uint(v[i]) : 0x7fc00000u;
    }
    uint32_t hi2 = upper ? __float_as_uint(upper[blockIdx.x]) : kInfBits;
    const uint32_t tot = wave_count_lt(r2, hi2);
    uint32_t res = 0xffffffffu; // "not better than the bound"
    if (tot > kq) {
        if (hi2 == kInfBits) {
            float mx = 0.f;
#pragma unroll
            for (int m = 0; m < NR; ++m) mx = fmaxf(mx, fabsf(__uint_as_float(r2[m])));
            mx = wave_max_f32(mx);
            if (finite_f(mx)) hi2 = __float_as_uint(mx) + 1u;
        }
        res = select_kth(r2, kq, hi2, tot);
    }
    if (lane == 0) {
        out[2 * blockIdx.x] = res;
        out[2 * blockIdx.x + 1] = tot;
    }
}

} // namespace
