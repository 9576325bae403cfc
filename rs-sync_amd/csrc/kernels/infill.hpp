// infill.hpp -- the stabiliser's borders filled from the neighbouring frames of the call (include/rssync_infill.h).  Part
// of the single HIP translation unit rssync_kernels.hip, after kernels/resample.hpp: the ray, the map, the inside rule and
// both samplers are the stabiliser's, called here; what is new is the order of the candidates (infill_math.hpp).
//
//   infill_rows_kernel      stabilize_rows_kernel with an index indirection: table (frame f, candidate k) is
//                           rs::stab_row_matrix of the time of f's k-th candidate against the target of f.  Times and
//                           targets are the call's arrays; nothing is expanded on the host.  A frame at an end of the call
//                           has fewer than 2 radius + 1 candidates: its last table places are never written and never read.
//   infill_kernel<C, F>     stabilize_kernel<C, false> (F = 0) and stabilize_bicubic_kernel<C> (F = 1): their tile, their
//                           thread-to-pixel assignment, their ray, formed once.  Then the candidate loop, per thread: the map
//                           against the candidate's table, and out at the first position that is inside.  The steps of the
//                           order, the candidate's frame and its table are the same in every lane (blockIdx.z is the frame):
//                           they stay in scalar registers, and only the lanes still looking are active.  A wave whose
//                           pixels are all inside at candidate 0 -- nearly every wave -- runs the body once: the work of
//                           stabilize_kernel.  The sampler runs once per pixel after the loop, on the frame that was chosen:
//                           its taps do not sit in the loop.  Two ballots and at most two atomics per wave: the pixels that
//                           got `fill`, and the pixels that came from another frame.
// (names without "stabilize" and with an integer FILTER: the tests count the kernels of those families)
#pragma once

namespace {

struct InfillRowsArgs {
    const double* table;
    const double* times;    // frame times of the call's frames
    const double* targets;  // [n_frames][4] unit quaternions of the call's frames
    float* rows_tab;        // [chunk frames][2 radius + 1][rows + 1][9]
    double start, fs, ro, delay;
    uint32_t n_knots, rows;
    uint32_t f0, n_frames;  // the chunk's first frame, the call's frames
    int32_t radius;
};

__global__ __launch_bounds__(256) void infill_rows_kernel(InfillRowsArgs A) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, fl = blockIdx.z;
    if (j > A.rows) return;
    const int64_t f = (int64_t)A.f0 + fl;
    const int64_t g = rs::infill_candidate(f, (int64_t)A.n_frames, A.radius, (int)k);
    if (g < 0) return;
    const double* t = A.targets + (size_t)f * 4;
    float m[9];
    rs::stab_row_matrix(A.table, (int)A.n_knots, A.start, A.fs, A.ro, A.times[g], (double)A.rows, A.delay, rs::RectQuat{t[0], t[1], t[2], t[3]},
                        (double)j, m);
    float* out = A.rows_tab + (((size_t)fl * (2 * A.radius + 1) + k) * (A.rows + 1) + j) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = m[i];
}

struct InfillArgs {
    const float4* rays;           // LENS: the ray map of the output camera, [out_height][out_width]
    const float* rows_tab;        // the chunk's tables: per frame 2 radius + 1 places of height + 1 entries
    const uint8_t* src;           // frame src0 of the call
    uint8_t* dst;                 // frame 0 of the chunk
    unsigned long long* outside;  // per frame of the chunk: filled pixels
    unsigned long long* borrowed; // per frame of the chunk: pixels of another frame
    uint64_t src_pitch, src_stride, dst_pitch, dst_stride;
    rs::RectLensF lens;           // the input lens
    rs::StabCamF cam;             // PINHOLE: the output camera
    float y_scale;                // (float)height / (float)out_height
    uint32_t width, height, out_width, out_height;
    int32_t iterations, fill;
    uint32_t f0, src0, n_frames;  // the chunk's first frame, the frame `src` points at, the call's frames
    int32_t radius;
};

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void infill_kernel(InfillArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    bool filled = false, lent = false;
    if (u < A.out_width && v < A.out_height) {
        float rx, ry, rz;
        if (CAMERA == 0) {
            const float4 r = A.rays[(size_t)v * A.out_width + u];
            rx = r.x; ry = r.y; rz = r.z;
        } else {
            rs::stab_pinhole_ray(A.cam, (float)u, (float)v, &rx, &ry, &rz);
        }
        const float y0 = rs::stab_start_row((float)v, A.y_scale);
        const int64_t f = (int64_t)A.f0 + fl;
        const size_t tab = (size_t)(A.height + 1) * 9;
        const float* rows = A.rows_tab + (size_t)fl * (2 * A.radius + 1) * tab; // the table of the next candidate
        int64_t donor = -1;
        float x = 0.0f, y = 0.0f;
        for (int step = 0; step <= 2 * A.radius; ++step) {
            const int64_t g = rs::infill_step_frame(f, step);
            if (!rs::infill_is_frame(g, (int64_t)A.n_frames)) continue;
            rs::rect_map_pixel(rows, (int)A.height, A.lens, A.iterations, y0, rx, ry, rz, &x, &y);
            if (rs::rect_inside(x, y, (int)A.width, (int)A.height)) {
                donor = g;
                break;
            }
            rows += tab;
        }
        uint32_t val = (uint32_t)A.fill;
        if (donor >= 0) {
            const uint8_t* src = A.src + (size_t)(donor - (int64_t)A.src0) * A.src_stride;
            if (FILTER == 0) val = rs::rect_sample(src, (size_t)A.src_pitch, (int)A.width, (int)A.height, x, y);
            else val = cubic8_sample(src, A.src_pitch, rs::cubic_taps((int)A.width, (int)A.height, x, y));
            lent = donor != f;
        } else {
            filled = true;
        }
        A.dst[(size_t)fl * A.dst_stride + (size_t)v * A.dst_pitch + u] = (uint8_t)val;
    }
    const unsigned long long m = __ballot(filled), b = __ballot(lent);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(A.outside + fl, (unsigned long long)__popcll(m));
        if (b) atomicAdd(A.borrowed + fl, (unsigned long long)__popcll(b));
    }
}

} // namespace
