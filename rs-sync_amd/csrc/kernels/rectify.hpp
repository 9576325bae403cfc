// rectify.hpp -- rolling-shutter rectification of grayscale frames with the synced gyro (include/rssync_rectify.h).
// Part of the single HIP translation unit rssync_kernels.hip (included there, in order).  The arithmetic of every step is
// rectify_math.hpp's; the kernels here only say which thread does which pixel, row or point.
//
//   rectify_rays_kernel    once per (lens, width, height), cached on the context: the unit ray of every output pixel, fp64
//                          (the driver's undistortion, polished to the inverse of the forward model; NaN where the lens
//                          images nothing) stored as float4.
//   rectify_rows_kernel    once per frame, all frames of a chunk in one launch: the rows + 1 matrices
//                          R(q(row time + delay)) R(q_ref)^T from the fp64 spline table, nine fp32 values each.
//   rectify_kernel<MAP>    one thread per output pixel, a workgroup = 64 x 4 pixels: a wave covers one row segment, so its
//                          lanes start from the same two table entries and stay within two or three of them -- the table
//                          reads are broadcasts out of L2 (36 B x rows per frame).  Per pixel: one 16 B ray, `iterations`
//                          x (two entries, lerp, 3 x 3 product, atan2f, degree-4 polynomial, one division), then four byte
//                          gathers and one byte store, coalesced along the row (MAP: the position itself instead, 8 B).
//                          Filled pixels are counted per frame: one ballot per wave, one atomic per wave that has any.
//   rectify_points_kernel  one thread per tracked point, closed form in fp64.
//
// Frames and results are addressed with a pitch and a frame stride: device-resident inputs and outputs are read and
// written in place, host ones through the chunk slots of the launcher.
#pragma once

namespace {

constexpr int kRectTW = 64, kRectTH = 4; // output tile of rectify_kernel (256 threads): one wave per row segment

struct RectRaysArgs {
    rs::Lens lens;
    uint32_t width, height;
    float4* rays;
};

__global__ __launch_bounds__(256) void rectify_rays_kernel(RectRaysArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    if (u >= A.width || v >= A.height) return;
    double ray[3];
    rs::rect_pixel_ray(A.lens, (double)u, (double)v, ray);
    A.rays[(size_t)v * A.width + u] = make_float4((float)ray[0], (float)ray[1], (float)ray[2], 0.0f);
}

struct RectRowsArgs {
    const double* table;   // fp64 spline table, 16 doubles per knot
    const double* times;   // frame times of the chunk's frames
    float* rows_tab;       // [n_frames][rows + 1][9]
    double start, fs, ro, delay, ref_row;
    uint32_t n_knots, rows, n_frames;
};

__global__ __launch_bounds__(256) void rectify_rows_kernel(RectRowsArgs A) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (j > A.rows) return;
    float m[9];
    rs::rect_row_matrix(A.table, (int)A.n_knots, A.start, A.fs, A.ro, A.times[f], (double)A.rows, A.delay, A.ref_row, (double)j, m);
    float* out = A.rows_tab + ((size_t)f * (A.rows + 1) + j) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = m[k];
}

struct RectArgs {
    const float4* rays;
    const float* rows_tab;       // the chunk's tables
    const uint8_t* src;          // frame 0 of the chunk
    uint8_t* dst;
    float2* map;                 // MAP: [height][width] source positions of frame 0
    unsigned long long* outside; // per frame of the chunk: filled pixels
    uint64_t src_pitch, src_stride, dst_pitch, dst_stride;
    rs::RectLensF lens;
    uint32_t width, height;
    int32_t iterations, fill;
};

template <bool MAP>
__global__ __launch_bounds__(256) void rectify_kernel(RectArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const bool live = u < A.width && v < A.height;
    bool filled = false;
    if (live) {
        const float4 r = A.rays[(size_t)v * A.width + u];
        float x, y;
        rs::rect_map_pixel(A.rows_tab + (size_t)f * (A.height + 1) * 9, (int)A.height, A.lens, A.iterations, (float)v, r.x, r.y, r.z, &x, &y);
        if (MAP) {
            A.map[(size_t)v * A.width + u] = make_float2(x, y);
        } else {
            uint8_t val = (uint8_t)A.fill;
            if (rs::rect_inside(x, y, (int)A.width, (int)A.height))
                val = rs::rect_sample(A.src + (size_t)f * A.src_stride, (size_t)A.src_pitch, (int)A.width, (int)A.height, x, y);
            else
                filled = true;
            A.dst[(size_t)f * A.dst_stride + (size_t)v * A.dst_pitch + u] = val;
        }
    }
    if (!MAP) {
        const unsigned long long m = __ballot(filled);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
    }
}

struct RectPointsArgs {
    const double* table;
    const double* points; // [count][2]
    double* out;
    rs::Lens lens;
    double start, fs, frame_time, rows, delay, ref_row;
    uint32_t n_knots;
    uint64_t count;
};

__global__ __launch_bounds__(256) void rectify_points_kernel(RectPointsArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.count) return;
    double ox, oy;
    rs::rect_forward_point(A.table, (int)A.n_knots, A.start, A.fs, A.lens, A.frame_time, A.rows, A.delay, A.ref_row, A.points[2 * i],
                           A.points[2 * i + 1], &ox, &oy);
    A.out[2 * i] = ox;
    A.out[2 * i + 1] = oy;
}

} // namespace
