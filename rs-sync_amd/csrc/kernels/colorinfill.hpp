// colorinfill.hpp -- the borders of colour frames filled from the neighbouring frames of the call
// (include/rssync_colorinfill.h): every format of the colour front but GRAY8, which runs kernels/infill.hpp.  Part of the
// single HIP translation unit rssync_kernels.hip, after kernels/infill.hpp.  A plane is a camera: every plane runs the gray
// infill's procedure -- the candidate order of infill_math.hpp, a row table per candidate, the first candidate that is inside
// -- with the plane's camera of kernels/color.hpp, and the value comes from the samplers of kernels/colorsample.hpp on the
// donor's plane: the bytes are the colour front's.  The kernels have bodies of their own, yuv8's and its siblings' shape
// with a candidate loop where those have one map evaluation (why not the shared bodies: DESIGN.md, "The colour infill").
//
//   donor_rows_kernel                     color_rows_entry with infill_rows_kernel's indirection: the luma and the chroma
//                                         table of every (chunk frame, candidate place) in one launch.  Table (f, k) of a
//                                         plane is rs::stab_row_matrix of the plane's time of f's k-th candidate against the
//                                         target of f; [chunk frame][place][rows + 1][9] per region.
//   donor_yuv8_kernel<C, NV12, F>         yuv8<NV12, F>'s shape: one thread per output chroma sample.  The
//                                         candidate loop for the chroma sample (U and V: one position, one donor), then one
//                                         loop for each of the 2 x 2 luma pixels.  Each ray is formed once, before its loop.
//   donor_yuv16_kernel<C, SEMI, SHIFT, F> yuv16<SEMI, SHIFT, F>'s: P010 <true, 6>, P016 <true, 0>, I010 <false, 0>
//   donor_rgba8_kernel<C, F>              rgba8<F>'s: one position and one donor for the four channels
//   donor_gray16_kernel<C, F>             gray16<F>'s
//
// The steps of the order, the candidate's frame and its table are the same in every lane (blockIdx.z is the frame): they
// stay in scalar registers, and only the lanes still looking are active, as in infill_kernel.  A wave whose samples are all
// inside their own frame at candidate 0 runs every loop body once: the constant camera's work.  The sampler runs once per
// sample after its loop, on the donor's plane.  Stores are the colour front's.  Four counters per frame -- filled and
// borrowed, plane 0 and chroma -- through color_count4 / color_count1.
// (a family name and an argument struct of their own, and an integer FILTER: the tests count the kernels of the other
// families by substrings of their names)
#pragma once

namespace {

struct DonorRowsArgs {
    const double* table;
    const double* times;    // luma frame times of the call's frames
    const double* times_c;  // chroma frame times of the call's frames
    const double* targets;  // [n_frames][4] unit quaternions of the call's frames: one per frame for all planes
    float* rows_tab;        // [chunk frames][2 radius + 1][rows + 1][9]
    float* rows_tab_c;      // [chunk frames][2 radius + 1][rows_c + 1][9]
    double start, fs, ro, delay;
    uint32_t n_knots, rows, rows_c; // rows_c == 0: no chroma plane
    uint32_t f0, n_frames;  // the chunk's first frame, the call's frames
    int32_t radius;
};

__global__ __launch_bounds__(256) void donor_rows_kernel(DonorRowsArgs A) {
    const uint32_t k = blockIdx.y, fl = blockIdx.z;
    const int64_t f = (int64_t)A.f0 + fl;
    const int64_t g = rs::infill_candidate(f, (int64_t)A.n_frames, A.radius, (int)k);
    if (g < 0) return;
    color_rows_entry(A, blockIdx.x * 256 + threadIdx.x, (size_t)g, (size_t)f, (size_t)fl * (2 * A.radius + 1) + k);
}

struct DonorArgs {
    ColorArgs C;                    // the colour kernels': src[k] is frame src0 of the call, dst[k] frame 0 of the chunk, the
                                    // cameras' rows_tab the chunk's tables, 2 radius + 1 places per frame; outside[_c] per
                                    // frame of the chunk
    unsigned long long* borrowed;   // per frame of the chunk: samples of plane 0 that came from another frame
    unsigned long long* borrowed_c; // ... and chroma samples
    uint32_t fill_y, fill_uv;       // 16-bit formats: the fills as stored words
    uint32_t f0, src0, n_frames;    // the chunk's first frame, the frame `src` points at, the call's frames
    int32_t radius;
};

// The candidate loop of output sample (u, v) of chunk frame fl in the plane of camera C (cols x rows, out_cols wide):
// infill_kernel's.  -> the donor and its position, or -1.
template <int CAMERA>
__device__ __forceinline__ int64_t donor_find(const DonorArgs& P, const ColorCam& C, uint32_t fl, uint32_t cols, uint32_t rows,
                                              uint32_t out_cols, uint32_t u, uint32_t v, float* x, float* y) {
    float rx, ry, rz;
    if (CAMERA == 0) {
        const float4 r = C.rays[(size_t)v * out_cols + u];
        rx = r.x; ry = r.y; rz = r.z;
    } else {
        rs::stab_pinhole_ray(C.cam, (float)u, (float)v, &rx, &ry, &rz);
    }
    const float y0 = rs::stab_start_row((float)v, C.y_scale);
    const int64_t f = (int64_t)P.f0 + fl;
    const size_t tab = (size_t)(rows + 1) * 9;
    const float* t = C.rows_tab + (size_t)fl * (2 * P.radius + 1) * tab; // the table of the next candidate
    for (int step = 0; step <= 2 * P.radius; ++step) {
        const int64_t g = rs::infill_step_frame(f, step);
        if (!rs::infill_is_frame(g, (int64_t)P.n_frames)) continue;
        rs::rect_map_pixel(t, (int)rows, C.lens, P.C.iterations, y0, rx, ry, rz, x, y);
        if (rs::rect_inside(*x, *y, (int)cols, (int)rows)) return g;
        t += tab;
    }
    return -1;
}

// plane k of the donor
__device__ __forceinline__ const uint8_t* donor_plane(const DonorArgs& P, int k, int64_t g) {
    return P.C.src[k] + (size_t)(g - (int64_t)P.src0) * P.C.src_stride[k];
}

template <int CAMERA, bool NV12, int FILTER>
__global__ __launch_bounds__(256) void donor_yuv8_kernel(DonorArgs P) {
    const ColorArgs& A = P.C;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, lent_c = false;
    uint32_t fill_y = 0, lent_y = 0;
    if (cu < ocw && cv < och) {
        const int64_t f = (int64_t)P.f0 + fl;
        // the chroma sample: one position and one donor for U and V
        float x, y;
        int64_t g = donor_find<CAMERA>(P, A.chroma, fl, cw, ch, ocw, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (g >= 0) {
            sample_uv8<NV12, FILTER>(donor_plane(P, 1, g), A.src_pitch[1], NV12 ? nullptr : donor_plane(P, 2, g), A.src_pitch[2], (int)cw, (int)ch,
                                    x, y, &cb, &cr);
            lent_c = g != f;
        } else {
            fill_c = true;
        }
        if (NV12) {
            color_store16(A.dst[1] + (size_t)fl * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb | (cr << 8));
        } else {
            A.dst[1][(size_t)fl * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + cu] = (uint8_t)cb;
            A.dst[2][(size_t)fl * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + cu] = (uint8_t)cr;
        }
        // the 2 x 2 luma pixels under it: a donor each
        uint8_t* dst = A.dst[0] + (size_t)fl * A.dst_stride[0] + (size_t)(2 * cv) * A.dst_pitch[0] + 2 * (size_t)cu;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            uint32_t pair = 0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = A.fill & 255u;
                if (g >= 0) {
                    val = sample_luma8<FILTER>(donor_plane(P, 0, g), A.src_pitch[0], (int)A.width, (int)A.height, x, y);
                    if (g != f) lent_y |= 1u << (2 * dy + dx);
                } else {
                    fill_y |= 1u << (2 * dy + dx);
                }
                pair |= val << (8 * dx);
            }
            color_store16(dst + (size_t)dy * A.dst_pitch[0], pair);
        }
    }
    color_count4(A, P.borrowed, P.borrowed_c, fl, fill_c, lent_c, fill_y, lent_y);
}

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__global__ __launch_bounds__(256) void donor_yuv16_kernel(DonorArgs P) {
    // the largest sample value: ten bits in P010's container (SHIFT 6) and in I010's planes, sixteen in P016
    constexpr float kMax = (SHIFT == 6 || !SEMI) ? 1023.0f : 65535.0f;
    const ColorArgs& A = P.C;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, lent_c = false;
    uint32_t fill_y = 0, lent_y = 0;
    if (cu < ocw && cv < och) {
        const int64_t f = (int64_t)P.f0 + fl;
        // the chroma sample: one position and one donor for U and V
        float x, y;
        int64_t g = donor_find<CAMERA>(P, A.chroma, fl, cw, ch, ocw, cu, cv, &x, &y);
        uint32_t cb = P.fill_uv & 0xffffu, cr = P.fill_uv >> 16;
        if (g >= 0) {
            sample_uv16<SEMI, SHIFT, FILTER>(donor_plane(P, 1, g), A.src_pitch[1], SEMI ? nullptr : donor_plane(P, 2, g), A.src_pitch[2], (int)cw,
                                            (int)ch, x, y, kMax, &cb, &cr);
            lent_c = g != f;
        } else {
            fill_c = true;
        }
        if (SEMI) {
            color_store32(A.dst[1] + (size_t)fl * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 4 * (size_t)cu, cb | (cr << 16));
        } else {
            color_store16(A.dst[1] + (size_t)fl * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb);
            color_store16(A.dst[2] + (size_t)fl * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + 2 * (size_t)cu, cr);
        }
        // the 2 x 2 luma pixels under it: a donor each
        uint8_t* dst = A.dst[0] + (size_t)fl * A.dst_stride[0] + (size_t)(2 * cv) * A.dst_pitch[0] + 4 * (size_t)cu;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            uint32_t pair = 0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = P.fill_y;
                if (g >= 0) {
                    val = sample_luma16<SHIFT, FILTER>(donor_plane(P, 0, g), A.src_pitch[0], (int)A.width, (int)A.height, x, y, kMax);
                    if (g != f) lent_y |= 1u << (2 * dy + dx);
                } else {
                    fill_y |= 1u << (2 * dy + dx);
                }
                pair |= val << (16 * dx);
            }
            color_store32(dst + (size_t)dy * A.dst_pitch[0], pair);
        }
    }
    color_count4(A, P.borrowed, P.borrowed_c, fl, fill_c, lent_c, fill_y, lent_y);
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void donor_rgba8_kernel(DonorArgs P) {
    const ColorArgs& A = P.C;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    bool filled = false, lent = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        const int64_t g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, u, v, &x, &y);
        uint32_t px = A.fill;
        if (g >= 0) {
            px = sample_rgba8<FILTER>(donor_plane(P, 0, g), A.src_pitch[0], (int)A.width, (int)A.height, x, y);
            lent = g != (int64_t)P.f0 + fl;
        } else {
            filled = true;
        }
        color_store32(A.dst[0] + (size_t)fl * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 4 * (size_t)u, px);
    }
    color_count1(A, P.borrowed, fl, filled, lent);
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void donor_gray16_kernel(DonorArgs P) {
    const ColorArgs& A = P.C;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    bool filled = false, lent = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        const int64_t g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, u, v, &x, &y);
        uint32_t val = P.fill_y;
        if (g >= 0) {
            val = sample_luma16<0, FILTER>(donor_plane(P, 0, g), A.src_pitch[0], (int)A.width, (int)A.height, x, y, 65535.0f);
            lent = g != (int64_t)P.f0 + fl;
        } else {
            filled = true;
        }
        color_store16(A.dst[0] + (size_t)fl * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 2 * (size_t)u, val);
    }
    color_count1(A, P.borrowed, fl, filled, lent);
}

} // namespace
