// color.hpp -- colour frames stabilised in one pass per frame (include/rssync_color.h): NV12, I420 and RGBA32.  Part of
// the single HIP translation unit rssync_kernels.hip, after kernels/stabilize.hpp, whose map it evaluates per plane with
// that plane's camera; what is new is in color_math.hpp.  GRAY8 runs stabilize_kernel itself.
//
//   color_rows_kernel        the luma and the chroma row table of every frame of a chunk in one launch: entries
//                            0 .. rows of the luma table, then 0 .. rows_c of the chroma table (stab_row_matrix with the
//                            chroma plane's rows and frame time, against the frame's one target).
//   color_yuv_kernel<C, NV>  one thread per chroma sample of the output.  It evaluates the chroma map once and samples U
//                            and V at that position -- NV12: every tap one 16-bit load of the interleaved pair and the
//                            result one 16-bit store; I420: two planes --, then renders the 2 x 2 luma pixels the sample
//                            covers, two adjacent bytes of a row as one 16-bit store.  A wave covers 128 x 2 luma pixels.
//   color_rgba_kernel<C>     one thread per output pixel: one map evaluation, every tap one 32-bit load, the four channels
//                            blended with the one pair of weights, one 32-bit store.
//
// Rows and pointers of a caller's planes need no alignment: the 16- and 32-bit accesses are byte copies of that width, which
// the target issues as one access whatever the address.  Filled pixels are counted as the stabiliser counts them: ballots
// of a wave, one atomic per counter and wave that has any.
#pragma once

namespace {

struct ColorRowsArgs {
    const double* table;
    const double* times;    // luma frame times of the chunk's frames
    const double* times_c;  // chroma frame times
    const double* targets;  // [n_frames][4] unit quaternions: one per frame for all planes
    float* rows_tab;        // [n_frames][rows + 1][9]
    float* rows_tab_c;      // [n_frames][rows_c + 1][9]
    double start, fs, ro, delay;
    uint32_t n_knots, rows, rows_c, n_frames; // rows_c == 0: no chroma plane
};

__global__ __launch_bounds__(256) void color_rows_kernel(ColorRowsArgs A) {
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const uint32_t f = blockIdx.y;
    const bool chroma = j > A.rows;
    if (chroma) {
        j -= A.rows + 1;
        if (!A.rows_c || j > A.rows_c) return;
    }
    const uint32_t rows = chroma ? A.rows_c : A.rows;
    const double time = chroma ? A.times_c[f] : A.times[f];
    const double* t = A.targets + (size_t)f * 4;
    float m[9];
    rs::stab_row_matrix(A.table, (int)A.n_knots, A.start, A.fs, A.ro, time, (double)rows, A.delay, rs::RectQuat{t[0], t[1], t[2], t[3]},
                        (double)j, m);
    float* out = (chroma ? A.rows_tab_c : A.rows_tab) + ((size_t)f * (rows + 1) + j) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = m[k];
}

// one camera of a colour call: the plane's output camera and input lens
struct ColorCam {
    const float4* rays;     // LENS: the ray map of the plane's output camera, [out rows][out cols]
    const float* rows_tab;  // the chunk's tables of the plane, rows + 1 entries per frame
    rs::RectLensF lens;     // the plane's input lens
    rs::StabCamF cam;       // PINHOLE: the plane's output camera
    float y_scale;          // (float)rows / (float)out rows of the plane
};

struct ColorArgs {
    ColorCam luma, chroma;       // (RGBA32: luma alone)
    const uint8_t* src[3];       // frame 0 of the chunk, per plane
    uint8_t* dst[3];
    uint64_t src_pitch[3], src_stride[3], dst_pitch[3], dst_stride[3];
    unsigned long long* outside;   // per frame of the chunk: filled pixels of plane 0
    unsigned long long* outside_c; // ... and filled chroma samples
    uint32_t width, height, out_width, out_height; // of plane 0
    int32_t iterations;
    uint32_t fill;               // the fill values as bytes: Y, U, V or R, G, B, A from the lowest
};

__device__ inline uint32_t color_load16(const uint8_t* p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}
__device__ inline uint32_t color_load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ inline void color_store16(uint8_t* p, uint32_t v) {
    const uint16_t s = (uint16_t)v;
    __builtin_memcpy(p, &s, 2);
}
__device__ inline void color_store32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// the source position of output pixel (u, v) of frame f in a plane of `rows` rows
template <int CAMERA>
__device__ inline void color_map(const ColorCam& C, uint32_t f, uint32_t rows, uint32_t out_cols, int iterations, uint32_t u, uint32_t v,
                                 float* x, float* y) {
    float rx, ry, rz;
    if (CAMERA == 0) {
        const float4 r = C.rays[(size_t)v * out_cols + u];
        rx = r.x; ry = r.y; rz = r.z;
    } else {
        rs::stab_pinhole_ray(C.cam, (float)u, (float)v, &rx, &ry, &rz);
    }
    rs::rect_map_pixel(C.rows_tab + (size_t)f * (rows + 1) * 9, (int)rows, C.lens, iterations, rs::stab_start_row((float)v, C.y_scale), rx, ry,
                       rz, x, y);
}

template <int CAMERA, bool NV12>
__global__ __launch_bounds__(256) void color_yuv_kernel(ColorArgs A) {
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, fill_00 = false, fill_01 = false, fill_10 = false, fill_11 = false;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position for U and V
        float x, y;
        color_map<CAMERA>(A.chroma, f, ch, ocw, A.iterations, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (rs::rect_inside(x, y, (int)cw, (int)ch)) {
            const rs::ColorTaps t = rs::color_taps((int)cw, (int)ch, x, y);
            if (NV12) {
                const uint8_t* p = A.src[1] + (size_t)f * A.src_stride[1] + (size_t)t.y0 * A.src_pitch[1] + 2 * (size_t)t.x0;
                const uint32_t p00 = color_load16(p), p01 = color_load16(p + 2);
                const uint32_t p10 = color_load16(p + A.src_pitch[1]), p11 = color_load16(p + A.src_pitch[1] + 2);
                cb = rs::color_blend((float)(p00 & 255u), (float)(p01 & 255u), (float)(p10 & 255u), (float)(p11 & 255u), t.fx, t.fy);
                cr = rs::color_blend((float)(p00 >> 8), (float)(p01 >> 8), (float)(p10 >> 8), (float)(p11 >> 8), t.fx, t.fy);
            } else {
                const uint8_t* p = A.src[1] + (size_t)f * A.src_stride[1] + (size_t)t.y0 * A.src_pitch[1] + t.x0;
                const uint8_t* q = A.src[2] + (size_t)f * A.src_stride[2] + (size_t)t.y0 * A.src_pitch[2] + t.x0;
                cb = rs::color_blend((float)p[0], (float)p[1], (float)p[A.src_pitch[1]], (float)p[A.src_pitch[1] + 1], t.fx, t.fy);
                cr = rs::color_blend((float)q[0], (float)q[1], (float)q[A.src_pitch[2]], (float)q[A.src_pitch[2] + 1], t.fx, t.fy);
            }
        } else {
            fill_c = true;
        }
        if (NV12) {
            color_store16(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb | (cr << 8));
        } else {
            A.dst[1][(size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + cu] = (uint8_t)cb;
            A.dst[2][(size_t)f * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + cu] = (uint8_t)cr;
        }
        // the 2 x 2 luma pixels under it
        const uint8_t* src = A.src[0] + (size_t)f * A.src_stride[0];
        uint8_t* dst = A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)(2 * cv) * A.dst_pitch[0] + 2 * (size_t)cu;
        const uint32_t fill_y = A.fill & 255u;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            uint32_t pair = 0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = fill_y;
                const bool in = rs::rect_inside(x, y, (int)A.width, (int)A.height);
                if (in) val = rs::rect_sample(src, (size_t)A.src_pitch[0], (int)A.width, (int)A.height, x, y);
                if (dy == 0 && dx == 0) fill_00 = !in;
                if (dy == 0 && dx == 1) fill_01 = !in;
                if (dy == 1 && dx == 0) fill_10 = !in;
                if (dy == 1 && dx == 1) fill_11 = !in;
                pair |= val << (8 * dx);
            }
            color_store16(dst + (size_t)dy * A.dst_pitch[0], pair);
        }
    }
    const unsigned long long mc = __ballot(fill_c);
    const uint32_t ny = (uint32_t)(__popcll(__ballot(fill_00)) + __popcll(__ballot(fill_01)) + __popcll(__ballot(fill_10)) +
                                   __popcll(__ballot(fill_11)));
    if ((threadIdx.x & 63) == 0) {
        if (ny) atomicAdd(A.outside + f, (unsigned long long)ny);
        if (mc) atomicAdd(A.outside_c + f, (unsigned long long)__popcll(mc));
    }
}

template <int CAMERA>
__global__ __launch_bounds__(256) void color_rgba_kernel(ColorArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, u, v, &x, &y);
        uint32_t px = A.fill;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height)) {
            const rs::ColorTaps t = rs::color_taps((int)A.width, (int)A.height, x, y);
            const uint8_t* p = A.src[0] + (size_t)f * A.src_stride[0] + (size_t)t.y0 * A.src_pitch[0] + 4 * (size_t)t.x0;
            const uint32_t p00 = color_load32(p), p01 = color_load32(p + 4);
            const uint32_t p10 = color_load32(p + A.src_pitch[0]), p11 = color_load32(p + A.src_pitch[0] + 4);
            px = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 8 * k;
                px |= (uint32_t)rs::color_blend((float)((p00 >> s) & 255u), (float)((p01 >> s) & 255u), (float)((p10 >> s) & 255u),
                                                (float)((p11 >> s) & 255u), t.fx, t.fy)
                      << s;
            }
        } else {
            filled = true;
        }
        color_store32(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 4 * (size_t)u, px);
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

} // namespace
