// resample.hpp -- the bicubic siblings of the kernels that write pixels (RSSYNC_FILTER_BICUBIC, include/rssync_stabilize.h):
// Part of the single HIP translation unit rssync_kernels.hip, after kernels/color16.hpp.  The bilinear kernels stay as
// they are, text and bits; these differ from them in the sampler alone -- the map, the inside test, the fills, the packed
// stores and the counters are theirs -- and all arithmetic on the taps is resample_math.hpp's.
//
//   stabilize_bicubic_kernel<C>        stabilize_kernel<C, false>
//   bicubic_yuv_kernel<C, NV>          color_yuv_kernel: one thread per chroma sample, the chroma map once, 16 taps for U
//                                      and V together (NV12: every tap one 16-bit load of the pair), then the 2 x 2 luma
//                                      pixels, 16 taps each: 80 taps a thread
//   bicubic_rgba_kernel<C>             color_rgba_kernel: every tap one 32-bit load, four channels on one set of weights
//   bicubic16_yuv_kernel<C, SEMI, SH>  color16_yuv_kernel (SEMI: every chroma tap one 32-bit load of the U V pair)
//   bicubic16_gray_kernel<C>           color16_gray_kernel
// (names of their own, not color_* / color16_*: the tests count the kernels of those families)
//
// Taps are per-thread loads through four clamped column offsets and four clamped row pointers, each computed once per
// position, not an LDS tile ("Bicubic taps").  One path for every inside pixel: the clamps are two instructions
// per offset, and one path means one set of bits.  The blends run row by row -- a row's four taps become one float per
// channel before the next row is touched -- so a position holds four floats per channel, and no kernel needs scratch.
#pragma once

namespace {

// one plane of bytes, the taps given
__device__ inline uint32_t cubic8_sample(const uint8_t* plane, uint64_t pitch, const rs::CubicTaps& t) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = plane + (size_t)t.y[j] * pitch;
        r[j] = rs::cubic_row((float)p[t.x[0]], (float)p[t.x[1]], (float)p[t.x[2]], (float)p[t.x[3]], t.wx);
    }
    return rs::cubic_finish(r[0], r[1], r[2], r[3], t.wy, 255.0f);
}

// a plane of pairs of 16-bit words (P010 / P016 chroma), every tap one 32-bit load -> the two results' stored words
template <int SHIFT>
__device__ inline void cubic16_pairs(const uint8_t* plane, uint64_t pitch, const rs::CubicTaps& t, float vmax, uint32_t* lo, uint32_t* hi) {
    float a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = plane + (size_t)t.y[j] * pitch;
        const uint32_t p0 = color_load32(p + 4 * (size_t)t.x[0]), p1 = color_load32(p + 4 * (size_t)t.x[1]);
        const uint32_t p2 = color_load32(p + 4 * (size_t)t.x[2]), p3 = color_load32(p + 4 * (size_t)t.x[3]);
        a[j] = rs::cubic_row((float)((p0 & 0xffffu) >> SHIFT), (float)((p1 & 0xffffu) >> SHIFT), (float)((p2 & 0xffffu) >> SHIFT),
                             (float)((p3 & 0xffffu) >> SHIFT), t.wx);
        b[j] = rs::cubic_row((float)(p0 >> (16 + SHIFT)), (float)(p1 >> (16 + SHIFT)), (float)(p2 >> (16 + SHIFT)), (float)(p3 >> (16 + SHIFT)),
                             t.wx);
    }
    *lo = rs::cubic_finish(a[0], a[1], a[2], a[3], t.wy, vmax) << SHIFT;
    *hi = rs::cubic_finish(b[0], b[1], b[2], b[3], t.wy, vmax) << SHIFT;
}

template <int CAMERA>
__global__ __launch_bounds__(256) void stabilize_bicubic_kernel(StabArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float rx, ry, rz;
        if (CAMERA == 0) {
            const float4 r = A.rays[(size_t)v * A.out_width + u];
            rx = r.x; ry = r.y; rz = r.z;
        } else {
            rs::stab_pinhole_ray(A.cam, (float)u, (float)v, &rx, &ry, &rz);
        }
        float x, y;
        rs::rect_map_pixel(A.rows_tab + (size_t)f * (A.height + 1) * 9, (int)A.height, A.lens, A.iterations,
                           rs::stab_start_row((float)v, A.y_scale), rx, ry, rz, &x, &y);
        uint32_t val = (uint32_t)A.fill;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height))
            val = cubic8_sample(A.src + (size_t)f * A.src_stride, A.src_pitch, rs::cubic_taps((int)A.width, (int)A.height, x, y));
        else
            filled = true;
        A.dst[(size_t)f * A.dst_stride + (size_t)v * A.dst_pitch + u] = (uint8_t)val;
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

template <int CAMERA, bool NV12>
__global__ __launch_bounds__(256) void bicubic_yuv_kernel(ColorArgs A) {
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, fill_00 = false, fill_01 = false, fill_10 = false, fill_11 = false;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position, one set of weights for U and V
        float x, y;
        color_map<CAMERA>(A.chroma, f, ch, ocw, A.iterations, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (rs::rect_inside(x, y, (int)cw, (int)ch)) {
            const rs::CubicTaps t = rs::cubic_taps((int)cw, (int)ch, x, y);
            if (NV12) {
                const uint8_t* plane = A.src[1] + (size_t)f * A.src_stride[1];
                float a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t* p = plane + (size_t)t.y[j] * A.src_pitch[1];
                    const uint32_t p0 = color_load16(p + 2 * (size_t)t.x[0]), p1 = color_load16(p + 2 * (size_t)t.x[1]);
                    const uint32_t p2 = color_load16(p + 2 * (size_t)t.x[2]), p3 = color_load16(p + 2 * (size_t)t.x[3]);
                    a[j] = rs::cubic_row((float)(p0 & 255u), (float)(p1 & 255u), (float)(p2 & 255u), (float)(p3 & 255u), t.wx);
                    b[j] = rs::cubic_row((float)(p0 >> 8), (float)(p1 >> 8), (float)(p2 >> 8), (float)(p3 >> 8), t.wx);
                }
                cb = rs::cubic_finish(a[0], a[1], a[2], a[3], t.wy, 255.0f);
                cr = rs::cubic_finish(b[0], b[1], b[2], b[3], t.wy, 255.0f);
            } else {
                cb = cubic8_sample(A.src[1] + (size_t)f * A.src_stride[1], A.src_pitch[1], t);
                cr = cubic8_sample(A.src[2] + (size_t)f * A.src_stride[2], A.src_pitch[2], t);
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
                if (in) val = cubic8_sample(src, A.src_pitch[0], rs::cubic_taps((int)A.width, (int)A.height, x, y));
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
__global__ __launch_bounds__(256) void bicubic_rgba_kernel(ColorArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, u, v, &x, &y);
        uint32_t px = A.fill;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height)) {
            const rs::CubicTaps t = rs::cubic_taps((int)A.width, (int)A.height, x, y);
            const uint8_t* plane = A.src[0] + (size_t)f * A.src_stride[0];
            float r[4][4]; // [channel][row]
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t* p = plane + (size_t)t.y[j] * A.src_pitch[0];
                const uint32_t p0 = color_load32(p + 4 * (size_t)t.x[0]), p1 = color_load32(p + 4 * (size_t)t.x[1]);
                const uint32_t p2 = color_load32(p + 4 * (size_t)t.x[2]), p3 = color_load32(p + 4 * (size_t)t.x[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int s = 8 * k;
                    r[k][j] = rs::cubic_row((float)((p0 >> s) & 255u), (float)((p1 >> s) & 255u), (float)((p2 >> s) & 255u),
                                            (float)((p3 >> s) & 255u), t.wx);
                }
            }
            px = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) px |= rs::cubic_finish(r[k][0], r[k][1], r[k][2], r[k][3], t.wy, 255.0f) << (8 * k);
        } else {
            filled = true;
        }
        color_store32(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 4 * (size_t)u, px);
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

template <int CAMERA, bool SEMI, int SHIFT>
__global__ __launch_bounds__(256) void bicubic16_yuv_kernel(ColorArgs A, uint32_t fill_y, uint32_t fill_uv) {
    // the largest sample value: ten bits in P010's container (SHIFT 6) and in I010's planes, sixteen in P016
    constexpr float kMax = (SHIFT == 6 || !SEMI) ? 1023.0f : 65535.0f;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, fill_00 = false, fill_01 = false, fill_10 = false, fill_11 = false;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position, one set of weights for U and V
        float x, y;
        color_map<CAMERA>(A.chroma, f, ch, ocw, A.iterations, cu, cv, &x, &y);
        uint32_t cb = fill_uv & 0xffffu, cr = fill_uv >> 16;
        if (rs::rect_inside(x, y, (int)cw, (int)ch)) {
            const rs::CubicTaps t = rs::cubic_taps((int)cw, (int)ch, x, y);
            if (SEMI) {
                cubic16_pairs<SHIFT>(A.src[1] + (size_t)f * A.src_stride[1], A.src_pitch[1], t, kMax, &cb, &cr);
            } else {
                cb = rs::cubic_sample16<SHIFT>(A.src[1] + (size_t)f * A.src_stride[1], (size_t)A.src_pitch[1], t, kMax);
                cr = rs::cubic_sample16<SHIFT>(A.src[2] + (size_t)f * A.src_stride[2], (size_t)A.src_pitch[2], t, kMax);
            }
        } else {
            fill_c = true;
        }
        if (SEMI) {
            color_store32(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 4 * (size_t)cu, cb | (cr << 16));
        } else {
            color_store16(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb);
            color_store16(A.dst[2] + (size_t)f * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + 2 * (size_t)cu, cr);
        }
        // the 2 x 2 luma pixels under it
        const uint8_t* src = A.src[0] + (size_t)f * A.src_stride[0];
        uint8_t* dst = A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)(2 * cv) * A.dst_pitch[0] + 4 * (size_t)cu;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            uint32_t pair = 0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = fill_y;
                const bool in = rs::rect_inside(x, y, (int)A.width, (int)A.height);
                if (in) val = rs::cubic_sample16<SHIFT>(src, (size_t)A.src_pitch[0], rs::cubic_taps((int)A.width, (int)A.height, x, y), kMax);
                if (dy == 0 && dx == 0) fill_00 = !in;
                if (dy == 0 && dx == 1) fill_01 = !in;
                if (dy == 1 && dx == 0) fill_10 = !in;
                if (dy == 1 && dx == 1) fill_11 = !in;
                pair |= val << (16 * dx);
            }
            color_store32(dst + (size_t)dy * A.dst_pitch[0], pair);
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
__global__ __launch_bounds__(256) void bicubic16_gray_kernel(ColorArgs A, uint32_t fill_y) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, u, v, &x, &y);
        uint32_t val = fill_y;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height))
            val = rs::cubic_sample16<0>(A.src[0] + (size_t)f * A.src_stride[0], (size_t)A.src_pitch[0],
                                        rs::cubic_taps((int)A.width, (int)A.height, x, y), 65535.0f);
        else
            filled = true;
        color_store16(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 2 * (size_t)u, val);
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

} // namespace
