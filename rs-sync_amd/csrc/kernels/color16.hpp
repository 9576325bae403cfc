// color16.hpp -- colour frames in 16-bit containers (include/rssync_color16.h): GRAY16, P010, P016 and I010.  Part of the
// single HIP translation unit rssync_kernels.hip, after kernels/color.hpp, whose arguments (ColorArgs: pitches and strides
// in bytes), cameras, map (color_map) and row tables these kernels use unchanged; what is new is the sample: a native
// uint16 word, for P010 with the value in its ten high bits (color_math.hpp).
//
//   color16_yuv_kernel<C, SEMI, SHIFT>  color_yuv_kernel's shape: one thread per chroma sample of the output, the chroma
//                                       map once, then the 2 x 2 luma pixels.  SEMI (P010, P016): every chroma tap one
//                                       32-bit load of the U V pair and the result one 32-bit store; planar (I010): two
//                                       planes of 16-bit words.  Two adjacent luma samples of a row go out as one 32-bit
//                                       store.  SHIFT 6 is P010's container, 0 everything else.
//   color16_gray_kernel<C>              one thread per output pixel, four 16-bit taps, one 16-bit store.
//
// Rows and pointers are 2-byte aligned and no more: the 32-bit accesses are color_load32 / color_store32, byte copies of
// that width.  The fills arrive as stored words (P010's shifted).  Filled samples are counted as color_yuv_kernel counts them.
#pragma once

namespace {

// the four taps of one plane of 16-bit words at an inside position -> the stored word of the result
template <int SHIFT>
__device__ inline uint32_t color16_sample(const uint8_t* plane, uint64_t pitch, const rs::ColorTaps& t) {
    const uint8_t* p = plane + (size_t)t.y0 * pitch + 2 * (size_t)t.x0;
    const uint32_t p00 = color_load16(p) >> SHIFT, p01 = color_load16(p + 2) >> SHIFT;
    const uint32_t p10 = color_load16(p + pitch) >> SHIFT, p11 = color_load16(p + pitch + 2) >> SHIFT;
    return (uint32_t)rs::color_blend16((float)p00, (float)p01, (float)p10, (float)p11, t.fx, t.fy) << SHIFT;
}

template <int CAMERA, bool SEMI, int SHIFT>
__global__ __launch_bounds__(256) void color16_yuv_kernel(ColorArgs A, uint32_t fill_y, uint32_t fill_uv) {
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, fill_00 = false, fill_01 = false, fill_10 = false, fill_11 = false;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position for U and V
        float x, y;
        color_map<CAMERA>(A.chroma, f, ch, ocw, A.iterations, cu, cv, &x, &y);
        uint32_t cb = fill_uv & 0xffffu, cr = fill_uv >> 16;
        if (rs::rect_inside(x, y, (int)cw, (int)ch)) {
            const rs::ColorTaps t = rs::color_taps((int)cw, (int)ch, x, y);
            if (SEMI) {
                const uint8_t* p = A.src[1] + (size_t)f * A.src_stride[1] + (size_t)t.y0 * A.src_pitch[1] + 4 * (size_t)t.x0;
                const uint32_t p00 = color_load32(p), p01 = color_load32(p + 4);
                const uint32_t p10 = color_load32(p + A.src_pitch[1]), p11 = color_load32(p + A.src_pitch[1] + 4);
                cb = (uint32_t)rs::color_blend16((float)((p00 & 0xffffu) >> SHIFT), (float)((p01 & 0xffffu) >> SHIFT),
                                                 (float)((p10 & 0xffffu) >> SHIFT), (float)((p11 & 0xffffu) >> SHIFT), t.fx, t.fy)
                     << SHIFT;
                cr = (uint32_t)rs::color_blend16((float)(p00 >> (16 + SHIFT)), (float)(p01 >> (16 + SHIFT)), (float)(p10 >> (16 + SHIFT)),
                                                 (float)(p11 >> (16 + SHIFT)), t.fx, t.fy)
                     << SHIFT;
            } else {
                cb = color16_sample<SHIFT>(A.src[1] + (size_t)f * A.src_stride[1], A.src_pitch[1], t);
                cr = color16_sample<SHIFT>(A.src[2] + (size_t)f * A.src_stride[2], A.src_pitch[2], t);
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
                if (in) val = color16_sample<SHIFT>(src, A.src_pitch[0], rs::color_taps((int)A.width, (int)A.height, x, y));
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
__global__ __launch_bounds__(256) void color16_gray_kernel(ColorArgs A, uint32_t fill_y) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, u, v, &x, &y);
        uint32_t val = fill_y;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height))
            val = color16_sample<0>(A.src[0] + (size_t)f * A.src_stride[0], A.src_pitch[0], rs::color_taps((int)A.width, (int)A.height, x, y));
        else
            filled = true;
        color_store16(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 2 * (size_t)u, val);
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

} // namespace
