// color16.hpp -- colour frames in 16-bit containers (include/rssync_color16.h): GRAY16, P010, P016 and I010.  Part of the
// single HIP translation unit rssync_kernels.hip, after kernels/color.hpp, whose arguments (ColorArgs: pitches and strides
// in bytes), cameras, position policies and counters these use unchanged; the sample is a native uint16 word, for P010 with
// the value in its ten high bits (color_math.hpp).  This file holds the two 16-bit thread shapes of every colour family:
//
//   yuv16<SEMI, SHIFT, F>(A, fill_y, fill_uv, pos)  yuv8's shape: one thread per chroma sample of the output, the chroma
//                                       position once, then the 2 x 2 luma pixels.  SEMI (P010, P016): the chroma result
//                                       one 32-bit store of the U V pair; planar (I010): two planes of 16-bit words.  Two
//                                       adjacent luma samples of a row go out as one 32-bit store.  SHIFT 6 is P010's
//                                       container, 0 everything else.
//   gray16<F>(A, fill_y, pos)           one thread per output pixel, one 16-bit store.
//   color16_yuv_kernel<C, SEMI, SHIFT>  yuv16<SEMI, SHIFT, 0> with ColorPos<C>
//   color16_gray_kernel<C>              gray16<0> with ColorPos<C>
//
// Rows and pointers are 2-byte aligned and no more: the 32-bit accesses are color_load32 / color_store32, byte copies of
// that width.  The fills arrive as stored words (P010's shifted).
#pragma once

namespace {

template <bool SEMI, int SHIFT, int FILTER, class POS>
__device__ __forceinline__ void yuv16(const ColorArgs& A, uint32_t fill_y, uint32_t fill_uv, const POS& pos) {
    // the largest sample value: ten bits in P010's container (SHIFT 6) and in I010's planes, sixteen in P016
    constexpr float kMax = (SHIFT == 6 || !SEMI) ? 1023.0f : 65535.0f;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool miss_c = false;
    uint32_t miss_y = 0;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position for U and V
        float x, y;
        bool in = pos.chroma(f, cu, cv, &x, &y);
        uint32_t cb = fill_uv & 0xffffu, cr = fill_uv >> 16;
        if (in)
            sample_uv16<SEMI, SHIFT, FILTER>(color_plane(A, 1, f), A.src_pitch[1], SEMI ? nullptr : color_plane(A, 2, f), A.src_pitch[2],
                                             (int)cw, (int)ch, x, y, kMax, &cb, &cr);
        miss_c = !in;
        if (SEMI) {
            color_store32(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 4 * (size_t)cu, cb | (cr << 16));
        } else {
            color_store16(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb);
            color_store16(A.dst[2] + (size_t)f * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + 2 * (size_t)cu, cr);
        }
        // the 2 x 2 luma pixels under it
        uint8_t* dst = A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)(2 * cv) * A.dst_pitch[0] + 4 * (size_t)cu;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            uint32_t pair = 0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                in = pos.luma(f, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = fill_y;
                if (in) val = sample_luma16<SHIFT, FILTER>(color_plane(A, 0, f), A.src_pitch[0], (int)A.width, (int)A.height, x, y, kMax);
                miss_y |= (uint32_t)!in << (2 * dy + dx);
                pair |= val << (16 * dx);
            }
            color_store32(dst + (size_t)dy * A.dst_pitch[0], pair);
        }
    }
    color_count4(A, nullptr, nullptr, f, miss_c, false, miss_y, 0);
}

template <int FILTER, class POS>
__device__ __forceinline__ void gray16(const ColorArgs& A, uint32_t fill_y, const POS& pos) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        uint32_t val = fill_y;
        if (pos.luma(f, u, v, &x, &y))
            val = sample_luma16<0, FILTER>(color_plane(A, 0, f), A.src_pitch[0], (int)A.width, (int)A.height, x, y, 65535.0f);
        else
            filled = true;
        color_store16(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 2 * (size_t)u, val);
    }
    color_count1(A, nullptr, f, filled, false);
}

template <int CAMERA, bool SEMI, int SHIFT>
__global__ __launch_bounds__(256) void color16_yuv_kernel(ColorArgs A, uint32_t fill_y, uint32_t fill_uv) {
    yuv16<SEMI, SHIFT, 0>(A, fill_y, fill_uv, ColorPos<CAMERA>{A});
}

template <int CAMERA>
__global__ __launch_bounds__(256) void color16_gray_kernel(ColorArgs A, uint32_t fill_y) {
    gray16<0>(A, fill_y, ColorPos<CAMERA>{A});
}

} // namespace
