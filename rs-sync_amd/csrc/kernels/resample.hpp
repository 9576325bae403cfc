// resample.hpp -- the bicubic siblings of the kernels that write pixels (RSSYNC_FILTER_BICUBIC, include/rssync_stabilize.h).
// Part of the single HIP translation unit rssync_kernels.hip, after kernels/color16.hpp.  The colour ones are the bodies of
// kernels/color.hpp and color16.hpp with the sampler F = 1 and the constant camera: the position, the fills, the packed
// stores and the counters are the bilinear kernels'; the taps are kernels/colorsample.hpp's (80 a thread of a 4:2:0 kernel:
// 16 for U and V together, 16 for each of the 2 x 2 luma pixels) and all arithmetic on them is resample_math.hpp's.
//
//   stabilize_bicubic_kernel<C>        stabilize_kernel<C, false> with cubic8_sample
//   bicubic_yuv_kernel<C, NV>          yuv8<NV, 1> with ColorPos<C>
//   bicubic_rgba_kernel<C>             rgba8<1> with ColorPos<C>
//   bicubic16_yuv_kernel<C, SEMI, SH>  yuv16<SEMI, SH, 1> with ColorPos<C>
//   bicubic16_gray_kernel<C>           gray16<1> with ColorPos<C>
// (names of their own, not color_* / color16_*: the tests count the kernels of those families)
#pragma once

namespace {

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
    yuv8<NV12, 1>(A, ColorPos<CAMERA>{A});
}

template <int CAMERA>
__global__ __launch_bounds__(256) void bicubic_rgba_kernel(ColorArgs A) {
    rgba8<1>(A, ColorPos<CAMERA>{A});
}

template <int CAMERA, bool SEMI, int SHIFT>
__global__ __launch_bounds__(256) void bicubic16_yuv_kernel(ColorArgs A, uint32_t fill_y, uint32_t fill_uv) {
    yuv16<SEMI, SHIFT, 1>(A, fill_y, fill_uv, ColorPos<CAMERA>{A});
}

template <int CAMERA>
__global__ __launch_bounds__(256) void bicubic16_gray_kernel(ColorArgs A, uint32_t fill_y) {
    gray16<1>(A, fill_y, ColorPos<CAMERA>{A});
}

} // namespace
