// yuv.hpp -- 4:2:2 and 4:4:4 frames stabilised in one pass per frame (include/rssync_yuv.h): I422, NV16, I444 and their
// kin in 16-bit containers I210, P210, P216 and I410.  Part of the single HIP translation unit rssync_kernels.hip, after
// kernels/color16.hpp and kernels/resample.hpp, whose arguments (ColorArgs), cameras (color_map), samplers
// (kernels/colorsample.hpp) and counters these use unchanged.  A 4:2:2 chroma plane is halved in x alone: its extent is
// (width >> 1, height), its output's (out_width >> 1, out_height), and its row table is the luma's.  Four thread shapes:
//
//   yuv422_8<NV, F>(A, pos)            one thread per chroma sample of the output.  It finds the chroma position once and
//                                      samples U and V there -- NV16: the result one 16-bit store of the interleaved pair;
//                                      I422: two planes --, then renders the 2 x 1 luma pixels under the sample, one 16-bit
//                                      store.  The grid is the chroma plane's: a wave covers 128 x 1 luma pixels.
//   yuv422_16<SEMI, SHIFT, F>(A, fill_y, fill_uv, pos)
//                                      the same on 16-bit words: SEMI (P210: SHIFT 6, P216) the U V pair one 32-bit store,
//                                      planar (I210) two planes; the luma pair one 32-bit store.
//   yuv444_8<F>(A, pos)                one thread per output pixel: one position, its taps and weights computed once, the
//   yuv444_16<F>(A, fill_y, fill_uv, pos)  three planes sampled there (I410: the words as written, results clamped to 1023
//                                      by the bicubic sampler as I010's are).
//
// F is the sampler (0 bilinear, 1 bicubic) and `pos` the position policy of kernels/color.hpp: luma(f, u, v, &x, &y) and
// chroma(f, u, v, &x, &y).  The bodies know nothing else of the camera, so a camera per frame or a donor loop can bring a
// policy of its own.
//
//   YuvPos<C>                             the constant camera with the 4:2:2 chroma extent
//   yuv422_kernel<C, NV, F>               yuv422_8<NV, F>
//   yuv422_16_kernel<C, SEMI, SHIFT, F>   yuv422_16<SEMI, SHIFT, F>
//   yuv444_kernel<C, F>                   yuv444_8<F>
//   yuv444_16_kernel<C, F>                yuv444_16<F>
//
// A sample whose position is outside is the fill and is counted: ballots of a wave, one atomic per counter and wave that
// has any.  A 4:4:4 frame's second count is its first.  Samples are set without a branch; only the sampler stands under
// the inside test.
#pragma once

namespace {

// the constant camera of a 4:2:2 (and, luma() alone, a 4:4:4) frame
template <int CAMERA>
struct YuvPos {
    const ColorArgs& A;
    __device__ __forceinline__ bool luma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)A.width, (int)A.height);
    }
    __device__ __forceinline__ bool chroma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        color_map<CAMERA>(A.chroma, f, A.height, A.out_width >> 1, A.iterations, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)(A.width >> 1), (int)A.height);
    }
};

// the three counters of a 4:2:2 kernel: bit 0 and 1 of miss_y are the thread's 2 x 1 luma pixels
__device__ __forceinline__ void yuv_count2(const ColorArgs& A, uint32_t f, bool miss_c, uint32_t miss_y) {
    const unsigned long long mc = __ballot(miss_c);
    const uint32_t ny = (uint32_t)__popcll(__ballot(miss_y & 1u)) + (uint32_t)__popcll(__ballot((miss_y >> 1) & 1u));
    if ((threadIdx.x & 63) == 0) {
        if (ny) atomicAdd(A.outside + f, (unsigned long long)ny);
        if (mc) atomicAdd(A.outside_c + f, (unsigned long long)__popcll(mc));
    }
}

// the two counters of a 4:4:4 kernel: every plane has the one position, so both count the same samples
__device__ __forceinline__ void yuv_count444(const ColorArgs& A, uint32_t f, bool filled) {
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) {
        atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
        atomicAdd(A.outside_c + f, (unsigned long long)__popcll(m));
    }
}

template <bool NV16, int FILTER, class POS>
__device__ __forceinline__ void yuv422_8(const ColorArgs& A, const POS& pos) {
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height, ocw = A.out_width >> 1, och = A.out_height;
    bool miss_c = false;
    uint32_t miss_y = 0;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position for U and V
        float x, y;
        bool in = pos.chroma(f, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (in)
            sample_uv8<NV16, FILTER>(color_plane(A, 1, f), A.src_pitch[1], NV16 ? nullptr : color_plane(A, 2, f), A.src_pitch[2], (int)cw,
                                     (int)ch, x, y, &cb, &cr);
        miss_c = !in;
        if (NV16) {
            color_store16(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb | (cr << 8));
        } else {
            A.dst[1][(size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + cu] = (uint8_t)cb;
            A.dst[2][(size_t)f * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + cu] = (uint8_t)cr;
        }
        // the 2 x 1 luma pixels under it
        uint32_t pair = 0;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            in = pos.luma(f, 2 * cu + dx, cv, &x, &y);
            uint32_t val = A.fill & 255u;
            if (in) val = sample_luma8<FILTER>(color_plane(A, 0, f), A.src_pitch[0], (int)A.width, (int)A.height, x, y);
            miss_y |= (uint32_t)!in << dx;
            pair |= val << (8 * dx);
        }
        color_store16(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)cv * A.dst_pitch[0] + 2 * (size_t)cu, pair);
    }
    yuv_count2(A, f, miss_c, miss_y);
}

template <bool SEMI, int SHIFT, int FILTER, class POS>
__device__ __forceinline__ void yuv422_16(const ColorArgs& A, uint32_t fill_y, uint32_t fill_uv, const POS& pos) {
    // the largest sample value: ten bits in P210's container (SHIFT 6) and in I210's planes, sixteen in P216
    constexpr float kMax = (SHIFT == 6 || !SEMI) ? 1023.0f : 65535.0f;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height, ocw = A.out_width >> 1, och = A.out_height;
    bool miss_c = false;
    uint32_t miss_y = 0;
    if (cu < ocw && cv < och) {
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
        uint32_t pair = 0;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            in = pos.luma(f, 2 * cu + dx, cv, &x, &y);
            uint32_t val = fill_y;
            if (in) val = sample_luma16<SHIFT, FILTER>(color_plane(A, 0, f), A.src_pitch[0], (int)A.width, (int)A.height, x, y, kMax);
            miss_y |= (uint32_t)!in << dx;
            pair |= val << (16 * dx);
        }
        color_store32(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)cv * A.dst_pitch[0] + 4 * (size_t)cu, pair);
    }
    yuv_count2(A, f, miss_c, miss_y);
}

// one plane of bytes, the bilinear taps given: rect_sample's byte
__device__ __forceinline__ uint32_t yuv_linear8(const uint8_t* plane, uint64_t pitch, const rs::ColorTaps& t) {
    const uint8_t* p = plane + (size_t)t.y0 * pitch + t.x0;
    return rs::color_blend((float)p[0], (float)p[1], (float)p[pitch], (float)p[pitch + 1], t.fx, t.fy);
}

template <int FILTER, class POS>
__device__ __forceinline__ void yuv444_8(const ColorArgs& A, const POS& pos) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        const bool in = pos.luma(f, u, v, &x, &y);
        uint32_t val[3] = {A.fill & 255u, (A.fill >> 8) & 255u, (A.fill >> 16) & 255u};
        if (in) {
            // the taps and the weights of the position once, for Y, U and V
            if (FILTER == 0) {
                const rs::ColorTaps t = rs::color_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = yuv_linear8(color_plane(A, k, f), A.src_pitch[k], t);
            } else {
                const rs::CubicTaps t = rs::cubic_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = cubic8_sample(color_plane(A, k, f), A.src_pitch[k], t);
            }
        }
        filled = !in;
#pragma unroll
        for (int k = 0; k < 3; ++k) A.dst[k][(size_t)f * A.dst_stride[k] + (size_t)v * A.dst_pitch[k] + u] = (uint8_t)val[k];
    }
    yuv_count444(A, f, filled);
}

template <int FILTER, class POS>
__device__ __forceinline__ void yuv444_16(const ColorArgs& A, uint32_t fill_y, uint32_t fill_uv, const POS& pos) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        const bool in = pos.luma(f, u, v, &x, &y);
        uint32_t val[3] = {fill_y, fill_uv & 0xffffu, fill_uv >> 16};
        if (in) {
            if (FILTER == 0) {
                const rs::ColorTaps t = rs::color_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = color16_sample<0>(color_plane(A, k, f), A.src_pitch[k], t);
            } else {
                const rs::CubicTaps t = rs::cubic_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = rs::cubic_sample16<0>(color_plane(A, k, f), (size_t)A.src_pitch[k], t, 1023.0f);
            }
        }
        filled = !in;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            color_store16(A.dst[k] + (size_t)f * A.dst_stride[k] + (size_t)v * A.dst_pitch[k] + 2 * (size_t)u, val[k]);
    }
    yuv_count444(A, f, filled);
}

template <int CAMERA, bool NV16, int FILTER>
__global__ __launch_bounds__(256) void yuv422_kernel(ColorArgs A) {
    yuv422_8<NV16, FILTER>(A, YuvPos<CAMERA>{A});
}

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__global__ __launch_bounds__(256) void yuv422_16_kernel(ColorArgs A, uint32_t fill_y, uint32_t fill_uv) {
    yuv422_16<SEMI, SHIFT, FILTER>(A, fill_y, fill_uv, YuvPos<CAMERA>{A});
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void yuv444_kernel(ColorArgs A) {
    yuv444_8<FILTER>(A, YuvPos<CAMERA>{A});
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void yuv444_16_kernel(ColorArgs A, uint32_t fill_y, uint32_t fill_uv) {
    yuv444_16<FILTER>(A, fill_y, fill_uv, YuvPos<CAMERA>{A});
}

} // namespace
