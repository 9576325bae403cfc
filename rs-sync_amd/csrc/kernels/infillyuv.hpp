// infillyuv.hpp -- the borders of 4:2:2 and 4:4:4 frames filled from the neighbouring frames of the call
// (include/rssync_infillyuv.h): I422, NV16, I444, I210, P210, P216 and I410.  Part of the single HIP translation unit
// rssync_kernels.hip, after kernels/colorinfill.hpp and kernels/yuv.hpp.  A plane is a camera: every plane runs the gray
// infill's procedure with the plane's camera of kernels/yuv.hpp -- a 4:2:2 chroma plane is halved in x alone, its extent
// (width >> 1, height), its output's (out_width >> 1, out_height), its row tables the luma's -- through the colour infill's
// candidate loop (donor_find, donor_plane of kernels/colorinfill.hpp), and the value comes from the samplers of
// kernels/colorsample.hpp on the donor's plane: the bytes are rssync_yuv_stabilize's.  The kernels have bodies of their
// own, yuv.hpp's thread shapes with a candidate loop where those have one map evaluation: the shared bodies read
// color_plane(A, k, blockIdx.z), and a donor is another frame ("The colour infill").
//
//   lend422_8_kernel<C, NV16, F>          yuv422_8<NV16, F>'s shape: one thread per output chroma sample.  The candidate loop
//                                         for the chroma sample (U and V: one position, one donor), then one loop for each
//                                         of the 2 x 1 luma pixels: three loops.  Each ray is formed once, before its loop.
//   lend422_16_kernel<C, SEMI, SHIFT, F>  yuv422_16<SEMI, SHIFT, F>'s: I210 <false, 0>, P210 <true, 6>, P216 <true, 0>
//   lend444_8_kernel<C, F>                yuv444_8<F>'s: one thread per pixel and one loop; the taps and weights of the
//                                         position once, applied to the three planes of the donor
//   lend444_16_kernel<C, F>               yuv444_16<F>'s: I410, clamped to 1023 by the bicubic sampler
//
// The sampler runs once per sample after its loop, on the donor's plane.  Stores are yuv.hpp's.  A 4:2:2 kernel has four
// counters per frame -- filled and borrowed, luma and chroma --, a 4:4:4 kernel two counts, each written to both entries:
// ballots of a wave, one atomic per counter and wave that has any.
// (a family name and an argument struct of their own: the tests count the kernels of the other families by substrings of
// their names, and a kernel's name holds its argument struct's)
#pragma once

namespace {

struct LendArgs {
    DonorArgs D;
};

// the four counters of a 4:2:2 kernel: bit 0 and 1 of miss_y / lent_y are the thread's 2 x 1 luma pixels
__device__ __forceinline__ void lend_count422(const DonorArgs& P, uint32_t fl, bool miss_c, bool lent_c, uint32_t miss_y, uint32_t lent_y) {
    const unsigned long long mc = __ballot(miss_c), bc = __ballot(lent_c);
    const uint32_t ny = (uint32_t)__popcll(__ballot(miss_y & 1u)) + (uint32_t)__popcll(__ballot((miss_y >> 1) & 1u));
    const uint32_t by = (uint32_t)__popcll(__ballot(lent_y & 1u)) + (uint32_t)__popcll(__ballot((lent_y >> 1) & 1u));
    if ((threadIdx.x & 63) == 0) {
        if (ny) atomicAdd(P.C.outside + fl, (unsigned long long)ny);
        if (mc) atomicAdd(P.C.outside_c + fl, (unsigned long long)__popcll(mc));
        if (by) atomicAdd(P.borrowed + fl, (unsigned long long)by);
        if (bc) atomicAdd(P.borrowed_c + fl, (unsigned long long)__popcll(bc));
    }
}

// the counters of a 4:4:4 kernel: every plane has the one position and the one donor, so both entries count the same samples
__device__ __forceinline__ void lend_count444(const DonorArgs& P, uint32_t fl, bool filled, bool lent) {
    const unsigned long long m = __ballot(filled), b = __ballot(lent);
    if ((threadIdx.x & 63) == 0) {
        if (m) {
            atomicAdd(P.C.outside + fl, (unsigned long long)__popcll(m));
            atomicAdd(P.C.outside_c + fl, (unsigned long long)__popcll(m));
        }
        if (b) {
            atomicAdd(P.borrowed + fl, (unsigned long long)__popcll(b));
            atomicAdd(P.borrowed_c + fl, (unsigned long long)__popcll(b));
        }
    }
}

template <int CAMERA, bool NV16, int FILTER>
__global__ __launch_bounds__(256) void lend422_8_kernel(LendArgs L) {
    const DonorArgs& P = L.D;
    const ColorArgs& A = P.C;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height, ocw = A.out_width >> 1, och = A.out_height;
    bool fill_c = false, lent_c = false;
    uint32_t fill_y = 0, lent_y = 0;
    if (cu < ocw && cv < och) {
        const int64_t f = (int64_t)P.f0 + fl;
        // the chroma sample: one position and one donor for U and V
        float x, y;
        int64_t g = donor_find<CAMERA>(P, A.chroma, fl, cw, ch, ocw, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (g >= 0) {
            sample_uv8<NV16, FILTER>(donor_plane(P, 1, g), A.src_pitch[1], NV16 ? nullptr : donor_plane(P, 2, g), A.src_pitch[2], (int)cw, (int)ch,
                                     x, y, &cb, &cr);
            lent_c = g != f;
        } else {
            fill_c = true;
        }
        if (NV16) {
            color_store16(A.dst[1] + (size_t)fl * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb | (cr << 8));
        } else {
            A.dst[1][(size_t)fl * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + cu] = (uint8_t)cb;
            A.dst[2][(size_t)fl * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + cu] = (uint8_t)cr;
        }
        // the 2 x 1 luma pixels under it: a donor each
        uint32_t pair = 0;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, 2 * cu + dx, cv, &x, &y);
            uint32_t val = A.fill & 255u;
            if (g >= 0) {
                val = sample_luma8<FILTER>(donor_plane(P, 0, g), A.src_pitch[0], (int)A.width, (int)A.height, x, y);
                if (g != f) lent_y |= 1u << dx;
            } else {
                fill_y |= 1u << dx;
            }
            pair |= val << (8 * dx);
        }
        color_store16(A.dst[0] + (size_t)fl * A.dst_stride[0] + (size_t)cv * A.dst_pitch[0] + 2 * (size_t)cu, pair);
    }
    lend_count422(P, fl, fill_c, lent_c, fill_y, lent_y);
}

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__global__ __launch_bounds__(256) void lend422_16_kernel(LendArgs L) {
    // the largest sample value: ten bits in P210's container (SHIFT 6) and in I210's planes, sixteen in P216
    constexpr float kMax = (SHIFT == 6 || !SEMI) ? 1023.0f : 65535.0f;
    const DonorArgs& P = L.D;
    const ColorArgs& A = P.C;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height, ocw = A.out_width >> 1, och = A.out_height;
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
        // the 2 x 1 luma pixels under it: a donor each
        uint32_t pair = 0;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, 2 * cu + dx, cv, &x, &y);
            uint32_t val = P.fill_y;
            if (g >= 0) {
                val = sample_luma16<SHIFT, FILTER>(donor_plane(P, 0, g), A.src_pitch[0], (int)A.width, (int)A.height, x, y, kMax);
                if (g != f) lent_y |= 1u << dx;
            } else {
                fill_y |= 1u << dx;
            }
            pair |= val << (16 * dx);
        }
        color_store32(A.dst[0] + (size_t)fl * A.dst_stride[0] + (size_t)cv * A.dst_pitch[0] + 4 * (size_t)cu, pair);
    }
    lend_count422(P, fl, fill_c, lent_c, fill_y, lent_y);
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void lend444_8_kernel(LendArgs L) {
    const DonorArgs& P = L.D;
    const ColorArgs& A = P.C;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    bool filled = false, lent = false;
    if (u < A.out_width && v < A.out_height) {
        // one position and one donor for Y, U and V
        float x, y;
        const int64_t g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, u, v, &x, &y);
        uint32_t val[3] = {A.fill & 255u, (A.fill >> 8) & 255u, (A.fill >> 16) & 255u};
        if (g >= 0) {
            // the taps and the weights of the position once, for the three planes of the donor
            if (FILTER == 0) {
                const rs::ColorTaps t = rs::color_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = yuv_linear8(donor_plane(P, k, g), A.src_pitch[k], t);
            } else {
                const rs::CubicTaps t = rs::cubic_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = cubic8_sample(donor_plane(P, k, g), A.src_pitch[k], t);
            }
            lent = g != (int64_t)P.f0 + fl;
        } else {
            filled = true;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) A.dst[k][(size_t)fl * A.dst_stride[k] + (size_t)v * A.dst_pitch[k] + u] = (uint8_t)val[k];
    }
    lend_count444(P, fl, filled, lent);
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void lend444_16_kernel(LendArgs L) {
    const DonorArgs& P = L.D;
    const ColorArgs& A = P.C;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t fl = blockIdx.z;
    bool filled = false, lent = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        const int64_t g = donor_find<CAMERA>(P, A.luma, fl, A.width, A.height, A.out_width, u, v, &x, &y);
        uint32_t val[3] = {P.fill_y, P.fill_uv & 0xffffu, P.fill_uv >> 16};
        if (g >= 0) {
            if (FILTER == 0) {
                const rs::ColorTaps t = rs::color_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = color16_sample<0>(donor_plane(P, k, g), A.src_pitch[k], t);
            } else {
                const rs::CubicTaps t = rs::cubic_taps((int)A.width, (int)A.height, x, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) val[k] = rs::cubic_sample16<0>(donor_plane(P, k, g), (size_t)A.src_pitch[k], t, 1023.0f);
            }
            lent = g != (int64_t)P.f0 + fl;
        } else {
            filled = true;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            color_store16(A.dst[k] + (size_t)fl * A.dst_stride[k] + (size_t)v * A.dst_pitch[k] + 2 * (size_t)u, val[k]);
    }
    lend_count444(P, fl, filled, lent);
}

} // namespace
