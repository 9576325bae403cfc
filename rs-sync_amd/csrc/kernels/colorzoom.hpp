// colorzoom.hpp -- colour frames rendered with one zoom per frame (include/rssync_colorzoom.h).  Part of the single HIP
// translation unit rssync_kernels.hip, after kernels/zoom.hpp.  These are the colour kernels of kernels/color.hpp,
// kernels/color16.hpp and kernels/resample.hpp with the output camera of frame blockIdx.z read from an array, as
// zoom_render_kernel is stabilize_kernel with such a camera: the map, the inside test, the taps, the blends, the packed
// stores, the ballots and the atomics are theirs, operation for operation, through the same device functions.
//
//   cams    [chunk frames][4]: luma fx zoom, luma fy zoom, chroma fx zoom, chroma fy zoom -- fp64 products formed by the
//           host exactly as color_api.cpp forms them for a constant zoom (the chroma pair is the luma pair times 0.5: exact)
//   PINHOLE that camera as StabCamF, then stab_pinhole_ray
//   LENS    no cached ray map serves a zoom per frame: rect_pixel_ray in fp64, cast to float, as rectify_rays_kernel fills
//           the cache -- the cache's bits by construction.  The chroma plane uses the chroma camera.  A thread of a 4:2:0
//           kernel evaluates five such rays, one after another, each dead before its sampler starts.
//
//   percam_yuv8_kernel<C, NV12, F>          color_yuv_kernel (F = 0) / bicubic_yuv_kernel (F = 1)
//   percam_rgba8_kernel<C, F>               color_rgba_kernel / bicubic_rgba_kernel
//   percam_yuv16_kernel<C, SEMI, SHIFT, F>  color16_yuv_kernel / bicubic16_yuv_kernel: P010 <true, 6>, P016 <true, 0>, I010 <false, 0>
//   percam_gray16_kernel<C, F>              color16_gray_kernel / bicubic16_gray_kernel
// GRAY8 runs zoom_render_kernel.
// (a family name and an argument struct of their own: the tests count the kernels of the other families by name)
#pragma once

namespace {

struct PercamArgs {
    ColorArgs C;                    // the colour kernels', without the ray maps; the planes' cameras hold cx, cy
    const double* cams;             // [chunk frames][4]
    double cx, cy, cx_c, cy_c;      // LENS: the rest of the luma and of the chroma output camera, fp64
    double k1, k2, k3, k4;
    uint32_t fill_y, fill_uv;       // 16-bit formats: the fills as stored words
};

// The lens camera's three-plane kernels (I420, I010) read their arguments from LDS, not from scalar registers, as
// zoom_fit_kernel does and for its reason: the fp64 constants of five rays and the 100-odd scalar registers of the
// arguments (three planes' pointers, pitches and strides in and out) overflow the scalar file by two registers, which the
// compiler parks in vector lanes ("SGPR spills").  The 408 bytes cost vector registers instead, which these kernels have to
// spare; every value stays the same in all threads.  The two-plane kernels fit as they are.
#define PERCAM_STAGE_IN_LDS(name, args) \
    __shared__ PercamArgs name;         \
    if (threadIdx.x == 0) name = args;  \
    __syncthreads()

// color_map with the plane's camera (fx, fy, cx, cy) of this frame
template <int CAMERA>
__device__ inline void percam_map(const PercamArgs& P, const ColorCam& C, double fx, double fy, double cx, double cy, uint32_t f, uint32_t rows,
                                  uint32_t u, uint32_t v, float* x, float* y) {
    float rx, ry, rz;
    if (CAMERA == 0) {
        double ray[3];
        rs::rect_pixel_ray(rs::Lens{0.0, fx, fy, cx, cy, P.k1, P.k2, P.k3, P.k4}, (double)u, (double)v, ray);
        rx = (float)ray[0]; ry = (float)ray[1]; rz = (float)ray[2];
    } else {
        rs::stab_pinhole_ray(rs::StabCamF{(float)fx, (float)fy, C.cam.cx, C.cam.cy}, (float)u, (float)v, &rx, &ry, &rz);
    }
    rs::rect_map_pixel(C.rows_tab + (size_t)f * (rows + 1) * 9, (int)rows, C.lens, P.C.iterations, rs::stab_start_row((float)v, C.y_scale), rx, ry,
                       rz, x, y);
}

template <int CAMERA, bool NV12, int FILTER>
__device__ __forceinline__ void percam_yuv8_body(const PercamArgs& P) {
    const ColorArgs& A = P.C;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, fill_00 = false, fill_01 = false, fill_10 = false, fill_11 = false;
    if (cu < ocw && cv < och) {
        const double* cam = P.cams + 4 * (size_t)f;
        // the chroma sample: one position for U and V
        float x, y;
        percam_map<CAMERA>(P, A.chroma, cam[2], cam[3], P.cx_c, P.cy_c, f, ch, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (rs::rect_inside(x, y, (int)cw, (int)ch)) {
            if (FILTER == 0) {
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
                percam_map<CAMERA>(P, A.luma, cam[0], cam[1], P.cx, P.cy, f, A.height, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = fill_y;
                const bool in = rs::rect_inside(x, y, (int)A.width, (int)A.height);
                if (in) {
                    if (FILTER == 0) val = rs::rect_sample(src, (size_t)A.src_pitch[0], (int)A.width, (int)A.height, x, y);
                    else val = cubic8_sample(src, A.src_pitch[0], rs::cubic_taps((int)A.width, (int)A.height, x, y));
                }
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

template <int CAMERA, bool NV12, int FILTER>
__global__ __launch_bounds__(256) void percam_yuv8_kernel(PercamArgs args) {
    if constexpr (CAMERA == 0 && !NV12) {
        PERCAM_STAGE_IN_LDS(P, args);
        percam_yuv8_body<CAMERA, NV12, FILTER>(P);
    } else {
        percam_yuv8_body<CAMERA, NV12, FILTER>(args);
    }
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void percam_rgba8_kernel(PercamArgs P) {
    const ColorArgs& A = P.C;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        const double* cam = P.cams + 4 * (size_t)f;
        float x, y;
        percam_map<CAMERA>(P, A.luma, cam[0], cam[1], P.cx, P.cy, f, A.height, u, v, &x, &y);
        uint32_t px = A.fill;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height)) {
            if (FILTER == 0) {
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
            }
        } else {
            filled = true;
        }
        color_store32(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 4 * (size_t)u, px);
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__device__ __forceinline__ void percam_yuv16_body(const PercamArgs& P) {
    // the largest sample value: ten bits in P010's container (SHIFT 6) and in I010's planes, sixteen in P016
    constexpr float kMax = (SHIFT == 6 || !SEMI) ? 1023.0f : 65535.0f;
    const ColorArgs& A = P.C;
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool fill_c = false, fill_00 = false, fill_01 = false, fill_10 = false, fill_11 = false;
    if (cu < ocw && cv < och) {
        const double* cam = P.cams + 4 * (size_t)f;
        // the chroma sample: one position for U and V
        float x, y;
        percam_map<CAMERA>(P, A.chroma, cam[2], cam[3], P.cx_c, P.cy_c, f, ch, cu, cv, &x, &y);
        uint32_t cb = P.fill_uv & 0xffffu, cr = P.fill_uv >> 16;
        if (rs::rect_inside(x, y, (int)cw, (int)ch)) {
            if (FILTER == 0) {
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
                const rs::CubicTaps t = rs::cubic_taps((int)cw, (int)ch, x, y);
                if (SEMI) {
                    cubic16_pairs<SHIFT>(A.src[1] + (size_t)f * A.src_stride[1], A.src_pitch[1], t, kMax, &cb, &cr);
                } else {
                    cb = rs::cubic_sample16<SHIFT>(A.src[1] + (size_t)f * A.src_stride[1], (size_t)A.src_pitch[1], t, kMax);
                    cr = rs::cubic_sample16<SHIFT>(A.src[2] + (size_t)f * A.src_stride[2], (size_t)A.src_pitch[2], t, kMax);
                }
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
                percam_map<CAMERA>(P, A.luma, cam[0], cam[1], P.cx, P.cy, f, A.height, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = P.fill_y;
                const bool in = rs::rect_inside(x, y, (int)A.width, (int)A.height);
                if (in) {
                    if (FILTER == 0) val = color16_sample<SHIFT>(src, A.src_pitch[0], rs::color_taps((int)A.width, (int)A.height, x, y));
                    else val = rs::cubic_sample16<SHIFT>(src, (size_t)A.src_pitch[0], rs::cubic_taps((int)A.width, (int)A.height, x, y), kMax);
                }
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

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__global__ __launch_bounds__(256) void percam_yuv16_kernel(PercamArgs args) {
    if constexpr (CAMERA == 0 && !SEMI) {
        PERCAM_STAGE_IN_LDS(P, args);
        percam_yuv16_body<CAMERA, SEMI, SHIFT, FILTER>(P);
    } else {
        percam_yuv16_body<CAMERA, SEMI, SHIFT, FILTER>(args);
    }
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void percam_gray16_kernel(PercamArgs P) {
    const ColorArgs& A = P.C;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        const double* cam = P.cams + 4 * (size_t)f;
        float x, y;
        percam_map<CAMERA>(P, A.luma, cam[0], cam[1], P.cx, P.cy, f, A.height, u, v, &x, &y);
        uint32_t val = P.fill_y;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height)) {
            const uint8_t* src = A.src[0] + (size_t)f * A.src_stride[0];
            if (FILTER == 0) val = color16_sample<0>(src, A.src_pitch[0], rs::color_taps((int)A.width, (int)A.height, x, y));
            else val = rs::cubic_sample16<0>(src, (size_t)A.src_pitch[0], rs::cubic_taps((int)A.width, (int)A.height, x, y), 65535.0f);
        } else {
            filled = true;
        }
        color_store16(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 2 * (size_t)u, val);
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

#undef PERCAM_STAGE_IN_LDS

} // namespace
