// colorzoom.hpp -- colour frames rendered with one zoom per frame (include/rssync_colorzoom.h).  Part of the single HIP
// translation unit rssync_kernels.hip, after kernels/zoom.hpp.  This file holds one position policy, PercamPos: the bodies
// of kernels/color.hpp and kernels/color16.hpp with the output camera of frame blockIdx.z read from an array, as
// zoom_render_kernel is stabilize_kernel with such a camera.  The inside test's answer, the taps, the blends, the packed
// stores, the ballots and the atomics are the bodies', the same text the constant-camera families run.
//
//   cams    [chunk frames][4]: luma fx zoom, luma fy zoom, chroma fx zoom, chroma fy zoom -- fp64 products formed by the
//           host exactly as color_api.cpp forms them for a constant zoom (the chroma pair is the luma pair times 0.5: exact)
//   PINHOLE that camera as StabCamF, then stab_pinhole_ray
//   LENS    no cached ray map serves a zoom per frame: rect_pixel_ray in fp64, cast to float, as rectify_rays_kernel fills
//           the cache -- the cache's bits by construction.  The chroma plane uses the chroma camera.  A thread of a 4:2:0
//           kernel evaluates five such rays, one after another, each dead before its sampler starts.
//
//   percam_yuv8_kernel<C, NV12, F>          yuv8<NV12, F> with PercamPos<C>: color_yuv_kernel's (F = 0) / bicubic_yuv_kernel's (F = 1) sibling
//   percam_rgba8_kernel<C, F>               rgba8<F>: color_rgba_kernel's / bicubic_rgba_kernel's
//   percam_yuv16_kernel<C, SEMI, SHIFT, F>  yuv16<SEMI, SHIFT, F>: P010 <true, 6>, P016 <true, 0>, I010 <false, 0>
//   percam_gray16_kernel<C, F>              gray16<F>
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
// arguments (three planes' pointers, pitches and strides in and out) overflow the scalar file by four (I010) to ten (I420)
// registers, which the compiler parks in vector lanes ("SGPR spills").  The 408 bytes cost vector registers instead
// (82 - 85 against 61 - 66), which these kernels have to spare; every value stays the same in all threads.  The two-plane
// kernels fit as they are.  (The figures without staging: this file compiled with both `if constexpr` conditions below set to
// false, read from the code object's notes as tests/test_colorzoom_cpu.py reads them.)
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

// the camera of frame f from P.cams
template <int CAMERA>
struct PercamPos {
    const PercamArgs& P;
    __device__ __forceinline__ bool luma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        const double* cam = P.cams + 4 * (size_t)f;
        percam_map<CAMERA>(P, P.C.luma, cam[0], cam[1], P.cx, P.cy, f, P.C.height, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)P.C.width, (int)P.C.height);
    }
    __device__ __forceinline__ bool chroma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        const double* cam = P.cams + 4 * (size_t)f;
        percam_map<CAMERA>(P, P.C.chroma, cam[2], cam[3], P.cx_c, P.cy_c, f, P.C.height >> 1, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)(P.C.width >> 1), (int)(P.C.height >> 1));
    }
};

template <int CAMERA, bool NV12, int FILTER>
__global__ __launch_bounds__(256) void percam_yuv8_kernel(PercamArgs args) {
    if constexpr (CAMERA == 0 && !NV12) {
        PERCAM_STAGE_IN_LDS(P, args);
        yuv8<NV12, FILTER>(P.C, PercamPos<CAMERA>{P});
    } else {
        yuv8<NV12, FILTER>(args.C, PercamPos<CAMERA>{args});
    }
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void percam_rgba8_kernel(PercamArgs P) {
    rgba8<FILTER>(P.C, PercamPos<CAMERA>{P});
}

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__global__ __launch_bounds__(256) void percam_yuv16_kernel(PercamArgs args) {
    if constexpr (CAMERA == 0 && !SEMI) {
        PERCAM_STAGE_IN_LDS(P, args);
        yuv16<SEMI, SHIFT, FILTER>(P.C, P.fill_y, P.fill_uv, PercamPos<CAMERA>{P});
    } else {
        yuv16<SEMI, SHIFT, FILTER>(args.C, args.fill_y, args.fill_uv, PercamPos<CAMERA>{args});
    }
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void percam_gray16_kernel(PercamArgs P) {
    gray16<FILTER>(P.C, P.fill_y, PercamPos<CAMERA>{P});
}

#undef PERCAM_STAGE_IN_LDS

} // namespace
