// zoomyuv.hpp -- 4:2:2 and 4:4:4 frames rendered with one zoom per frame (include/rssync_zoomyuv.h).  Part of the single HIP
// translation unit rssync_kernels.hip, after kernels/yuv.hpp and kernels/colorzoom.hpp.  This file holds one position
// policy, FramecamPos: the four bodies of kernels/yuv.hpp with the output camera of frame blockIdx.z read from an array, as
// kernels/colorzoom.hpp runs the 4:2:0 bodies.  It is PercamPos with the 4:2:2 chroma extent -- (width >> 1, height), and
// the luma's row table --; the inside test's answer, the taps, the blends, the packed stores, the ballots and the atomics are
// the bodies', the same text the constant-camera kernels run.
//
//   cams    [chunk frames][4]: luma fx zoom, luma fy zoom, chroma fx, chroma fy -- fp64 products formed by the host exactly
//           as color_host.hpp forms them for a constant zoom (4:2:2: the chroma pair is (luma fx zoom) * 0.5, exact, and
//           luma fy zoom itself; 4:4:4: not read)
//   PINHOLE that camera as StabCamF, then stab_pinhole_ray
//   LENS    rect_pixel_ray in fp64, cast to float, as rectify_rays_kernel fills the cache -- the cache's bits by
//           construction (percam_map).  A thread of a 4:2:2 kernel evaluates three such rays, the chroma sample's and its
//           two luma pixels', one after another, each dead before its sampler starts; a thread of a 4:4:4 kernel one.
//
//   framecam_422_kernel<C, NV, F>              yuv422_8<NV, F> with FramecamPos<C>: NV16 <true>, I422 <false>
//   framecam_422_16_kernel<C, SEMI, SHIFT, F>  yuv422_16<SEMI, SHIFT, F>: P210 <true, 6>, P216 <true, 0>, I210 <false, 0>
//   framecam_444_kernel<C, F>                  yuv444_8<F>: I444
//   framecam_444_16_kernel<C, F>               yuv444_16<F>: I410
// (a family name and an argument struct of their own: the tests count the kernels of the other families by name)
#pragma once

namespace {

// PercamArgs under a name of its own; C.chroma holds the 4:2:2 chroma plane's camera, its row table the luma's
struct FramecamArgs : PercamArgs {};

// The lens camera's three-plane 4:2:2 kernels (I422, I210) read their arguments from LDS, not from scalar registers, for the
// reason kernels/colorzoom.hpp gives: three planes' pointers, pitches and strides in and out beside the fp64 constants of
// three rays overflow the scalar file, and the compiler parks the rest in vector lanes ("SGPR spills").  Without staging
// (this file compiled with the constant below false, the figures read from the code object's notes as
// tests/test_zoomyuv_cpu.py reads them) those kernels have 106 scalar registers and spill ten (I422) and four (I210), with
// 57 - 63 vector registers; staged they have 94, spill none and use 74 - 77 vector registers and 408 bytes of LDS, which
// they have to spare; every value stays the same in all threads.  The two-plane kernels (NV16, P210, P216: 96 scalar
// registers), the one-ray 4:4:4 kernels (I444, I410: 90) and every pinhole kernel (65 - 83) fit as they are.
constexpr bool kFramecamStage = true;

#define FRAMECAM_STAGE_IN_LDS(name, args) \
    __shared__ FramecamArgs name;         \
    if (threadIdx.x == 0) name = args;    \
    __syncthreads()

// the camera of frame f from P.cams, the chroma plane halved in x alone
template <int CAMERA>
struct FramecamPos {
    const PercamArgs& P;
    __device__ __forceinline__ bool luma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        return PercamPos<CAMERA>{P}.luma(f, u, v, x, y);
    }
    __device__ __forceinline__ bool chroma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        const double* cam = P.cams + 4 * (size_t)f;
        percam_map<CAMERA>(P, P.C.chroma, cam[2], cam[3], P.cx_c, P.cy_c, f, P.C.height, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)(P.C.width >> 1), (int)P.C.height);
    }
};

template <int CAMERA, bool NV16, int FILTER>
__global__ __launch_bounds__(256) void framecam_422_kernel(FramecamArgs args) {
    if constexpr (kFramecamStage && CAMERA == 0 && !NV16) {
        FRAMECAM_STAGE_IN_LDS(P, args);
        yuv422_8<NV16, FILTER>(P.C, FramecamPos<CAMERA>{P});
    } else {
        yuv422_8<NV16, FILTER>(args.C, FramecamPos<CAMERA>{args});
    }
}

template <int CAMERA, bool SEMI, int SHIFT, int FILTER>
__global__ __launch_bounds__(256) void framecam_422_16_kernel(FramecamArgs args) {
    if constexpr (kFramecamStage && CAMERA == 0 && !SEMI) {
        FRAMECAM_STAGE_IN_LDS(P, args);
        yuv422_16<SEMI, SHIFT, FILTER>(P.C, P.fill_y, P.fill_uv, FramecamPos<CAMERA>{P});
    } else {
        yuv422_16<SEMI, SHIFT, FILTER>(args.C, args.fill_y, args.fill_uv, FramecamPos<CAMERA>{args});
    }
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void framecam_444_kernel(FramecamArgs P) {
    yuv444_8<FILTER>(P.C, FramecamPos<CAMERA>{P});
}

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void framecam_444_16_kernel(FramecamArgs P) {
    yuv444_16<FILTER>(P.C, P.fill_y, P.fill_uv, FramecamPos<CAMERA>{P});
}

#undef FRAMECAM_STAGE_IN_LDS

} // namespace
