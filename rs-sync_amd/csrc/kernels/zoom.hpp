// zoom.hpp -- the dynamic zoom (include/rssync_zoom.h): every frame's smallest clear zoom, and frames rendered with one
// zoom per frame.  Part of the single HIP translation unit rssync_kernels.hip, after kernels/resample.hpp: the map, the
// border rule and both samplers are the stabiliser's, called here; what is new is in zoom_math.hpp.
//
//   zoom_fit_kernel            one 256-thread workgroup per frame, the whole bisection in the kernel.  Thread t owns the
//                              border pixels t, t + 256, ..; for a candidate zoom it evaluates what
//                              stabilize_coverage_kernel evaluates (camera times zoom in fp64, the ray in place, the map,
//                              !rect_inside) and stops at its first outside pixel; one __syncthreads_or makes the step's
//                              decision uniform, so lo and hi live in registers of every thread and no thread leaves the
//                              procedure (rs::zoom_bisect, the one the CPU check runs).  Thread 0 writes zoom and status.
//                              The arguments are staged in LDS (see the kernel): 184 bytes.
//   zoom_render_kernel<C, F>   stabilize_kernel<C, false> (F = 0) and stabilize_bicubic_kernel<C> (F = 1) with the output
//                              camera of frame blockIdx.z read from an array: (fx zoom, fy zoom), the products formed in
//                              fp64 by the host as the stabiliser's are.  PINHOLE: that camera as StabCamF, then
//                              stab_pinhole_ray.  LENS: no cached ray map serves a zoom per frame, so the ray is computed
//                              in place as rectify_rays_kernel computes it -- rect_pixel_ray in fp64, cast to float: the
//                              cache's bits by construction.  The ray is dead before the sampler starts, and no
//                              instantiation needs scratch.
// (names without "stabilize" and with an integer FILTER: the tests count the kernels of those families)
#pragma once

namespace {

struct ZoomFitArgs {
    const float* rows_tab;  // the chunk's tables
    double* zooms;          // [chunk frames]
    uint32_t* status;       // [chunk frames]
    rs::Lens cam;           // the output camera at zoom 1 with the lens's k1 .. k4 (ro unused)
    rs::RectLensF lens;     // the input lens
    double lo, hi;
    float y_scale;
    uint32_t width, height, out_width, out_height, n_border;
    int32_t iterations, camera, steps;
};

// clear(frame, zoom) of the workgroup's frame, uniform over the workgroup: every thread must call it
template <int CAMERA>
__device__ inline bool zoom_border_clear(const ZoomFitArgs& A, const float* tab, double zoom) {
    rs::Lens cam = A.cam;
    cam.fx = A.cam.fx * zoom;
    cam.fy = A.cam.fy * zoom;
    bool out = false;
    for (uint32_t b = threadIdx.x; b < A.n_border && !out; b += 256) {
        uint32_t u, v;
        rs::stab_border_pixel(b, A.out_width, A.out_height, &u, &v);
        float rx, ry, rz;
        if (CAMERA == 0) {
            double ray[3];
            rs::rect_pixel_ray(cam, (double)u, (double)v, ray);
            rx = (float)ray[0]; ry = (float)ray[1]; rz = (float)ray[2];
        } else {
            rs::stab_pinhole_ray(rs::StabCamF{(float)cam.fx, (float)cam.fy, (float)cam.cx, (float)cam.cy}, (float)u, (float)v, &rx, &ry, &rz);
        }
        float x, y;
        rs::rect_map_pixel(tab, (int)A.height, A.lens, A.iterations, rs::stab_start_row((float)v, A.y_scale), rx, ry, rz, &x, &y);
        out = !rs::rect_inside(x, y, (int)A.width, (int)A.height);
    }
    return !__syncthreads_or(out); // (the loop above has no barrier, and the steps of the bisection are uniform)
}

__global__ __launch_bounds__(256) void zoom_fit_kernel(ZoomFitArgs args) {
    // The arguments are read from LDS, not from scalar registers.  Inside the two loops the compiler hoists the fp64
    // constants of the ray (sin, cos, atan2: some thirty scalar and a hundred vector registers) in front of the loops;
    // with the 46 scalar registers of the arguments live across them as well the scalar file overflows and values are
    // parked in vector lanes (14 .. 23 "SGPR spills" in every arrangement tried).  Vector registers are plentiful here
    // (one workgroup per frame, 256 threads), so the arguments go where they cost vector registers: no spill of either
    // kind, no scratch.  Every value is the same in all threads: the branches and the barrier below are uniform in fact.
    __shared__ ZoomFitArgs A;
    if (threadIdx.x == 0) A = args;
    __syncthreads();
    const uint32_t f = blockIdx.x;
    const float* tab = A.rows_tab + (size_t)f * (A.height + 1) * 9;
    uint32_t status;
    double zoom;
    if (A.camera == 0) zoom = rs::zoom_bisect([&](double z) { return zoom_border_clear<0>(A, tab, z); }, A.lo, A.hi, A.steps, &status);
    else zoom = rs::zoom_bisect([&](double z) { return zoom_border_clear<1>(A, tab, z); }, A.lo, A.hi, A.steps, &status);
    if (threadIdx.x == 0) {
        A.zooms[f] = zoom;
        A.status[f] = status;
    }
}

struct ZoomRenderArgs {
    StabArgs S;             // stabilize_kernel's, without the ray map; S.cam holds cx, cy
    const double* cams;     // [chunk frames][2]: fx zoom, fy zoom
    double cx, cy, k1, k2, k3, k4;  // LENS: the rest of the output camera, fp64
};

template <int CAMERA, int FILTER>
__global__ __launch_bounds__(256) void zoom_render_kernel(ZoomRenderArgs Z) {
    const StabArgs& A = Z.S;
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        const double fx = Z.cams[2 * (size_t)f], fy = Z.cams[2 * (size_t)f + 1];
        float rx, ry, rz;
        if (CAMERA == 0) {
            double ray[3];
            rs::rect_pixel_ray(rs::Lens{0.0, fx, fy, Z.cx, Z.cy, Z.k1, Z.k2, Z.k3, Z.k4}, (double)u, (double)v, ray);
            rx = (float)ray[0]; ry = (float)ray[1]; rz = (float)ray[2];
        } else {
            rs::stab_pinhole_ray(rs::StabCamF{(float)fx, (float)fy, A.cam.cx, A.cam.cy}, (float)u, (float)v, &rx, &ry, &rz);
        }
        float x, y;
        rs::rect_map_pixel(A.rows_tab + (size_t)f * (A.height + 1) * 9, (int)A.height, A.lens, A.iterations,
                           rs::stab_start_row((float)v, A.y_scale), rx, ry, rz, &x, &y);
        uint32_t val = (uint32_t)A.fill;
        if (rs::rect_inside(x, y, (int)A.width, (int)A.height)) {
            const uint8_t* src = A.src + (size_t)f * A.src_stride;
            if (FILTER == 0) val = rs::rect_sample(src, (size_t)A.src_pitch, (int)A.width, (int)A.height, x, y);
            else val = cubic8_sample(src, A.src_pitch, rs::cubic_taps((int)A.width, (int)A.height, x, y));
        } else {
            filled = true;
        }
        A.dst[(size_t)f * A.dst_stride + (size_t)v * A.dst_pitch + u] = (uint8_t)val;
    }
    const unsigned long long m = __ballot(filled);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
}

} // namespace
