// limit.hpp -- the path limiter (include/rssync_limit.h): how far every frame may follow its goal at a fixed zoom without
// showing a border.  Part of the single HIP translation unit rssync_kernels.hip, after kernels/zoom.hpp: the row table, the
// map and the border rule are the stabiliser's, called here; what is new is in limit_math.hpp.
//
//   limit_fit_kernel   one 256-thread workgroup per frame, the whole bisection over the strength in the kernel
//                      (rs::limit_bisect, the one the CPU check runs).  The camera of a frame is fixed; what changes with
//                      every candidate is the target, and with it the frame's whole row table.  Per candidate:
//                        1. every thread forms c(a) and normalises it (uniform work, no hand-off);
//                        2. thread t rebuilds the table entries t, t + 256, .. of the frame's slot of the chunk's buffer;
//                        3. __syncthreads();
//                        4. thread t maps the border pixels t, t + 256, .. as zoom_fit_kernel does and stops at its first
//                           outside pixel;
//                        5. one __syncthreads_or makes the decision uniform; the next candidate's table writes come after it.
//                      Thread 0 writes strength and status.
//
// The table hand-off through global memory.  Correctness rests on two things, neither of them a property of a cache:
//   stores of a candidate's table before its loads: the __syncthreads() of step 3.  The compiler emits it as a
//     workgroup-scope release fence, the barrier and a workgroup-scope acquire fence: every wave's table stores have
//     completed before it arrives, and no load of step 4 is moved above it.  All waves of a workgroup run on one compute
//     unit, so workgroup scope is enough for global memory that only this workgroup touches (LLVM's AMDGPU memory model;
//     the library never asks for thread-group-split mode); no other workgroup reads or writes a frame's slot, and the slot
//     is stored to in this kernel, so its loads are vector loads, not loads through the scalar cache.
//   loads of a candidate's table before the next candidate's stores: data dependence, NOT the barrier of step 5, whose
//     fence (inside __syncthreads_or's reduction) may cover LDS only.  A thread's vote `out` is computed from the values
//     its table loads returned, so every load has returned before the thread votes; the next candidate's strength is
//     computed from the vote's result, and every table entry stored for it is computed from that strength, so no such
//     store can be issued, by the hardware or by a reordering compiler, before every thread has voted.
//
// Two things do not change between the candidates of a frame.  Both choices were measured (profiles/limit_rate.json, with
// builds that have since been removed):
//   the border's rays with the lens camera, 16 bytes each: KEPT.  They are computed once in front of the bisection into a
//     slot in global memory of which a thread reads only what it wrote itself.  The fp64 ray (sin, cos, atan2) leaves the
//     bisection's loop and its constants leave the loop's scalar registers -- 96 SGPRs, 166 VGPRs, no spill, where the
//     kernel that computed them per candidate had 106, 197 and four spilled SGPRs -- and the fit runs at 2.3 to 2.4
//     times the rate of that kernel.
//   the orientations q(row time) of the height + 1 rows, 32 bytes each: COMPUTED AGAIN for every candidate.  Kept in global
//     memory (at 2160 rows they are 69 KB a frame, which in LDS would leave two workgroups a compute unit) they changed
//     the rate by about 1 % in either direction, within the measurement's spread, at 57 MB of device memory a chunk:
//     one fused cubic per component and a square root against a 32-byte load.
// (the names hold none of the strings by which the tests count the kernels of the other families)
#pragma once

namespace {

struct LimitFitArgs {
    const double* table;    // fp64 spline table
    const double* times;    // frame times of the chunk's frames
    const double* own;      // [chunk frames][4]: the path at sigma 0
    const double* goal;     // [chunk frames][4]: the caller's targets as given, or the path at sigma
    const double* cams;     // [chunk frames]: the zoom of every frame
    float* rows_tab;        // the chunk's tables, rebuilt here
    float4* rays;           // LENS: [chunk frames][n_border]: the border's rays, kept between candidates; else NULL
    double* strengths;      // [chunk frames]
    uint32_t* status;       // [chunk frames]
    rs::Lens cam;           // the output camera at zoom 1 with the lens's k1 .. k4 (ro unused)
    rs::RectLensF lens;     // the input lens
    double start, fs, ro, delay;
    float y_scale;
    uint32_t n_knots, width, height, out_width, out_height, n_border;
    int32_t iterations, camera, steps;
};

// what differs from frame to frame: the same in all threads
struct LimitFrame {
    double r[4], g[4], time, fx, fy;
    float* tab;     // the frame's slots
    float4* rays;   // (LENS)
};

// clear(frame, a) of the workgroup's frame, uniform over the workgroup: every thread must call it
__device__ inline bool limit_border_clear(const LimitFitArgs& A, const LimitFrame& F, double a) {
    double c[4], u[4];
    rs::limit_blend(F.r, F.g, a, c);
    rs::limit_unit(c, u);
    const rs::RectQuat qt{u[0], u[1], u[2], u[3]};
    for (uint32_t j = threadIdx.x; j <= A.height; j += 256) {
        float m[9];
        rs::stab_row_matrix(A.table, (int)A.n_knots, A.start, A.fs, A.ro, F.time, (double)A.height, A.delay, qt, (double)j, m);
        float* out = F.tab + (size_t)j * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = m[k];
    }
    __syncthreads(); // the table is whole (see the head of this file)
    rs::Lens cam = A.cam;
    cam.fx = F.fx;
    cam.fy = F.fy;
    bool out = false;
    for (uint32_t b = threadIdx.x; b < A.n_border && !out; b += 256) {
        uint32_t bu, bv;
        rs::stab_border_pixel(b, A.out_width, A.out_height, &bu, &bv);
        float rx, ry, rz;
        if (A.camera == 0) {
            const float4 ray = F.rays[b];
            rx = ray.x; ry = ray.y; rz = ray.z;
        } else {
            rs::stab_pinhole_ray(rs::StabCamF{(float)cam.fx, (float)cam.fy, (float)cam.cx, (float)cam.cy}, (float)bu, (float)bv, &rx, &ry, &rz);
        }
        float x, y;
        rs::rect_map_pixel(F.tab, (int)A.height, A.lens, A.iterations, rs::stab_start_row((float)bv, A.y_scale), rx, ry, rz, &x, &y);
        out = !rs::rect_inside(x, y, (int)A.width, (int)A.height);
    }
    return !__syncthreads_or(out); // (uniform; the next candidate's stores depend on this result: see the head of this file)
}

__global__ __launch_bounds__(256) void limit_fit_kernel(LimitFitArgs args) {
    // the arguments are read from LDS, not from scalar registers, for zoom_fit_kernel's reason: the fp64 constants of the
    // ray and of the spline are hoisted in front of the loops, and with the arguments live across them as well the scalar
    // file overflows.  Every value is the same in all threads: the branches and the barriers below are uniform in fact.
    __shared__ LimitFitArgs A;
    __shared__ LimitFrame F; // (the frame's values as well: eleven doubles and two pointers that are the same in all threads)
    const uint32_t f = blockIdx.x;
    if (threadIdx.x == 0) {
        A = args;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            F.r[i] = args.own[(size_t)f * 4 + i];
            F.g[i] = args.goal[(size_t)f * 4 + i];
        }
        F.time = args.times[f];
        F.fx = args.cam.fx * args.cams[f];
        F.fy = args.cam.fy * args.cams[f];
        F.tab = args.rows_tab + (size_t)f * (args.height + 1) * 9;
        F.rays = args.camera == 0 ? args.rays + (size_t)f * args.n_border : nullptr;
    }
    __syncthreads();
    if (A.camera == 0) {
        // the border's rays, once: thread t later reads exactly the entries t, t + 256, .. it writes here
        float4* rays = F.rays;
        rs::Lens cam = A.cam;
        cam.fx = F.fx;
        cam.fy = F.fy;
        for (uint32_t b = threadIdx.x; b < A.n_border; b += 256) {
            uint32_t bu, bv;
            rs::stab_border_pixel(b, A.out_width, A.out_height, &bu, &bv);
            double ray[3];
            rs::rect_pixel_ray(cam, (double)bu, (double)bv, ray);
            rays[b] = make_float4((float)ray[0], (float)ray[1], (float)ray[2], 0.0f);
        }
    }
    uint32_t status;
    const double strength = rs::limit_bisect([&](double a) { return limit_border_clear(A, F, a); }, A.steps, &status);
    if (threadIdx.x == 0) {
        A.strengths[f] = strength;
        A.status[f] = status;
    }
}

} // namespace
