// stabilize.hpp -- frames rendered at a target orientation that is not their own (include/rssync_stabilize.h): a smoothed
// gyro path or the caller's orientations, optionally through another output camera.  Part of the single HIP translation
// unit rssync_kernels.hip, after kernels/rectify.hpp, whose ray map, tile and per-pixel arithmetic it shares; what is new
// is in stabilize_math.hpp.
//
//   stabilize_path_kernel      one wave per frame.  Lane l takes the taps l, l + 64, .. of the 385 in that order, then one
//                              shuffle tree (32, 16, .., 1) adds the lanes: one assignment and one tree whatever the number
//                              of frames, so a frame's bits depend on nothing but its time.  fp64; the weights come
//                              tabulated from the host.
//   stabilize_rows_kernel      rectify_rows_kernel with one target orientation per frame instead of q_ref.
//   stabilize_kernel<CAM, MAP> rectify_kernel over the OUTPUT's pixels: the ray from the cached map of the output camera
//                              (LENS) or three fp32 divisions (PINHOLE), the start row scaled to the input's rows, then the
//                              rectifier's iteration, inside test and sampler against the input frame.
//   stabilize_coverage_kernel  one thread per (frame, zoom, border pixel of the output): the same map with the ray computed
//                              in place (the zoom changes the camera, so no cached map serves), counted where the source
//                              is not inside.  One ballot per wave, one atomic per wave that has any.
#pragma once

namespace {

struct StabPathArgs {
    const double* table;    // fp64 spline table
    const double* times;    // frame times
    const double* weights;  // rs::kStabTaps Gaussian weights
    double* quats;          // [n_frames][4]
    double start, fs, t_lo, t_hi, ro, delay, sigma;
    uint32_t n_knots, n_frames;
};

__global__ __launch_bounds__(64) void stabilize_path_kernel(StabPathArgs A) {
    const uint32_t f = blockIdx.x, lane = threadIdx.x;
    const double tc = rs::stab_centre_time(A.times[f], A.ro, A.delay);
    const rs::RectQuat q0 = rs::rect_orientation(A.table, (int)A.n_knots, A.start, A.fs, tc);
    rs::RectQuat q = q0;
    if (A.sigma > 0.0) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = (int)lane; i < rs::kStabTaps; i += 64)
            rs::stab_tap(A.table, (int)A.n_knots, A.start, A.fs, A.t_lo, A.t_hi, tc, A.sigma, i, A.weights[i], q0, acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += __shfl_down(acc[k], off, 64);
        }
        q = rs::stab_finish(acc); // (lane 0 holds the whole sum)
    }
    if (lane == 0) {
        double* out = A.quats + (size_t)f * 4;
        out[0] = q.w; out[1] = q.x; out[2] = q.y; out[3] = q.z;
    }
}

struct StabRowsArgs {
    const double* table;
    const double* times;    // frame times of the chunk's frames
    const double* targets;  // [n_frames][4] unit quaternions of the chunk's frames
    float* rows_tab;        // [n_frames][rows + 1][9]
    double start, fs, ro, delay;
    uint32_t n_knots, rows, n_frames;
};

__global__ __launch_bounds__(256) void stabilize_rows_kernel(StabRowsArgs A) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (j > A.rows) return;
    const double* t = A.targets + (size_t)f * 4;
    float m[9];
    rs::stab_row_matrix(A.table, (int)A.n_knots, A.start, A.fs, A.ro, A.times[f], (double)A.rows, A.delay, rs::RectQuat{t[0], t[1], t[2], t[3]},
                        (double)j, m);
    float* out = A.rows_tab + ((size_t)f * (A.rows + 1) + j) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = m[k];
}

struct StabArgs {
    const float4* rays;          // LENS: the ray map of the output camera, [out_height][out_width]
    const float* rows_tab;       // the chunk's tables, height + 1 entries per frame
    const uint8_t* src;          // frame 0 of the chunk
    uint8_t* dst;
    float2* map;                 // MAP: [out_height][out_width] source positions of frame 0
    unsigned long long* outside; // per frame of the chunk: filled pixels
    uint64_t src_pitch, src_stride, dst_pitch, dst_stride;
    rs::RectLensF lens;          // the input lens
    rs::StabCamF cam;            // PINHOLE: the output camera
    float y_scale;               // (float)height / (float)out_height
    uint32_t width, height, out_width, out_height;
    int32_t iterations, fill;
};

template <int CAMERA, bool MAP>
__global__ __launch_bounds__(256) void stabilize_kernel(StabArgs A) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const bool live = u < A.out_width && v < A.out_height;
    bool filled = false;
    if (live) {
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
        if (MAP) {
            A.map[(size_t)v * A.out_width + u] = make_float2(x, y);
        } else {
            uint8_t val = (uint8_t)A.fill;
            if (rs::rect_inside(x, y, (int)A.width, (int)A.height))
                val = rs::rect_sample(A.src + (size_t)f * A.src_stride, (size_t)A.src_pitch, (int)A.width, (int)A.height, x, y);
            else
                filled = true;
            A.dst[(size_t)f * A.dst_stride + (size_t)v * A.dst_pitch + u] = val;
        }
    }
    if (!MAP) {
        const unsigned long long m = __ballot(filled);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
    }
}

struct StabCoverArgs {
    const float* rows_tab;  // the chunk's tables
    const double* zooms;    // [n_zooms]
    uint32_t* outside;      // [chunk frames][n_zooms]
    rs::Lens cam;           // the output camera at zoom 1 with the lens's k1 .. k4 (ro unused)
    rs::RectLensF lens;     // the input lens
    float y_scale;
    uint32_t width, height, out_width, out_height, n_border, n_zooms;
    int32_t iterations, camera;
};

__global__ __launch_bounds__(256) void stabilize_coverage_kernel(StabCoverArgs A) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y, f = blockIdx.z;
    bool out = false;
    if (b < A.n_border) {
        uint32_t u, v;
        rs::stab_border_pixel(b, A.out_width, A.out_height, &u, &v);
        rs::Lens cam = A.cam;
        cam.fx = A.cam.fx * A.zooms[z];
        cam.fy = A.cam.fy * A.zooms[z];
        float rx, ry, rz;
        if (A.camera == 0) {
            double ray[3];
            rs::rect_pixel_ray(cam, (double)u, (double)v, ray);
            rx = (float)ray[0]; ry = (float)ray[1]; rz = (float)ray[2];
        } else {
            rs::stab_pinhole_ray(rs::StabCamF{(float)cam.fx, (float)cam.fy, (float)cam.cx, (float)cam.cy}, (float)u, (float)v, &rx, &ry, &rz);
        }
        float x, y;
        rs::rect_map_pixel(A.rows_tab + (size_t)f * (A.height + 1) * 9, (int)A.height, A.lens, A.iterations,
                           rs::stab_start_row((float)v, A.y_scale), rx, ry, rz, &x, &y);
        out = !rs::rect_inside(x, y, (int)A.width, (int)A.height);
    }
    const unsigned long long m = __ballot(out);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(A.outside + (size_t)f * A.n_zooms + z, (uint32_t)__popcll(m));
}

} // namespace
