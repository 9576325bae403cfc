/*
 * rssync_stabilize.h -- grayscale frames rendered at a target orientation that is not their own, on the GPU: a smoothed
 * camera path, any orientation the caller brings (horizon lock, a fixed view), optionally through a pinhole camera of
 * another size, with the zoom that keeps the borders out of the picture.  Part of librssync_core.so; a separate header
 * as rssync_rectify.h is, whose conventions these are: rssync_lens; a row's time is T + ro * row / rows; q(t) is the
 * componentwise cubic spline through the gyro orientations, renormalised, clamped to the knots; a camera ray c sees the
 * world direction R(q)^T c; rotation only.
 *
 * The path.  For a frame with time T the centre time is T_c = T + ro * 0.5 + delay.  The taps are k = -192 .. 192, the
 * tap time t_k = T_c + k * sigma / 64 clamped to the first and last knot time, the weight w_k = exp(-0.5 (k / 64)^2)
 * (tabulated once by the host in fp64: no device exp enters the result).  q_k = q(t_k); s_k = -1 if q_k . q_0 < 0, else
 * +1; acc = sum_k w_k s_k q_k; q_s = acc / |acc|.  sigma == 0 returns q(T_c) without the sum.  fp64 throughout, one fixed
 * assignment of taps to lanes and one fixed reduction tree: a frame's bits depend on its time alone, not on the number
 * of frames in the call or on how they were chunked.
 *
 * The map of output pixel (u, v).  The output camera is (fx * zoom, fy * zoom, cx, cy) = (fx', fy', cx, cy).  Its ray r:
 * RSSYNC_CAMERA_LENS, the rectifier's ray of that camera with the lens's k1 .. k4 (the driver's undistortion polished
 * to the inverse of the forward model; fp64, kept as fp32) -- an output pixel that camera cannot image (rssync_rectify.h)
 * has no ray: its position in rssync_stabilize_map is (NaN, NaN), it gets `fill`, is counted in n_outside, and as a
 * border pixel it counts as outside at every zoom of the coverage at which it cannot be imaged;
 * RSSYNC_CAMERA_PINHOLE, ((u - cx) / fx', (v - cy) / fy', 1) normalised, in fp32.  A table of height + 1 matrices
 * M_j = R(q(T + ro * j / height + delay)) R(q_target)^T (fp64, kept as nine fp32 values), where q_target is the path's
 * q_s or the caller's target, normalised in fp64 by the library.  Then, from y = v * (height / out_height) (the factor
 * formed in fp32: exactly 1 when the sizes agree), the rectifier's iteration, `iterations` times:
 * M = M_i + (y' - i)(M_(i+1) - M_i) with y' = y clamped to [0, height - 1] and i = floor(y'), (x, y) = project(M r) with
 * the input lens.  The last (x, y) is the source position in the input frame: inside when 0 <= x <= width - 1 and
 * 0 <= y <= height - 1.  Sampling is the rectifier's bilinear sampler, bit for bit (params->filter ==
 * RSSYNC_FILTER_BILINEAR, the default), or the bicubic one below; pixels whose source is outside get `fill`.
 *
 * Sampling, RSSYNC_FILTER_BICUBIC: Keys' cubic convolution with a = -0.5 (Catmull-Rom) over 4 x 4 taps.  For an inside
 * position (x, y): ix = min(floor(x), width - 2), tx = x - ix (in [0, 1], 1 on the last column only), iy and ty
 * likewise; the tap columns are clamp(ix + d, 0, width - 1) for d = -1, 0, 1, 2 and the rows likewise -- the edge is
 * replicated, so the inside rule, the map and n_outside are those of the bilinear sampler.  The weights of t are
 *     w0 = ((1 - 0.5 t) t - 0.5) t     w1 = ((1.5 t - 2.5) t) t + 1
 *     w2 = ((2 - 1.5 t) t + 0.5) t     w3 = ((0.5 t - 0.5) t) t,
 * exactly (-0, 1, 0, 0) at t = 0 and (0, 0, 1, 0) at t = 1: an integer position returns its sample, and a camera at rest
 * is still the identity.  Per tap row j, r_j = (wx0 p_j0 + wx1 p_j1) + (wx2 p_j2 + wx3 p_j3); then
 * val = (wy0 r_0 + wy1 r_1) + (wy2 r_2 + wy3 r_3), clamped to 0 .. 255 (the kernel overshoots at edges in the picture)
 * and rounded to the nearest integer, ties to even.  Every operation is one fp32 operation rounded on its own, in this
 * order.  The kernel keeps more detail than the bilinear one (noise resampled at a fractional position keeps a standard
 * deviation of 60.9 of 73.9 grey levels instead of 50.2); it costs sixteen taps a pixel instead of four.
 *
 * The anchor: with targets == NULL, sigma = 0, all-default parameters and out_width x out_height == width x height the
 * map equals rssync_rectify_map at its default ref_row bit for bit and the frames equal rssync_rectify_frames byte for
 * byte ((height / 2) / height is exactly 0.5, so q_target is the rectifier's q_ref).
 *
 * Coverage.  outside[f][z] is the number of the 2 (out_width + out_height) - 4 border pixels of the output whose source
 * is not inside, for frame f with params->zoom replaced by zooms[z].  The map is continuous and one-to-one: if the
 * output's border maps inside the frame its interior does too, so the border is enough to choose a zoom.
 *
 * Frames and results are laid out and placed as rssync_rectify.h says: host memory or device memory of the problem's
 * first device, pitched, host memory in chunks of a fixed budget; the result has its own size.
 *
 * Errors follow rssync_set_panic_mode; each returns non-zero and leaves the problem usable: no gyro data installed; NULL
 * pointers; a frame whose row times plus delay leave the gyro's knots (only the path's taps are clamped); sigma negative
 * or non-finite; a zoom or a zooms[] entry <= 0 or non-finite; a non-finite or zero target; only some of fx, fy, cx, cy
 * given; camera or filter outside its enum; sizes below 2; pitches below widths; iterations or fill out of range; out overlapping
 * the frames; a pointer into another device's memory.
 */
#ifndef RSSYNC_STABILIZE_H
#define RSSYNC_STABILIZE_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_CAMERA_LENS = 0, RSSYNC_CAMERA_PINHOLE = 1 };
enum { RSSYNC_FILTER_BILINEAR = 0, RSSYNC_FILTER_BICUBIC = 1 };

/* NULL or all zeros = all defaults */
typedef struct rssync_stabilize_params {
    double sigma;          /* s, >= 0: Gaussian smoothing of the path, used where targets == NULL; 0 = none: q(T_c) itself */
    double zoom;           /* multiplies the output camera's fx, fy; 0 = 1 */
    double fx, fy, cx, cy; /* output camera; all four 0 = the lens's, fx and cx scaled by out_width / width, fy and cy by
                              out_height / height */
    int32_t camera;        /* RSSYNC_CAMERA_LENS: the input lens's k1 .. k4 on the output camera; RSSYNC_CAMERA_PINHOLE: none */
    int32_t iterations;    /* 1 .. 8; 0 = default: 3 */
    int32_t fill;          /* 0 .. 255: value of pixels whose source is outside the frame */
    int32_t filter;        /* RSSYNC_FILTER_BILINEAR (0, the default) or RSSYNC_FILTER_BICUBIC: "Sampling" above.  Read by
                              rssync_stabilize_frames; the map and the coverage check it and do not depend on it.  It lies in
                              what was the struct's tail padding: the size stays 64 bytes, the offset is 60 */
} rssync_stabilize_params;

/* The smoothed path at n frame times (host): quats is n x {w, x, y, z}, host or device memory. */
int rssync_stabilize_path(rssync_problem* p, const double* frame_times, size_t n, double ro, double delay, double sigma, double* quats);

/* The source position of every output pixel of a frame at frame_time: map_xy is out_height x out_width x {x, y} (host or
 * device memory), positions outside the image included as computed.  target: 4 doubles {w, x, y, z} (host), or NULL = the
 * path at params->sigma. */
int rssync_stabilize_map(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                         double frame_time, double delay, const double* target, const rssync_stabilize_params* params, float* map_xy);

/* Stabilise n_frames frames.  frame_times: n_frames times in seconds (host).  targets: n_frames x {w, x, y, z} (host), or
 * NULL = the path.  out: n_frames x out_height rows of out_width pixels, rows out_pitch and frames out_stride bytes
 * apart; bytes of `out` between the rows are not written.  out must not overlap frames.  n_outside: NULL, or n_frames
 * counts of the pixels that got `fill` (host). */
int rssync_stabilize_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                            size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                            const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                            size_t out_stride, uint64_t* n_outside);

/* The border counts of n_frames frames at n_zooms zooms: outside is n_frames x n_zooms (host).  All pairs run in one
 * device pipeline with one wait. */
int rssync_stabilize_coverage(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                              const double* frame_times, size_t n_frames, double delay, const double* targets,
                              const rssync_stabilize_params* params, const double* zooms, size_t n_zooms, uint32_t* outside);

#ifdef __cplusplus
}
#endif
#endif
