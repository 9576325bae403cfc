/*
 * rssync_track.h -- grayscale frames -> tracked grid points on the GPU: the reference driver's optical-flow step
 * (core_testcode.cpp:97-133), ahead of rssync_ext_set_track_pixels.  Part of librssync_core.so; a separate header
 * because it is not part of the reference's surface (rssync.h) nor of its flat mirror (rssync_c.h).
 *
 * The tracker is a sparse pyramidal Lucas-Kanade (inverse compositional, translation only) at the driver's grid:
 * points (i, j) for i = step, 2 step, ... < width (outer) and j = step, ... < height (inner), i.e.
 * floor((width-1)/step) * floor((height-1)/step) points in x-major order.  Pyramid: separable binomial
 * [1 4 6 4 1] / 16, even pixels kept, reflect-101 border, level size ((w+1)/2, (h+1)/2).  Flow starts at 0 at the
 * coarsest level and doubles between levels; sampling is bilinear with coordinates clamped to the border.
 *
 * Frames: n_frames x height rows of width uint8 pixels (gray), rows `pitch` bytes apart, frames `frame_stride` bytes
 * apart, in host memory or in device memory of the problem's first device (rssync_ext_device_context); a pointer into
 * another device's memory is an error.  n frames give n-1 pairs (frame k, frame k+1).  Decoding and colour
 * conversion are the caller's.
 *
 * Calls keep no state: to stream a long video, pass overlapping batches -- frames [k, k+B], then [k+B, k+2B], ... --
 * with first_frame = k, k+B, ...; the pair (k+B-1, k+B) belongs to the first batch only.  The result of a pair does not
 * depend on the batch it was tracked in.  Frames are processed in chunks of a fixed device-memory budget.
 *
 * Errors follow rssync_set_panic_mode: n_frames < 2, NULL pointers, pitch < width, step < 1, a frame too small for
 * the pyramid (every level at least 3 x 3), non-finite frame times, a NULL lens, bad parameters.
 */
#ifndef RSSYNC_TRACK_H
#define RSSYNC_TRACK_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a tracked point; every point is handed on whatever its status (the reference hands on every point) */
#define RSSYNC_TRACK_OK 0
#define RSSYNC_TRACK_ILL_CONDITIONED 1 /* smallest eigenvalue of the 2x2 structure tensor / window area < min_eig (level 0) */
#define RSSYNC_TRACK_LEFT_IMAGE 2      /* b left the image */
#define RSSYNC_TRACK_ITER_CAP 3        /* max_iters reached at the finest level */

/* 0 in any field = its default (the customary pyramidal-LK values); NULL = all defaults */
typedef struct rssync_track_params {
    int32_t grid_step; /* px; default 200 (the driver's) */
    int32_t window;    /* odd side of the square window, 3 .. 21; default 21 */
    int32_t levels;    /* pyramid levels including the frame itself, 1 .. 8; default 4 */
    int32_t max_iters; /* per level; default 30 */
    double epsilon;    /* px: stop when an update is shorter; default 0.01 */
    double min_eig;    /* intensity^2 / px^2 (pixel values 0 .. 255); default 1e-4 */
} rssync_track_params;

/* Track the grid points of every pair.  Outputs (P = grid points, n_frames - 1 pairs):
 *   points_a  P x {x, y}                     the grid
 *   points_b  (n_frames-1) x P x {x, y}      a + flow
 *   status    (n_frames-1) x P               RSSYNC_TRACK_*
 *   residual  (n_frames-1) x P               mean |I_b - T| over the window at b, level 0 (pixel values)
 * cap: the caller's room in grid points (P); *n_points = P, also when cap is too small (then an error). */
int rssync_track_points(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                        size_t frame_stride, const rssync_track_params* params, double* points_a, double* points_b,
                        uint8_t* status, float* residual, size_t cap, size_t* n_points);

/* Track, then rssync_ext_set_track_pixels(p, first_frame + k, frame_times[k], frame_times[k+1], grid, b_k, P, lens,
 * height) for every pair k: frames in, the problem's tracks out.  frame_times: n_frames times in seconds. */
int rssync_track_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                        size_t frame_stride, const double* frame_times, int64_t first_frame, const rssync_lens* lens,
                        const rssync_track_params* params);

#ifdef __cplusplus
}
#endif
#endif
