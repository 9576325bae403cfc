/*
 * rssync_rectify.h -- grayscale frames with the rolling-shutter skew removed, on the GPU, from the gyro data and the
 * delay the solver has found.  Part of librssync_core.so; a separate header because it is not part of the reference's
 * surface (rssync.h) nor of its flat mirror (rssync_c.h).
 *
 * For a frame with time T the result is what a global-shutter camera with the same lens would have seen at the
 * orientation q_ref = q(T + ro * ref_row / rows + delay): every output pixel (u, v) is looked up in the rolling-shutter
 * frame at the position where its ray was captured.  Rotation only (the solver estimates no translation).  Conventions
 * are the solver's: q(t) is the componentwise cubic spline through the gyro orientations, renormalised, a camera ray c
 * sees the world direction R(q)^T c (core_private.cpp:24-28); a row's time is frame_time + ro * row / rows
 * (core_testcode.cpp:144-145); rssync_lens is the fisheye model of rssync_ext_set_track_pixels.
 *
 * The map, per output pixel: r = unit ray of (u, v) (the driver's undistortion, polished with three Newton steps on the
 * model's true derivative so that it is the inverse of the forward model below for every lens; fp64, kept as fp32); a
 * table of the
 * rows + 1 matrices M_j = R(q(T + ro * j / rows + delay)) R(q_ref)^T (fp64, kept as fp32); then, from y = v,
 * `iterations` times: M = M_i + (y' - i)(M_(i+1) - M_i) with y' = y clamped to [0, rows - 1] and i = floor(y'),
 * (x, y) = project(M r) with the closed-form forward model theta_d = theta (1 + k1 theta^2 + .. + k4 theta^8).  The last
 * (x, y) is the source position: inside the image when 0 <= x <= width - 1 and 0 <= y <= height - 1.  At 2 rad/s and
 * 11 ms of readout the third iteration moves the map by 2e-5 px.
 *
 * Sampling is bilinear in fp32 in one fixed order of operations (x0 = min(floor(x), width - 2), fx = x - x0, likewise y;
 * top = p00 + fx (p01 - p00), bot = p10 + fx (p11 - p10), value = top + fy (bot - top), rounded to nearest even), so the
 * bytes are reproducible from the map.  Pixels whose source lies outside get `fill`.
 *
 * A pixel the lens cannot image -- its centred, normalised radius lies beyond the model's largest value on (0, pi / 2),
 * or the inversion is left with a residual above 1e-10 px -- has no ray: its position in rssync_rectify_map is (NaN, NaN),
 * it gets `fill` and is counted in n_outside; rssync_rectify_points answers (NaN, NaN) for such a point.
 *
 * Frames are n_frames x height rows of width uint8 pixels, rows `pitch` bytes apart, frames `frame_stride` bytes apart;
 * the frames and the result may each be host memory or device memory of the problem's first device
 * (rssync_ext_device_context); a pointer into another device's memory is an error.  Device memory is read and written in
 * place, host memory passes through the device in chunks of a fixed budget.  The calls keep no state but a cache of the
 * ray map of the last (lens, width, height).
 *
 * Errors follow rssync_set_panic_mode: no gyro data installed; a frame whose row times plus delay leave the gyro's
 * knots (nothing is extrapolated); NULL pointers; pitch < width; width or height below 2; non-finite times, delay or
 * lens; negative ro; parameters out of range; the result overlapping the frames.
 */
#ifndef RSSYNC_RECTIFY_H
#define RSSYNC_RECTIFY_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NULL = all defaults.  A struct of all zeros means all defaults too, so that `= {0}` works; as soon as any field is
 * non-zero the fields are read one by one, and then ref_row 0 IS row 0 -- to ask for row 0 with black fill, write
 * iterations out (3).  A NEGATIVE ref_row always means its default. */
typedef struct rssync_rectify_params {
    double ref_row;     /* the row whose time the output is rendered at, 0 .. rows; negative = default: rows / 2 */
    int32_t iterations; /* 1 .. 8; 0 = default: 3 */
    int32_t fill;       /* 0 .. 255: value of pixels whose source is outside the frame */
} rssync_rectify_params;

/* The source position of every output pixel of a frame at frame_time: map_xy is height x width x {x, y} (host or
 * device memory), positions outside the image included as computed. */
int rssync_rectify_map(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, double frame_time, double delay,
                       const rssync_rectify_params* params, float* map_xy);

/* Rectify n_frames frames.  frame_times: n_frames times in seconds (host).  out: as the frames, rows out_pitch and
 * frames out_stride bytes apart; bytes of `out` between the rows are not written.  out must not overlap frames.
 * n_outside: NULL, or n_frames counts of the pixels that got `fill` (host). */
int rssync_rectify_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                          size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay,
                          const rssync_rectify_params* params, uint8_t* out, size_t out_pitch, size_t out_stride, uint64_t* n_outside);

/* The forward direction, for tracked points: a position (x, y) in the rolling-shutter frame goes to its position in the
 * rectified frame, project(R(q_ref) R(q(T + ro * y / rows + delay))^T ray(x, y)): closed form, fp64, the orientation taken
 * at the point's own row (not from the table of rows).  points, out: count x {x, y} (host or device memory).  A point
 * whose row time leaves the gyro's knots takes the orientation of the nearest knot. */
int rssync_rectify_points(rssync_problem* p, const double* points, size_t count, size_t width, size_t height,
                          const rssync_lens* lens, double frame_time, double delay, const rssync_rectify_params* params, double* out);

#ifdef __cplusplus
}
#endif
#endif
