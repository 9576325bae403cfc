/*
 * stabilize_hip.h -- the stabiliser's launchers in rssync_kernels.hip (kernels/stabilize.hpp), called by
 * stabilize_api.cpp.  Internal to librssync_core.so and not in include/rssync_hip.h, for rectify_hip.h's reason: the
 * stabiliser has no CPU double; only the product library links stabilize_api.cpp.
 */
#ifndef RSSYNC_STABILIZE_HIP_H
#define RSSYNC_STABILIZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "rectify_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* every field resolved and checked (stabilize_api.cpp): no "default" values here */
typedef struct rship_stabilize_cfg {
    uint32_t width, height;         /* the input frames */
    uint32_t out_width, out_height; /* the result */
    double lens[9];                 /* the input lens: ro, fx, fy, cx, cy, k1 .. k4 */
    double cam[4];                  /* the output camera: fx, fy (zoom included), cx, cy */
    double start, fs;               /* the gyro table's time of knot 0 and its rate */
    uint32_t n_knots;               /* ... and its knots: must be the context's table */
    double delay;
    double sigma;                   /* >= 0: the path's smoothing where no targets are given */
    int32_t camera;                 /* RSSYNC_CAMERA_LENS / RSSYNC_CAMERA_PINHOLE */
    int32_t iterations;             /* 1 .. 8 */
    int32_t fill;                   /* 0 .. 255 */
    int32_t filter;                 /* RSSYNC_FILTER_BILINEAR / RSSYNC_FILTER_BICUBIC; in the struct's former tail padding
                                       (offset 172 of 176), so a zero-filled configuration of old is bilinear */
} rship_stabilize_cfg;

/* The smoothed path at n frame times (host): quats [n][4] {w, x, y, z}, host or device.  cfg: lens[0] (ro), start, fs,
 * n_knots, delay and sigma are read. */
int rship_stabilize_path(rship_ctx* c, const double* frame_times, size_t n, const rship_stabilize_cfg* cfg, double* quats);
/* Stabilise n_frames frames (rship_rectify_frames' memory rules and chunking; the result is out_width x out_height).
 * targets: n_frames x 4 unit quaternions (host), or NULL = the path at cfg->sigma.  budget_bytes: device bytes for the
 * two chunk slots, 0 = the library's fixed budget (the tests pass a small one). */
int rship_stabilize_frames(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                           const double* frame_times, const double* targets, const rship_stabilize_cfg* cfg, uint8_t* out,
                           size_t out_pitch, size_t out_stride, uint64_t* n_outside, size_t budget_bytes);
/* the source position of every output pixel of one frame: map_xy [out_height][out_width]{x, y} (host or device);
 * target: 4 (host, unit) or NULL = the path */
int rship_stabilize_map(rship_ctx* c, double frame_time, const double* target, const rship_stabilize_cfg* cfg, float* map_xy);
/* outside [n_frames][n_zooms] (host): border pixels of the output whose source is not inside, with cam's fx, fy (given
 * at zoom 1) multiplied by zooms[z].  One pipeline, one wait. */
int rship_stabilize_coverage(rship_ctx* c, const double* frame_times, uint32_t n_frames, const double* targets,
                             const rship_stabilize_cfg* cfg, const double* zooms, uint32_t n_zooms, uint32_t* outside);

#ifdef __cplusplus
}
#endif
#endif
