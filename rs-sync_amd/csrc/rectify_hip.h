/*
 * rectify_hip.h -- the rectifier's launchers in rssync_kernels.hip (kernels/rectify.hpp), called by rectify_api.cpp.
 *
 * Internal to librssync_core.so and deliberately NOT in include/rssync_hip.h, for track_hip.h's reason: that header is
 * the device ABI the host solver is also linked against in its CPU test double, which implements every rship_* declared
 * there.  The rectifier has no CPU double; only the product library links rectify_api.cpp.
 */
#ifndef RSSYNC_RECTIFY_HIP_H
#define RSSYNC_RECTIFY_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rssync_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* every field resolved and checked (rectify_api.cpp): no "default" values here */
typedef struct rship_rectify_cfg {
    uint32_t width, height;
    double lens[9];        /* ro, fx, fy, cx, cy, k1 .. k4 */
    double start, fs;      /* the gyro table's time of knot 0 and its rate */
    uint32_t n_knots;      /* ... and its knots: must be the context's table */
    double delay;
    double ref_row;        /* 0 .. height */
    int32_t iterations;    /* 1 .. 8 */
    int32_t fill;          /* 0 .. 255 */
} rship_rectify_cfg;

/* Rectify n_frames frames of width x height bytes (rows `pitch` bytes apart, frames `frame_stride` bytes apart) into
 * out (out_pitch, out_stride).  Each of the two may be host memory or memory of the context's device; device memory is
 * read and written in place, host memory goes through two chunk slots on the copy stream, the next chunk's upload under
 * this chunk's kernels.  frame_times: n_frames host doubles.  n_outside: n_frames host values, or NULL.
 * budget_bytes: device bytes for the two chunk slots, 0 = the library's fixed budget (the tests pass a small one so that
 * small frames span several chunks). */
int rship_rectify_frames(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                         const double* frame_times, const rship_rectify_cfg* cfg, uint8_t* out, size_t out_pitch, size_t out_stride,
                         uint64_t* n_outside, size_t budget_bytes);
/* the source position of every output pixel of one frame: map_xy [height][width]{x, y} (host or device) */
int rship_rectify_map(rship_ctx* c, double frame_time, const rship_rectify_cfg* cfg, float* map_xy);
/* rolling-shutter positions -> rectified positions, fp64: points, out [count]{x, y} (host or device) */
int rship_rectify_points(rship_ctx* c, const double* points, size_t count, double frame_time, const rship_rectify_cfg* cfg, double* out);

#ifdef __cplusplus
}

struct rssync_problem; /* include/rssync_c.h */

namespace rssync_host __attribute__((visibility("hidden"))) {
/* sync_problem.cpp: the spline table of the installed gyro data is on the problem's devices (built now if a setter left it
 * to the first solve); panics when no gyro data was set */
void ensure_gyro_table(rssync_problem* p);
} /* namespace rssync_host */
#endif
#endif
