/*
 * track_hip.h -- the tracker's launchers in rssync_kernels.hip (kernels/track.hpp), called by track_api.cpp.
 *
 * Internal to librssync_core.so and deliberately NOT in include/rssync_hip.h: that header is the device ABI the
 * host solver is also linked against in its CPU test double, which implements every rship_* declared there.
 * The tracker has no CPU double; only the product library links track_api.cpp.
 */
#ifndef RSSYNC_TRACK_HIP_H
#define RSSYNC_TRACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rssync_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* every field resolved (no 0 = default here: track_api.cpp resolves and checks them) */
typedef struct rship_track_cfg {
    uint32_t width, height;   /* level 0 */
    uint32_t step;            /* grid step (px) */
    uint32_t window;          /* odd, 3 .. 21 */
    uint32_t levels;          /* 1 .. 8; every level at least 3 x 3 */
    uint32_t max_iters;
    float epsilon;            /* px */
    float min_eig;            /* smallest eigenvalue of the structure tensor / window area */
} rship_track_cfg;

/* Frames [n_frames] of width x height bytes, rows `pitch` bytes apart, frames `frame_stride` bytes apart, in host memory
 * or in device memory of the context's device.  Tracks the grid points of every pair (k, k+1): flow[2 * (k * P + i)],
 * status[k * P + i], residual[k * P + i] with P = floor((w-1)/step) * floor((h-1)/step) (host buffers).  Frames are
 * uploaded in chunks of a fixed device budget on the context's copy stream, overlapping the previous chunk's kernels. */
int rship_track_frames(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                       const rship_track_cfg* cfg, float* flow, uint8_t* status, float* residual);
/* the pyramid the tracker builds, for tests: levels 1 .. levels-1 of each frame, level after level, packed
 * (w_l * h_l floats each), frame after frame.  The frames must fit one chunk. */
int rship_track_pyramid(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                        const rship_track_cfg* cfg, float* out);

#ifdef __cplusplus
}
#endif
#endif
