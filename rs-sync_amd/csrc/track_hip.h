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

/* corner features (features_api.cpp): every field resolved and checked there */
typedef struct rship_feature_cfg {
    rship_track_cfg lk;  /* step unused */
    uint32_t cell;       /* 16 .. 128 */
    uint32_t block;      /* odd, 3 .. 9 */
    double quality;      /* (0, 1] */
    float max_fb_error;  /* px */
} rship_feature_cfg;

/* Detect the corners of every frame but the last (kernels/features.hpp) and track each frame's list forward to the next
 * frame and back.  S = ceil(w / cell) * ceil(h / cell) slots per pair: points[2 * (k * S + i)] (x, y), counts[k],
 * flow_fwd / flow_bwd [2 * (k * S + i)], status[k * S + i] (0 .. 4), fb_error[k * S + i] (host buffers); entries at
 * i >= counts[k] are unspecified.  Chunks, uploads and input kinds as rship_track_frames. */
int rship_features_track(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                         const rship_feature_cfg* cfg, int32_t* points, uint32_t* counts, float* flow_fwd, float* flow_bwd,
                         uint8_t* status, float* fb_error);
/* for tests: LK of caller-given integer points, the forward pass of rship_features_track with the residual --
 * lk_kernel's computation at points[2 * (k * cap + i)] for i < counts[k] (points inside the frame).  Outputs laid out as
 * the points; cfg->step unused. */
int rship_track_list(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                     const rship_track_cfg* cfg, const int32_t* points, const uint32_t* counts, uint32_t cap, float* flow,
                     uint8_t* status, float* residual);

#ifdef __cplusplus
}

struct rssync_track_params; // include/rssync_track.h

namespace rssync_host __attribute__((visibility("hidden"))) {
/* the tracker's parameters with their defaults resolved and checked (track_api.cpp; panics on a bad one) */
rship_track_cfg resolve_track_params(const rssync_track_params* p, size_t width, size_t height);
} // namespace rssync_host
#endif
#endif
