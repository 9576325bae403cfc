/*
 * rssync_features.h -- grayscale frames -> corner features tracked forward and backward on the GPU, the usual front end
 * of a video/gyro sync ahead of rssync_ext_set_track_pixels.  Part of librssync_core.so, next to the grid tracker
 * (rssync_track.h), whose frame layout, pyramid, LK and batching rules it shares.
 *
 * Detector (per frame, level 0, integers only -- tests/feature_reference.py restates it bit for bit):
 *   gx = I[y][x+1] - I[y][x-1], gy = I[y+1][x] - I[y-1][x]; over a block x block window centred on the pixel
 *   A = sum gx^2, B = sum gx gy, C = sum gy^2 (int32); R = 64 (A C - B^2) - 3 (A + C)^2 (int64; Harris, k = 3/64).
 *   Valid pixels: b <= x <= width-1-b, b <= y <= height-1-b with b = block/2 + 1.  p beats q iff R(p) > R(q), or they are
 *   equal and p's raster index y width + x is smaller.  p is a local maximum iff it beats each of its valid
 *   8-neighbours.  T = max(1, ceil(quality * (double)R_max)) over the frame's valid pixels.  Cells of cell x cell px,
 *   numbered x-major (x outer, y inner) with partial cells at the right and bottom: a cell's feature is its local
 *   maximum that beats all others, if its R >= T.  A frame's features are listed in cell order, at most
 *   S = ceil(width / cell) * ceil(height / cell).
 *
 * Tracking: LK forward from frame k to k+1 at each feature a (rssync_track.h's LK: the same pyramid, window, stopping
 * rules and statuses 0 .. 3), then backward from k+1 to k started at b = a + flow_fwd.  fb_error = |flow_fwd + flow_bwd|
 * in fp32.  A track of forward status 0 becomes RSSYNC_FEATURE_FB_MISMATCH when the backward status is not 0 or
 * fb_error > max_fb_error.  The backward pass runs for tracks of forward status 0 only; the others have a NaN fb_error.
 *
 * Errors follow rssync_set_panic_mode, with the tracker's checks plus: cell outside 16 .. 128, block even or outside
 * 3 .. 9, quality outside (0, 1], a negative max_fb_error or min_tracks, lk.grid_step not 0, a frame smaller than
 * 2 b + 1.
 */
#ifndef RSSYNC_FEATURES_H
#define RSSYNC_FEATURES_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_track.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a track whose forward status is 0 but whose backward pass failed or did not come back within max_fb_error */
#define RSSYNC_FEATURE_FB_MISMATCH 4

/* 0 in any field = its default; NULL = all defaults */
typedef struct rssync_feature_params {
    int32_t cell;          /* px, 16 .. 128; default 64 */
    int32_t block;         /* odd, 3 .. 9; default 5 */
    double quality;        /* (0, 1]: the threshold's share of the frame's largest response; default 0.01 */
    double max_fb_error;   /* px; default 0.5 */
    int32_t min_tracks;    /* rssync_features_frames: fewest kept tracks a pair needs to be handed on; default 8 */
    rssync_track_params lk; /* the LK settings; grid_step must be 0 */
} rssync_feature_params;

/* Detect and track the features of every pair k (frame k -> frame k+1).  Outputs, each laid out [k][cap] over the
 * n_frames - 1 pairs, of which the first counts[k] entries of pair k are set:
 *   points_a  {x, y}   the features of frame k (integer pixels), in cell order
 *   points_b  {x, y}   a + flow_fwd
 *   status             RSSYNC_TRACK_* (0 .. 3, forward) or RSSYNC_FEATURE_FB_MISMATCH
 *   fb_error           px
 * cap: the caller's room per pair; *n_cells = S, also when cap < S (then an error). */
int rssync_features_track(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                          size_t frame_stride, const rssync_feature_params* params, double* points_a, double* points_b,
                          uint8_t* status, float* fb_error, uint32_t* counts, size_t cap, size_t* n_cells);

/* Detect and track, then rssync_ext_set_track_pixels(p, first_frame + k, frame_times[k], frame_times[k+1], a_k, b_k, n_k,
 * lens, height) with the status-0 tracks of every pair k that keeps at least min_tracks of them.  A pair with fewer is not
 * handed on, and what the problem held for that frame index is left as it was.  *n_set (may be NULL): the pairs handed
 * on.  frame_times: n_frames times in seconds. */
int rssync_features_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                           size_t frame_stride, const double* frame_times, int64_t first_frame, const rssync_lens* lens,
                           const rssync_feature_params* params, size_t* n_set);

#ifdef __cplusplus
}
#endif
#endif
