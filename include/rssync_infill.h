/*
 * rssync_infill.h -- the stabiliser's borders filled from the neighbouring frames of the call, on the GPU: an output pixel
 * whose source lies outside its own frame is looked up in the frames before and after it, rendered at this frame's target
 * orientation, before it gets `fill`.  The model is rotation only, so a neighbouring frame seen from this frame's target
 * shows the same world directions.  The third answer to a border, beside the zoom that crops it away (rssync_zoom.h) and
 * the limiter that gives up smoothing until none shows (rssync_limit.h): the zoom and the smoothing stay.  Part of
 * librssync_core.so; a separate header as rssync_zoom.h is.  Conventions, parameters, defaults, output camera, targets,
 * memory placement and errors are those of rssync_stabilize.h; params->zoom is read (one zoom for the call).  Grayscale
 * (8-bit) frames; both cameras, both filters, any output size, host or device memory, pitched or not.
 *
 * Targets and rays.  The target of frame f, q_f, is the caller's targets[f] or the path at params->sigma, exactly as
 * rssync_stabilize_frames uses it.  An output pixel's ray is the one rssync_stabilize_frames uses -- the cached ray map
 * (RSSYNC_CAMERA_LENS) or the three fp32 divisions (RSSYNC_CAMERA_PINHOLE).  It does not depend on the candidate and is
 * formed once.
 *
 * Candidates.  The candidates of frame f, in order: f itself; then for d = 1 .. radius the frame f - d, then f + d.  A
 * candidate is skipped where it falls outside 0 .. n_frames - 1.  Neighbours are frames of this call only, by index: the
 * caller orders the frames.
 *
 * The map per candidate.  For candidate g the row table is that of rssync_stabilize.h for a frame with time T_g =
 * frame_times[g] against the target q_f, rows 0 .. height; the source position is the stabiliser's iteration of the ray
 * with that table, from the same start row, with the same number of iterations and the same lens.  The first candidate
 * whose position is inside (0 <= x <= width - 1 and 0 <= y <= height - 1) gives the value: params->filter's sampler
 * applied to frame g at that position.
 *
 * Fill and counts.  A pixel for which no candidate is inside, or which has no ray, gets params->fill.  n_outside[f] counts
 * the pixels of frame f that got `fill`; n_borrowed[f] counts those whose value came from a candidate other than f.
 *
 * What follows, and holds exactly:
 *   - With explicit `targets`, every pixel is byte for byte the pixel of rssync_stabilize_frames called on frame g alone
 *     (time T_g, target targets[f], the same params), for the first g in the order that does not fill it.
 *   - radius == 0, or n_frames == 1, is rssync_stabilize_frames byte for byte, with n_borrowed all 0.
 *   - Frame f's bytes and counts depend on the frames max(0, f - radius) .. min(n_frames - 1, f + radius) of the call and
 *     on nothing else: not on how the call was chunked, not on host or device memory, not on pitches.
 *
 * Errors, besides those of rssync_stabilize.h: a radius outside 0 .. 8.  Each returns non-zero and leaves the problem
 * usable.
 *
 * Not here: colour and 16-bit formats (rssync_colorinfill.h has them); a zoom per frame (rssync_zoom.h); blending or
 * feathering at the seam between a frame and its donor; neighbours that are not frames of the call.
 */
#ifndef RSSYNC_INFILL_H
#define RSSYNC_INFILL_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"
#include "rssync_stabilize.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_INFILL_MAX_RADIUS = 8 };

/* rssync_stabilize_frames with the borders taken from up to `radius` (0 .. 8) frames on each side.  n_outside: NULL, or
 * n_frames counts of the pixels that got `fill`; n_borrowed: NULL, or n_frames counts of the pixels taken from another
 * frame (both host). */
int rssync_infill_stabilize(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                            size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                            const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                            size_t out_stride, uint64_t* n_outside, int32_t radius, uint64_t* n_borrowed);

#ifdef __cplusplus
}
#endif
#endif
