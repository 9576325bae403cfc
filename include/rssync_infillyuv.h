/*
 * rssync_infillyuv.h -- the borders of 4:2:2 and 4:4:4 video filled from the neighbouring frames of the call, on the GPU:
 * the infill of rssync_infill.h for every format of rssync_yuv.h (I422, NV16, I444, I210, P210, P216, I410), as
 * rssync_colorinfill.h is for the 4:2:0 family.  Part of librssync_core.so; a separate header with one function, whose
 * signature is rssync_colorinfill_stabilize's.
 *
 * Everything that is not the candidate loop is rssync_yuv_stabilize's, unchanged: the layouts, the fills by depth, the
 * alignment of 16-bit planes, the sizes (4:2:2 widths even and at least 4), the chroma site, parameters, defaults, output
 * cameras, targets, memory placement and errors; params->stab.zoom is read (one zoom for the call).  Both cameras, both
 * filters, any output size, host or device memory, pitched or not.
 *
 * A plane is a camera.  Every plane runs the procedure of rssync_infill.h with its own camera:
 *   - Candidates.  The candidates of frame f, in order: f itself; then for d = 1 .. radius the frame f - d, then f + d.  A
 *     candidate is skipped where it falls outside 0 .. n_frames - 1.
 *   - The map per candidate.  For candidate g the row table is frame g's (time T_g, height + 1 entries) against the target
 *     of frame f, the one target of all of f's planes: the caller's targets[f], or the path at params->stab.sigma.  The ray
 *     of an output sample does not depend on the candidate and is formed once.
 *   - The value.  The first candidate whose position is inside that plane (0 <= x <= cols - 1 and 0 <= y <= rows - 1 of
 *     the plane) gives the value, through params->stab.filter's sampler for that format, applied to that plane of frame g.
 *   - 4:2:2 chroma.  The plane is rssync_yuv.h's camera halved in x alone: its lens, its output camera, width / 2 x height,
 *     the luma's row table and frame time.  U and V share the one position and the one donor.  A luma pixel and the chroma
 *     sample over it are decided apart and may come from different frames.
 *   - 4:4:4.  Y, U and V of a pixel share one position, one donor and one set of taps and weights.
 *
 * Fill and counts.  A sample for which no candidate is inside, or which has no ray, gets its plane's fill.  n_outside[f]
 * holds two counts: the samples of plane 0 of frame f that got the fill, then the chroma samples (of one chroma plane) that
 * got it.  n_borrowed[f] holds two counts: the samples of plane 0 whose value came from a candidate other than f, then the
 * chroma samples.  For 4:4:4 the second count of each equals the first, as rssync_yuv.h has it for n_outside.
 *
 * What follows, and holds exactly:
 *   - 8-bit planes.  With explicit `targets`, each plane is rssync_infill_stabilize of that plane as gray frames, byte for
 *     byte, both counts included, where the gray call uses that plane's lens, frame times, output camera (out_camera) and
 *     fill.  This covers Y, U and V of I422 and of I444 (whose chroma uses the luma camera) and the deinterleaved U and V
 *     of NV16: NV16 is I422 with the chroma interleaved.
 *   - Every sample, 16-bit included, is the sample of rssync_yuv_stabilize called on frame g alone, with time T_g, target
 *     targets[f] and the same params, for the first g in the order that does not fill it.
 *   - radius == 0, or n_frames == 1, is rssync_yuv_stabilize byte for byte, with n_borrowed all 0.
 *   - A 16-bit format on 8-bit values (P210: on values << 6) gives the 8-bit sibling's result widened, counts included:
 *     every sample with the bilinear sampler; with the bicubic one, which clamps to the format's range, every sample but
 *     those the sibling clamped at 255, which are 255 or more.
 *   - Frame f's bytes and counts depend on the frames max(0, f - radius) .. min(n_frames - 1, f + radius) of the call and
 *     on nothing else: not on how the call was chunked, not on host or device memory, not on pitches.
 *
 * Errors, besides those of rssync_yuv_stabilize: a radius outside 0 .. 8; a format that is none of RSSYNC_YUV_* ("format").
 * Each returns non-zero and leaves the problem usable.
 *
 * Not here: a joint donor for luma and chroma; a zoom per frame together with the infill (rssync_zoomyuv.h); blending or
 * feathering at the seam between a frame and its donor; packed 4:2:2 (YUY2, UYVY, v210).
 */
#ifndef RSSYNC_INFILLYUV_H
#define RSSYNC_INFILLYUV_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_infill.h"
#include "rssync_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rssync_yuv_stabilize with the borders taken from up to `radius` (0 .. RSSYNC_INFILL_MAX_RADIUS) frames on each side:
 * format is any of RSSYNC_YUV_*; n_outside and n_borrowed are NULL or n_frames x 2 values (host): plane 0, chroma. */
int rssync_infillyuv_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                               const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                               const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                               uint64_t* n_outside, int32_t radius, uint64_t* n_borrowed);

#ifdef __cplusplus
}
#endif
#endif
