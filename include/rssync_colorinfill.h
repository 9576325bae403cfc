/*
 * rssync_colorinfill.h -- the borders of colour video filled from the neighbouring frames of the call, on the GPU: the
 * infill of rssync_infill.h for every format of rssync_color.h and rssync_color16.h (GRAY8, NV12, I420, RGBA32, GRAY16,
 * P010, P016, I010); the 4:2:2 and 4:4:4 formats of rssync_yuv.h have rssync_infillyuv.h.  Part of librssync_core.so; a
 * separate header as rssync_colorzoom.h is.  Layout, parameters, defaults,
 * output cameras, targets, fills, chroma site, alignment rules, memory placement and errors are those of
 * rssync_color_stabilize and, for the formats RSSYNC_COLOR16_*, rssync_color16_stabilize; params->stab.zoom is read (one
 * zoom for the call).  Both cameras, both filters, any output size, host or device memory, pitched or not.
 *
 * A plane is a camera.  Every plane runs the procedure of rssync_infill.h with its own camera:
 *   - Candidates.  The candidates of frame f, in order: f itself; then for d = 1 .. radius the frame f - d, then f + d.  A
 *     candidate is skipped where it falls outside 0 .. n_frames - 1.
 *   - The map per candidate.  For candidate g the row table is that of the plane (rssync_color.h) for frame g against the
 *     target of frame f, the one target of all of f's planes: the caller's targets[f], or the path at params->stab.sigma at
 *     the LUMA frame time.  The ray of an output sample does not depend on the candidate and is formed once.
 *   - The value.  The first candidate whose position is inside that plane (0 <= x <= cols - 1 and 0 <= y <= rows - 1 of
 *     the plane) gives the value, through params->stab.filter's sampler for that format, applied to that plane of frame g.
 *   - Chroma.  For a 4:2:0 chroma plane the camera, the lens and the row count are those of rssync_color.h.  The time of
 *     candidate g is T_g + ro * (oy / height).  U and V share the one position and the one donor.
 *   - RGBA32.  One position and one donor per pixel for the four channels.
 *   - Donors are chosen per sample and per plane: a luma pixel and the chroma sample over it may come from different frames.
 *
 * Fill and counts.  A sample for which no candidate is inside, or which has no ray, gets its plane's fill.  n_outside[f]
 * holds two counts: the samples of plane 0 of frame f that got the fill, then the chroma samples (one per U V pair) that
 * got it.  n_borrowed[f] holds two counts: the samples of plane 0 whose value came from a candidate other than f, then the
 * chroma samples.  The chroma entries are 0 for single-plane formats.
 *
 * What follows, and holds exactly:
 *   - 8-bit planes.  With explicit `targets`, each plane is rssync_infill_stabilize of that plane as gray frames, byte for
 *     byte, both counts included, where the gray call uses that plane's lens, frame times, output camera (out_camera) and
 *     fill.  This covers Y, the U and V of I420, and the deinterleaved U and V of NV12; each RGBA32 channel uses the luma
 *     camera.
 *   - Every sample, 16-bit included, is the sample of rssync_color_stabilize / rssync_color16_stabilize called on frame g
 *     alone, with time T_g, target targets[f] and the same params, for the first g in the order that does not fill it.
 *   - radius == 0, or n_frames == 1, is rssync_color_stabilize / rssync_color16_stabilize byte for byte, with n_borrowed
 *     all 0.
 *   - RSSYNC_COLOR_GRAY8 is rssync_infill_stabilize byte for byte and runs its kernels.
 *   - A 16-bit format on 8-bit values (P010: on values << 6) gives the 8-bit sibling's result widened, counts included, as
 *     rssync_color16.h states for the plain stabiliser: every sample with the bilinear sampler; with the bicubic one, which
 *     clamps to the format's range, every sample but those the sibling clamped at 255, which are 255 or more.
 *   - Frame f's bytes and counts depend on the frames max(0, f - radius) .. min(n_frames - 1, f + radius) of the call and
 *     on nothing else: not on how the call was chunked, not on host or device memory, not on pitches.
 *
 * The limiter's targets (rssync_limit.h) and a constant params->stab.zoom combine with it unchanged.
 *
 * Errors, besides those of the defining calls: a radius outside 0 .. 8; a format that is none of RSSYNC_COLOR_* and
 * RSSYNC_COLOR16_*.  Each returns non-zero and leaves the problem usable.
 *
 * Not here: a joint donor for the planes of a sample (luma and chroma are decided apart); a zoom per frame together with
 * the infill (rssync_colorzoom.h); blending or feathering at the seam between a frame and its donor; neighbours that are
 * not frames of the call.
 */
#ifndef RSSYNC_COLORINFILL_H
#define RSSYNC_COLORINFILL_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_color16.h"
#include "rssync_infill.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rssync_color_stabilize / rssync_color16_stabilize with the borders taken from up to `radius` (0 ..
 * RSSYNC_INFILL_MAX_RADIUS) frames on each side: format is any of RSSYNC_COLOR_* or RSSYNC_COLOR16_*; n_outside and
 * n_borrowed are NULL or n_frames x 2 values (host): plane 0, chroma. */
int rssync_colorinfill_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                                 const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                                 const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                                 uint64_t* n_outside, int32_t radius, uint64_t* n_borrowed);

#ifdef __cplusplus
}
#endif
#endif
