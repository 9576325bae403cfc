/*
 * rssync_zoom.h -- the dynamic zoom of the stabiliser: the smallest zoom every frame needs to keep its borders out of the
 * picture, found on the GPU; that curve smoothed into an envelope that never undercuts a frame; and grayscale frames
 * rendered with one zoom per frame.  Part of librssync_core.so; a separate header as rssync_stabilize.h is, whose
 * conventions, parameters, defaults, output camera, targets and errors these are.  In all three functions params->zoom
 * is not read, as in rssync_stabilize_coverage.
 *
 * The fit.  clear(f, z) means: rssync_stabilize_coverage of frame f with zooms = {z} returns 0.  Per frame, in fp64:
 *   not clear(f, zoom_hi):  zooms[f] = zoom_hi, status[f] = RSSYNC_ZOOM_NOT_CLEAR;
 *   else clear(f, zoom_lo): zooms[f] = zoom_lo, status[f] = RSSYNC_ZOOM_CLEAR;
 *   else lo = zoom_lo, hi = zoom_hi and `steps` times: mid = 0.5 * (lo + hi); if clear(f, mid) hi = mid, else lo = mid;
 *        then zooms[f] = hi, status[f] = RSSYNC_ZOOM_CLEAR.
 * steps is 1 .. 40, 0 = the default: 12.  The result is defined by this procedure, not by an assumption that clear is
 * monotone in z: a host that runs the procedure through rssync_stabilize_coverage gets the same bits.  A frame with status
 * RSSYNC_ZOOM_CLEAR is clear at its zoom.  The whole bisection of a frame runs in one kernel, all frames in one pipeline
 * with one wait.
 *
 * The envelope.  For non-decreasing frame_times t, zooms z and a window in seconds, with
 * W(f) = { g : |t_g - t_f| <= window }:
 *   e[f] = max over W(f) of z[g];   k(d) = exp(-0.5 * (3 d / window)^2);
 *   s[f] = (sum over W(f), ascending g, of k(t_g - t_f) * e[g]) / (sum over W(f), ascending g, of k(t_g - t_f));
 *   out[f] = max(min(s[f], max over W(f) of e[g]), z[f]);   window == 0 copies z.
 * Every e[g] with g in W(f) is a maximum over a window that contains f, so s[f] >= z[f] up to rounding; the final max
 * makes out[f] >= z[f] exact: a frame that was clear at its fitted zoom is rendered at no smaller one.  A mean of the
 * e[g] cannot exceed the largest of them but by rounding either, which the min takes away: the envelope of a curve never
 * exceeds the curve's maximum, and equals it where every e[g] of the window does.  Host, fp64.
 *
 * The render.  rssync_zoom_stabilize is rssync_stabilize_frames with the output camera (fx * zooms[f], fy * zooms[f],
 * cx, cy) for frame f.  Frame f's bytes and n_outside[f] are those of rssync_stabilize_frames called on that frame alone
 * with params->zoom = zooms[f], byte for byte: both cameras, both filters, any output size, host or device memory,
 * pitched or not, however the call was chunked.  Grayscale (8-bit) frames.
 *
 * Errors, besides those of rssync_stabilize.h: zoom_lo, zoom_hi or a zooms[] entry <= 0 or non-finite; zoom_lo >=
 * zoom_hi; steps outside 0 .. 40; a negative or non-finite window; decreasing or non-finite frame times in
 * rssync_zoom_smooth.  Each returns non-zero and leaves the problem usable.
 */
#ifndef RSSYNC_ZOOM_H
#define RSSYNC_ZOOM_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"
#include "rssync_stabilize.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_ZOOM_CLEAR = 0, RSSYNC_ZOOM_NOT_CLEAR = 1 };

/* The smallest clear zoom of n_frames frames in [zoom_lo, zoom_hi]: zooms is n_frames doubles, status NULL or n_frames
 * values RSSYNC_ZOOM_* (both host).  frame_times, targets, params: as rssync_stabilize_coverage takes them. */
int rssync_zoom_fit(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                    const double* frame_times, size_t n_frames, double delay, const double* targets,
                    const rssync_stabilize_params* params, double zoom_lo, double zoom_hi, int32_t steps, double* zooms,
                    uint32_t* status);

/* The envelope of n zooms at non-decreasing frame_times (all host): out is n doubles and may be `zooms` itself.  p is
 * used for error reporting only: no device work is done. */
int rssync_zoom_smooth(rssync_problem* p, const double* frame_times, const double* zooms, size_t n, double window, double* out);

/* rssync_stabilize_frames with one zoom per frame: zooms is n_frames doubles (host). */
int rssync_zoom_stabilize(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                          size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                          const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                          size_t out_stride, uint64_t* n_outside, const double* zooms);

#ifdef __cplusplus
}
#endif
#endif
