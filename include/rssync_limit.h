/*
 * rssync_limit.h -- the path limited to a zoom: given the zoom the caller is willing to pay, how far every frame may
 * follow its goal -- the smoothed path or the caller's targets -- without showing a border; that curve smoothed into a
 * lower envelope; and the targets that result, which every renderer of the library takes unchanged.  The opposite of
 * rssync_zoom.h, which finds the zoom a given path needs.  Part of librssync_core.so; a separate header as
 * rssync_stabilize.h is, whose conventions, parameters, defaults, output camera, targets and errors these are.
 *
 * Definitions.  For frame f with time T:
 *   r_f   the frame's own orientation: what rssync_stabilize_path(..., sigma = 0) returns for it;
 *   g_f   the goal: the caller's targets[f] as given, or what rssync_stabilize_path(..., sigma = params->sigma) returns
 *         where targets == NULL;
 *   c_f(a), the candidate target at strength a in [0, 1]:
 *         c_f(0) = r_f and c_f(1) = g_f, copied, not computed;
 *         for 0 < a < 1, with d = ((r.w g.w + r.x g.x) + r.y g.y) + r.z g.z and s = d < 0 ? -1 : 1, every component is
 *         (1 - a) * r_i + (s * a) * g_i: five fp64 operations, each rounded on its own.  It is not normalised: every entry
 *         point of the library normalises a target once, with a division by its norm, and so does the fit;
 *   z_f   zooms[f], or params->zoom (0 = 1) where zooms == NULL;
 *   clear(f, a) means: rssync_stabilize_coverage of frame f alone, with the explicit target c_f(a) and zooms = { z_f },
 *         returns 0.
 *
 * The fit, per frame:
 *   clear(f, 1):          strengths[f] = 1, status[f] = RSSYNC_LIMIT_CLEAR;
 *   else not clear(f, 0): strengths[f] = 0, status[f] = RSSYNC_LIMIT_NOT_CLEAR: the frame shows a border even without
 *                         smoothing at this zoom;
 *   else lo = 0, hi = 1 and `steps` times: mid = 0.5 * (lo + hi); if clear(f, mid) lo = mid, else hi = mid;
 *        then strengths[f] = lo, status[f] = RSSYNC_LIMIT_CLEAR.
 * steps is 1 .. 40, 0 = the default: 12.  The result is defined by this procedure, not by an assumption that clear is
 * monotone in a: a host that runs the procedure through rssync_stabilize_path and rssync_stabilize_coverage gets the same
 * bits.  A frame with status RSSYNC_LIMIT_CLEAR is clear at its strength.  The whole bisection of a frame runs in one
 * kernel, which rebuilds the frame's row table for every candidate; all frames in one pipeline with one wait.
 *
 * WHAT IS GUARANTEED.  A frame is guaranteed clear only AT its fitted strength.  Below it -- where rssync_limit_smooth
 * puts it -- the frame is clear wherever clear(f, .) is monotone, which it was on every frame tried, but which nothing
 * here proves.  A caller that must know runs rssync_stabilize_coverage once with the targets of rssync_limit_targets.
 *
 * The envelope.  rssync_zoom_smooth mirrored, with its W(f) = { g : |t_g - t_f| <= window } and its
 * k(d) = exp(-0.5 * (3 d / window)^2), for strengths a:
 *   e[f] = min over W(f) of a[g];
 *   s[f] = (sum over W(f), ascending g, of k(t_g - t_f) * e[g]) / (sum over W(f), ascending g, of k(t_g - t_f));
 *   out[f] = min(max(s[f], min over W(f) of e[g]), a[f]);   window == 0 copies a.
 * The output never exceeds a frame's fitted strength and never falls below the curve's minimum.  Host, fp64.
 *
 * The targets.  rssync_limit_targets returns c_f(strengths[f]) for every frame, to be passed as `targets` to
 * rssync_stabilize_frames, _map, _coverage, rssync_zoom_*, rssync_color_*, rssync_color16_* or rssync_colorzoom_*.  With
 * all strengths 1 these are the goal's bits, so a render with them is the render with the goal as explicit targets, byte
 * for byte; with all strengths 0 they are rssync_stabilize_path at sigma 0, with default parameters the rectifier's anchor.
 *
 * Errors, besides those of rssync_stabilize.h and rssync_zoom.h: a strength outside [0, 1] or non-finite; steps outside
 * 0 .. 40; a zooms[] entry <= 0 or non-finite; null outputs; a negative or non-finite window; decreasing or non-finite
 * frame times in rssync_limit_smooth.  Each returns non-zero and leaves the problem usable.
 */
#ifndef RSSYNC_LIMIT_H
#define RSSYNC_LIMIT_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"
#include "rssync_stabilize.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_LIMIT_CLEAR = 0, RSSYNC_LIMIT_NOT_CLEAR = 1 };

/* The largest clear strength of n_frames frames: zooms is NULL or n_frames doubles, strengths n_frames doubles, status NULL
 * or n_frames values RSSYNC_LIMIT_* (all host).  frame_times, targets, params: as rssync_stabilize_coverage takes them,
 * but params->zoom is read where zooms == NULL. */
int rssync_limit_fit(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                     const double* frame_times, size_t n_frames, double delay, const double* targets,
                     const rssync_stabilize_params* params, const double* zooms, int32_t steps, double* strengths, uint32_t* status);

/* The lower envelope of n strengths at non-decreasing frame_times (all host): out is n doubles and may be `strengths`
 * itself.  p is used for error reporting only: no device work is done. */
int rssync_limit_smooth(rssync_problem* p, const double* frame_times, const double* strengths, size_t n, double window, double* out);

/* c_f(strengths[f]) for every frame: out_targets is n_frames x {w, x, y, z} (host).  ro, delay: as rssync_stabilize_path
 * takes them; targets: NULL or n_frames x 4, the goals; sigma: the goal's where targets == NULL. */
int rssync_limit_targets(rssync_problem* p, const double* frame_times, size_t n_frames, double ro, double delay, const double* targets,
                         double sigma, const double* strengths, double* out_targets);

#ifdef __cplusplus
}
#endif
#endif
