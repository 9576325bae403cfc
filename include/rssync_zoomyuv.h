/*
 * rssync_zoomyuv.h -- the dynamic zoom for 4:2:2 and 4:4:4 video: every format of rssync_yuv.h rendered with one zoom per
 * frame, and a zoom per frame fitted so that every plane is clear, the 4:2:2 chroma plane included.  Part of
 * librssync_core.so; a separate header as rssync_colorzoom.h is, whose two signatures these functions have.  Conventions,
 * formats, parameters, defaults, output cameras, targets, fills and errors are those of rssync_yuv.h and rssync_zoom.h.  In
 * both functions `format` is one of RSSYNC_YUV_* and params->stab.zoom is not read, as in rssync_zoom_stabilize.  The
 * resulting curve is smoothed with rssync_zoom_smooth, unchanged.
 *
 * The render.  rssync_zoomyuv_stabilize is rssync_yuv_stabilize with the luma output camera (fx * zooms[f], fy * zooms[f],
 * cx, cy) for frame f, and the chroma camera that belongs to it (rssync_yuv.h: that fx halved, that fy).  Frame f's bytes in
 * every plane are those of rssync_yuv_stabilize called on that frame alone with params->stab.zoom = zooms[f], and the
 * frame's two n_outside counts are that call's too.  This holds byte for byte: both cameras, both filters, both chroma
 * sites, default and explicit fills, host or device memory, pitched or not, any output size, however the call was chunked.
 * Bytes between the rows of `out` are not written.  For 4:4:4 the second count equals the first.
 *
 * The fit.  The result is defined by this procedure, which a host can run through rssync_zoom_fit and
 * rssync_stabilize_path and get the same bits:
 *   1. zL, sL = rssync_zoom_fit of plane 0: width x height, lens, out_width x out_height, frame_times, targets,
 *      params->stab.
 *   2. the 4:2:2 formats (I422, NV16, I210, P210, P216): zC, sC = rssync_zoom_fit of the chroma plane as the camera of its
 *      own that rssync_yuv.h describes, in that header's operations: the chroma lens; the size (width / 2) x height; the
 *      output size (out_width / 2) x out_height; the frame times T themselves (there is no vertical offset); params->stab
 *      with the chroma output camera at zoom 1 given as fx, fy, cx, cy.
 *   3. the targets of step 2 are the caller's.  When the caller's are NULL they are the quaternions that
 *      rssync_stabilize_path(frame_times, n_frames, ro, delay, sigma) returns, passed as explicit targets: all planes of a
 *      frame are held against the frame's one target.
 *   4. the check of the frame times against the gyro data is the luma's alone.
 *   5. zooms[f] = max(zL[f], zC[f]), status[f] = sL[f] | sC[f].
 *   6. the 4:4:4 formats (I444, I410), whose planes share one camera, return step 1.
 * A frame with status RSSYNC_ZOOM_CLEAR is clear in the plane that set its zoom at that zoom, and in the other plane at
 * that plane's own, smaller, fitted zoom.
 *
 * Errors, besides those of rssync_yuv_stabilize and of rssync_zoom_fit: zooms is NULL ("no zooms"); an entry of zooms is
 * <= 0 or non-finite ("zoom"); a format that is none of RSSYNC_YUV_* ("format").  Each returns non-zero and leaves the
 * problem usable.
 *
 * Not here: the infill for these formats.
 */
#ifndef RSSYNC_ZOOMYUV_H
#define RSSYNC_ZOOMYUV_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_yuv.h"
#include "rssync_zoom.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rssync_yuv_stabilize with one zoom per frame: format is any of RSSYNC_YUV_*, zooms is n_frames doubles (host), n_outside
 * NULL or n_frames x 2 values (host). */
int rssync_zoomyuv_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                             const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                             const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                             uint64_t* n_outside, const double* zooms);

/* The smallest zoom of n_frames frames in [zoom_lo, zoom_hi] that clears every plane of the format: zooms is n_frames
 * doubles, status NULL or n_frames values RSSYNC_ZOOM_* (both host); steps 1 .. 40, 0 = 12. */
int rssync_zoomyuv_fit(rssync_problem* p, int format, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                       size_t out_height, const double* frame_times, size_t n_frames, double delay, const double* targets,
                       const rssync_color_params* params, double zoom_lo, double zoom_hi, int32_t steps, double* zooms,
                       uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
