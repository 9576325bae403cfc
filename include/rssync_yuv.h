/*
 * rssync_yuv.h -- 4:2:2 and 4:4:4 video stabilised on the GPU: what rssync_color.h and rssync_color16.h do for the 4:2:0
 * layouts, for the layouts mirrorless and cinema cameras, capture cards and intermediate codecs give: I422, NV16 and I444
 * with 8-bit samples, I210 (yuv422p10le), P210, P216 and I410 (yuv444p10le) in 16-bit containers.  Every plane of a frame
 * is rendered in one pass.  Part of librssync_core.so; a separate header with two functions whose signatures are
 * rssync_color_stabilize's and rssync_color_map's.
 *
 * Everything that is not about the chroma plane's geometry is the colour front's, unchanged: rssync_color_image,
 * rssync_color_params, the path and the targets, the zoom and the output camera, the iterations, both samplers
 * (params->stab.filter), host and device memory, the chunking and the overlap rule.  See rssync_color.h, and
 * rssync_color16.h for the samples in 16-bit containers.
 *
 * Formats.  These numbers go through this header's functions, rssync_zoomyuv.h's (a zoom per frame) and rssync_infillyuv.h's alone:
 * rssync_color_*, rssync_color16_*, rssync_colorzoom_* and rssync_colorinfill_* turn them away, and these functions turn
 * every other number away.  Row widths are in bytes; every plane has H rows.
 *   format                planes              row bytes        sample and container
 *   I422                  Y, U, V             W, W / 2, W / 2  8-bit
 *   NV16                  Y, interleaved U V  W, W             8-bit
 *   I444                  Y, U, V             W, W, W          8-bit
 *   I210 (yuv422p10le)    I422's              twice I422's     10-bit, the word as written (I010's rules, its bicubic clamp to
 *                                                              1023 included)
 *   P210                  NV16's              twice NV16's     10-bit, value = word >> 6, stored word = value << 6 (P010's)
 *   P216                  NV16's              twice NV16's     16-bit
 *   I410 (yuv444p10le)    I444's              twice I444's     10-bit, the word as written
 * The fill defaults and ranges follow rssync_color16.h's table by depth (8 bits: rssync_color.h's; U and V get
 * 1 << (depth - 1)); the formats in 16-bit containers need pointers, pitches and -- when n_frames > 1 -- strides that are
 * multiples of 2 ("alignment").
 *
 * The 4:2:2 chroma plane is the image of a camera of its own.  Chroma sample (cu, cv) sits at luma position
 * (2 cu + ox, cv): RSSYNC_CHROMA_CENTER ox = 0.5, RSSYNC_CHROMA_LEFT ox = 0; there is no vertical offset.  All of this in fp64:
 *   input lens      ro, fx * 0.5, fy, (cx - ox) * 0.5, cy, k1 .. k4; the plane is width / 2 x height
 *   frame time      T itself; the row table has height + 1 entries and is the luma's bit for bit (same rows, time and target)
 *   output camera   the luma's after defaults, scaling and zoom, (fx', fy', cx', cy'), as (fx' * 0.5, fy', (cx' - ox) * 0.5, cy'),
 *                   of size out_width / 2 x out_height; the start row's factor is the luma's
 *   target          the luma's
 * 4:4:4: all three planes share the luma's camera and one position per pixel; chroma_site is checked and otherwise not read.
 *
 * With explicit targets every plane is what rssync_stabilize_frames gives for that plane as a gray frame -- with the
 * chroma lens, T, the chroma output camera and the frame's target --, byte for byte: the counts, both cameras and both
 * samplers.  NV16's chroma is I422's, interleaved.  A format in a 16-bit container on 8-bit values is its 8-bit sibling
 * widened (P210: << 6), as rssync_color16.h's formats are.
 *
 * Sizes.  4:2:2: width and out_width even and at least 4; the heights follow the stabiliser's rule (at least 2, odd
 * allowed).  4:4:4: the stabiliser's rules.
 *
 * n_outside: NULL, or n_frames x 2 counts (host): the pixels of plane 0 that were filled, the chroma samples (of one chroma
 * plane) that were filled.  For 4:4:4 the second count equals the first.
 *
 * A zoom that clears a 4:2:2 chroma plane is rssync_zoom_fit (rssync_zoom.h) on that plane's camera as given above.
 *
 * Errors are the colour front's: a format outside the enum below ("format"); an odd or too small 4:2:2 width ("even"); a
 * misaligned plane of 16-bit samples ("alignment"); a NULL plane the format needs ("is NULL"); a pitch below the row bytes
 * ("pitch"); a fill outside the format's range ("fill"); a chroma site outside its enum ("chroma_site"); a plane other than
 * 0 or 1 asked of rssync_yuv_map ("plane").  The problem stays usable after an error.
 *
 * Not here: packed 4:2:2 (YUY2, UYVY, v210); 4:4:4 at 16 bits beyond I410.  A zoom per frame: rssync_zoomyuv.h.  The
 * borders filled from neighbouring frames: rssync_infillyuv.h.
 */
#ifndef RSSYNC_YUV_H
#define RSSYNC_YUV_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_color.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_YUV_I422 = 32, RSSYNC_YUV_NV16 = 33, RSSYNC_YUV_I444 = 34,
       RSSYNC_YUV_I210 = 48, RSSYNC_YUV_P210 = 49, RSSYNC_YUV_P216 = 50, RSSYNC_YUV_I410 = 51 };

/* rssync_color_stabilize for the formats above */
int rssync_yuv_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                         const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                         const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                         uint64_t* n_outside);

/* The source position of every output sample of a plane: plane 0 is rssync_stabilize_map bit for bit; plane 1 of a 4:2:2
 * format is out_height x out_width / 2 x {x, y} in chroma-plane coordinates; plane 1 of a 4:4:4 format is plane 0.  map_xy:
 * host or device memory.  target: 4 doubles (host), or NULL = the path. */
int rssync_yuv_map(rssync_problem* p, int format, int plane, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                   size_t out_height, double frame_time, double delay, const double* target, const rssync_color_params* params,
                   float* map_xy);

#ifdef __cplusplus
}
#endif
#endif
