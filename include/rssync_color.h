/*
 * rssync_color.h -- colour frames stabilised on the GPU: what rssync_stabilize.h does for 8-bit grayscale, for the
 * layouts decoders hand out and viewers take: NV12, I420 (planar 4:2:0) and RGBA32, every plane of a frame rendered in
 * one pass.  Part of librssync_core.so; a separate header as rssync_stabilize.h is, whose conventions, parameters, path,
 * map and sampler these are.  Rectification in colour is rssync_color_stabilize with sigma = 0, default parameters and
 * the same size (rssync_stabilize.h's anchor).
 *
 * Plane 0 (Y, gray, RGBA) is rssync_stabilize_frames of that plane: same map, same bytes; RGBA has one position per
 * pixel and the sampler's arithmetic applies per channel.  params->stab.filter chooses the sampler of every plane and
 * channel (rssync_stabilize.h, "Sampling"): with RSSYNC_FILTER_BICUBIC the eight weights of a position are computed once
 * and shared by U and V and by R, G, B and A; every statement here that names rssync_stabilize_frames holds with that
 * filter in both calls.  rssync_color_map checks the field and does not depend on it.
 *
 * A 4:2:0 chroma plane is the image of a camera of its own.  Chroma sample (cu, cv) sits at luma position
 * (2 cu + ox, 2 cv + oy): RSSYNC_CHROMA_CENTER (ox, oy) = (0.5, 0.5), RSSYNC_CHROMA_LEFT (0, 0.5).  All of this in fp64:
 *   input lens      ro, fx * 0.5, fy * 0.5, (cx - ox) * 0.5, (cy - oy) * 0.5, k1 .. k4; the frame is width / 2 x height / 2
 *   frame time      T_c = T + ro * (oy / height); the row table has height / 2 + 1 entries q(T_c + ro * (j / (height / 2)) +
 *                   delay) against the target.  The check of the frame times stays the luma's; the table's last entry lies
 *                   ro * oy / height past the luma's last row: q() clamps it to the last knot, and its weight is 0.
 *   output camera   the luma's after defaults, scaling and zoom, (fx', fy', cx', cy'), as
 *                   (fx' * 0.5, fy' * 0.5, (cx' - ox) * 0.5, (cy' - oy) * 0.5), of size out_width / 2 x out_height / 2;
 *                   the start row's factor is (float)(height / 2) / (float)(out_height / 2)
 *   target          the luma's: the path's q_s at T + ro * 0.5 + delay, or the caller's: one target per frame for all planes
 * then the stabiliser's map, inside test (against the chroma plane's size) and sampler, unchanged; U and V are sampled at
 * the one position.  A chroma plane's result is what rssync_stabilize_frames gives for that plane as a gray frame with
 * the chroma lens, T_c, the chroma output camera and the luma's target, byte for byte.
 *
 * Layout.  Row widths in bytes: GRAY8 W; NV12 W (Y) and W (UV, interleaved U V pairs, H / 2 rows); I420 W, W / 2, W / 2;
 * RGBA32 4 W.  Memory is host memory or device memory of the problem's first device; all planes of `in` are of one kind
 * and all planes of `out` are of one kind.  Bytes of `out` between the rows are not written.  NV12 and I420: width,
 * height, out_width and out_height must be even and at least 4; GRAY8 and RGBA32: sizes as in the stabiliser.
 *
 * Fill.  fill_set == 0: Y, gray, R, G and B get stab.fill, U and V 128, A 255.  fill_set != 0: fill[] is used as written in
 * the order Y, U, V / R, G, B, A / gray, each 0 .. 255, and stab.fill is not read.
 *
 * Errors are the stabiliser's, and: a format or chroma site outside the enum; a NULL plane the format needs; a pitch below
 * the plane's row bytes; a stride below pitch x rows when n_frames > 1; odd or too small 4:2:0 sizes; a fill outside
 * 0 .. 255; any output plane overlapping any input plane; planes of mixed kinds; plane 1 asked of a single-plane format.
 */
#ifndef RSSYNC_COLOR_H
#define RSSYNC_COLOR_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_c.h"
#include "rssync_stabilize.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_COLOR_GRAY8 = 0, RSSYNC_COLOR_NV12 = 1, RSSYNC_COLOR_I420 = 2, RSSYNC_COLOR_RGBA32 = 3 };
enum { RSSYNC_CHROMA_CENTER = 0, RSSYNC_CHROMA_LEFT = 1 };

typedef struct rssync_color_image {
    uint8_t* plane[3];                  /* GRAY8: [0]; NV12: Y, UV; I420: Y, U, V; RGBA32: [0] */
    size_t pitch[3];                    /* bytes between rows */
    size_t stride[3];                   /* bytes between frames */
} rssync_color_image;

/* NULL or all zeros = all defaults */
typedef struct rssync_color_params {
    rssync_stabilize_params stab;
    int32_t chroma_site;                /* RSSYNC_CHROMA_CENTER or RSSYNC_CHROMA_LEFT */
    int32_t fill_set;                   /* 0: the fills follow stab.fill; else fill[] is used */
    int32_t fill[4];
} rssync_color_params;

/* Stabilise n_frames frames of `format`.  frame_times: n_frames times in seconds (host).  targets: n_frames x {w, x, y, z}
 * (host), or NULL = the path.  n_outside: NULL, or n_frames x 2 counts (host): the pixels of plane 0 that were filled, the
 * chroma samples that were filled (0 for GRAY8 and RGBA32). */
int rssync_color_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                           const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                           const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                           uint64_t* n_outside);

/* The source position of every output sample of a plane: plane 0 (luma or the only plane) is rssync_stabilize_map bit for
 * bit; plane 1 (NV12, I420) is out_height / 2 x out_width / 2 x {x, y} in chroma-plane coordinates.  map_xy: host or device
 * memory.  target: 4 doubles (host), or NULL = the path. */
int rssync_color_map(rssync_problem* p, int format, int plane, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                     size_t out_height, double frame_time, double delay, const double* target, const rssync_color_params* params,
                     float* map_xy);

#ifdef __cplusplus
}
#endif
#endif
