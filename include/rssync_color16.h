/*
 * rssync_color16.h -- colour frames with 10- and 16-bit samples stabilised on the GPU: what rssync_color.h does for 8-bit
 * samples, for the layouts a decoder hands out for 10-bit video: P010 and P016 (hardware decoders), planar 10-bit I010
 * (yuv420p10le) and 16-bit gray.  Part of librssync_core.so; a separate header with one function.
 *
 * Everything that is not about the sample is rssync_color_stabilize's: the path and the targets, zoom and output camera, the
 * chroma camera and its siting, the iterations, host and device memory, chunking, the overlap rule, the meaning of
 * n_outside, rssync_color_image and rssync_color_params.  See rssync_color.h.
 *
 * Formats.  A sample is a native (little-endian) uint16 word; pitches and strides are bytes, as before.
 *   format   planes and geometry            sample value                     stored word    fill range
 *   GRAY16   GRAY8's                        the word                         value          0 .. 65535
 *   P010     NV12's (Y; interleaved U V)    word >> 6 (low six bits ignored) value << 6     0 .. 1023
 *   P016     NV12's                         the word                         value          0 .. 65535
 *   I010     I420's (yuv420p10le)           the word as written              value          0 .. 1023
 * Row widths in bytes are twice the 8-bit sibling's: GRAY16 2 W; P010 and P016 2 W (Y) and 2 W (UV, H / 2 rows); I010 2 W, W, W.
 * I010's words are taken as written: a word above 1023 is not masked, and the result lies within the range of its taps
 * (with the bilinear sampler only: see below).
 *
 * The map of a plane is the sibling format's rssync_color_map, bit for bit (ask it with RSSYNC_COLOR_GRAY8, _NV12 or _I420).
 * The inside test, the taps and the weights are the 8-bit sampler's; the blend is its three fp32 operations in its order on
 * the sample values, rounded to nearest even into uint16.  By monotone rounding the result never leaves the range of the
 * four taps.  U and V are sampled at the one position.  P010's output words have their low six bits zero.
 *
 * With params->stab.filter == RSSYNC_FILTER_BICUBIC (rssync_stabilize.h, "Sampling") the sixteen taps are blended on the
 * sample values -- P010's unpacked with >> 6 before and packed with << 6 after, as above -- and the kernel overshoots, so
 * the value is clamped to the format's range before it is rounded: 0 .. 65535 for GRAY16 and P016, 0 .. 1023 for P010 and
 * for I010.  I010's taps are still taken as written, but its result is then clamped to 1023 whatever they hold.
 *
 * Fill.  fill_set == 0: Y and gray get stab.fill << (depth - 8) (stab.fill still 0 .. 255), U and V 1 << (depth - 1), depth
 * 10 for P010 and I010 and 16 for GRAY16 and P016.  fill_set != 0: fill[] is used in the format's order (Y, U, V / gray) in
 * sample values within the table's range, and stab.fill is not read.  P010's fills are stored << 6 like any other value.
 *
 * Errors are rssync_color_stabilize's, and: a format outside 16 .. 19, the 8-bit formats included ("format"); a plane
 * pointer, a pitch or -- when n_frames > 1 -- a stride that is not a multiple of 2 ("alignment"); a pitch below the row bytes
 * above; a fill outside the format's range.  rssync_color_stabilize and rssync_color_map do not take these formats.
 */
#ifndef RSSYNC_COLOR16_H
#define RSSYNC_COLOR16_H

#include <stddef.h>
#include <stdint.h>

#include "rssync_color.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSSYNC_COLOR16_GRAY16 = 16, RSSYNC_COLOR16_P010 = 17, RSSYNC_COLOR16_P016 = 18, RSSYNC_COLOR16_I010 = 19 };

int rssync_color16_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                             const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                             const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                             uint64_t* n_outside);

#ifdef __cplusplus
}
#endif
#endif
