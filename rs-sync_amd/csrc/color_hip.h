/*
 * color_hip.h -- the colour front's launchers in rssync_kernels.hip (kernels/color.hpp, kernels/color16.hpp), called by
 * color_api.cpp.
 * Internal to librssync_core.so and not in include/rssync_hip.h, for stabilize_hip.h's reason: only the product library
 * links color_api.cpp.
 */
#ifndef RSSYNC_COLOR_HIP_H
#define RSSYNC_COLOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "stabilize_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* include/rssync_color.h's rssync_color_image; 16-bit formats: pointers, pitches and strides are multiples of 2 */
typedef struct rship_color_image {
    uint8_t* plane[3];
    size_t pitch[3];
    size_t stride[3];
} rship_color_image;

/* every field resolved and checked (color_api.cpp) */
typedef struct rship_color_cfg {
    rship_stabilize_cfg luma;   /* plane 0, or the only plane: the stabiliser's configuration of the call (fill unused) */
    rship_stabilize_cfg chroma; /* 4:2:0: the chroma plane's size, lens and output camera; everything else as in luma */
    double chroma_time;         /* 4:2:0: ro * (oy / height), what a chroma plane's frame time lies after the frame's */
    int32_t format;             /* RSSYNC_COLOR_* or RSSYNC_COLOR16_* */
    int32_t fill[4];            /* per channel: Y, U, V / R, G, B, A / gray; 0 .. 255, 16-bit formats: sample values, 0 .. 1023
                                   (P010, I010) or 0 .. 65535 (GRAY16, P016), and luma.fill is not read */
} rship_color_cfg;

/* Stabilise n_frames colour frames: rship_stabilize_frames' memory rules and chunking, every plane of `in` of one kind
 * (host or this device) and every plane of `out` of one kind.  n_outside: NULL or n_frames x 2 (host): filled pixels of
 * plane 0, filled chroma samples.  budget_bytes: device bytes for the two chunk slots, 0 = the library's fixed budget. */
int rship_color_frames(rship_ctx* c, const rship_color_image* in, uint32_t n_frames, const double* frame_times, const double* targets,
                       const rship_color_cfg* cfg, const rship_color_image* out, uint64_t* n_outside, size_t budget_bytes);
/* the source position of every output sample of one plane of one frame (plane 0 or, 4:2:0, 1): map_xy
 * [plane's out rows][plane's out cols]{x, y}, host or device; target: 4 (host, unit) or NULL = the path */
int rship_color_map(rship_ctx* c, int plane, double frame_time, const double* target, const rship_color_cfg* cfg, float* map_xy);

#ifdef __cplusplus
}
#endif
#endif
