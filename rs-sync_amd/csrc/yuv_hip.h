/*
 * yuv_hip.h -- the launchers of the 4:2:2 and 4:4:4 formats in rssync_kernels.hip (kernels/yuv.hpp), called by yuv_api.cpp.
 * Internal to librssync_core.so and not in include/rssync_hip.h, for stabilize_hip.h's reason: only the product library
 * links yuv_api.cpp.
 */
#ifndef RSSYNC_YUV_HIP_H
#define RSSYNC_YUV_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "color_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rship_color_frames for include/rssync_yuv.h's formats (cfg->format 32 .. 34, 48 .. 51), every field resolved and checked
 * (yuv_api.cpp).  4:2:2: cfg->chroma is the chroma plane's size (width / 2 x height), lens and output camera; 4:4:4:
 * cfg->chroma is not read.  cfg->chroma_time is 0: a chroma plane's rows are the luma's.  n_outside: NULL or n_frames x 2
 * (host): filled pixels of plane 0, filled chroma samples (4:4:4: the same number again). */
int rship_yuv_frames(rship_ctx* c, const rship_color_image* in, uint32_t n_frames, const double* frame_times, const double* targets,
                     const rship_color_cfg* cfg, const rship_color_image* out, uint64_t* n_outside, size_t budget_bytes);
/* the source position of every output sample of plane 0 or 1 of one frame: map_xy [plane's out rows][plane's out cols]
 * {x, y}, host or device; 4:4:4: plane 1 is plane 0; target: 4 (host, unit) or NULL = the path */
int rship_yuv_map(rship_ctx* c, int plane, double frame_time, const double* target, const rship_color_cfg* cfg, float* map_xy);

#ifdef __cplusplus
}
#endif
#endif
