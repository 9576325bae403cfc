/*
 * zoomyuv_hip.h -- the launcher of 4:2:2 and 4:4:4 frames with one zoom per frame in rssync_kernels.hip
 * (kernels/zoomyuv.hpp), called by zoomyuv_api.cpp.  Internal to librssync_core.so like yuv_hip.h, whose configuration and
 * images it takes: cfg->luma.cam and cfg->chroma.cam hold the output cameras at zoom 1, the zooms come beside them.
 */
#ifndef RSSYNC_ZOOMYUV_HIP_H
#define RSSYNC_ZOOMYUV_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "color_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rship_yuv_frames with the luma camera's fx, fy multiplied by zooms[f] (host, n_frames, finite and > 0) for frame f and the
 * 4:2:2 chroma camera that belongs to it (that fx halved, that fy): its formats, memory rules, chunk pipeline, counts and
 * budget. */
int rship_zoomyuv_frames(rship_ctx* c, const rship_color_image* in, uint32_t n_frames, const double* frame_times, const double* targets,
                         const rship_color_cfg* cfg, const double* zooms, const rship_color_image* out, uint64_t* n_outside,
                         size_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
