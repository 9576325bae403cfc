/*
 * colorzoom_hip.h -- the launcher of colour frames with one zoom per frame in rssync_kernels.hip (kernels/colorzoom.hpp),
 * called by colorzoom_api.cpp.  Internal to librssync_core.so like color_hip.h, whose configuration and images it takes:
 * cfg->luma.cam and cfg->chroma.cam hold the output cameras at zoom 1, the zooms come beside them.
 */
#ifndef RSSYNC_COLORZOOM_HIP_H
#define RSSYNC_COLORZOOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "color_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rship_color_frames with both cameras' fx, fy multiplied by zooms[f] (host, n_frames, finite and > 0) for frame f: its
 * memory rules, chunk pipeline, counts and budget.  GRAY8 runs rship_zoom_frames' kernels. */
int rship_colorzoom_frames(rship_ctx* c, const rship_color_image* in, uint32_t n_frames, const double* frame_times, const double* targets,
                           const rship_color_cfg* cfg, const double* zooms, const rship_color_image* out, uint64_t* n_outside,
                           size_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
