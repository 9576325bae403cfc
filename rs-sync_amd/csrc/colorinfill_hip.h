/*
 * colorinfill_hip.h -- the colour infill's launcher in rssync_kernels.hip (kernels/colorinfill.hpp), called by
 * colorinfill_api.cpp.  Internal to librssync_core.so like color_hip.h, whose configuration and images it takes:
 * cfg->luma.cam and cfg->chroma.cam hold the output cameras with the zoom applied, as for rship_color_frames.
 */
#ifndef RSSYNC_COLORINFILL_HIP_H
#define RSSYNC_COLORINFILL_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "color_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rship_color_frames with every sample whose source is outside its own frame's plane looked up in the frames f - 1, f + 1,
 * .., f - radius, f + radius of the call (radius 0 .. 8), in that order, per sample and per plane.  n_outside, n_borrowed:
 * NULL or n_frames x 2 (host): plane 0, chroma.  A chunk of output frames needs its input frames and `radius` more on each
 * side: host planes are uploaded with that halo, device planes are read in place.  GRAY8 runs rship_infill_frames.
 * budget_bytes: 0 = the default; a chunk is at least one output frame with its halo. */
int rship_colorinfill_frames(rship_ctx* c, const rship_color_image* in, uint32_t n_frames, const double* frame_times, const double* targets,
                             const rship_color_cfg* cfg, const rship_color_image* out, uint64_t* n_outside, int32_t radius,
                             uint64_t* n_borrowed, size_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
