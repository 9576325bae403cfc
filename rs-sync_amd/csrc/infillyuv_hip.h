/*
 * infillyuv_hip.h -- the launcher of the infill for 4:2:2 and 4:4:4 frames in rssync_kernels.hip (kernels/infillyuv.hpp),
 * called by infillyuv_api.cpp.  Internal to librssync_core.so like yuv_hip.h, whose configuration and images it takes:
 * cfg->luma.cam and cfg->chroma.cam hold the output cameras with the zoom applied, as for rship_yuv_frames.
 */
#ifndef RSSYNC_INFILLYUV_HIP_H
#define RSSYNC_INFILLYUV_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "color_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rship_yuv_frames with every sample whose source is outside its own frame's plane looked up in the frames f - 1, f + 1,
 * .., f - radius, f + radius of the call (radius 0 .. 8), in that order, per sample and per plane.  n_outside, n_borrowed:
 * NULL or n_frames x 2 (host): plane 0, chroma; 4:4:4: the first count twice.  A chunk of output frames needs its input
 * frames and `radius` more on each side: host planes are uploaded with that halo, device planes are read in place.
 * budget_bytes: 0 = the default; a chunk is at least one output frame with its halo. */
int rship_infillyuv_frames(rship_ctx* c, const rship_color_image* in, uint32_t n_frames, const double* frame_times, const double* targets,
                           const rship_color_cfg* cfg, const rship_color_image* out, uint64_t* n_outside, int32_t radius,
                           uint64_t* n_borrowed, size_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
