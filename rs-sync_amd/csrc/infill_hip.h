/*
 * infill_hip.h -- the infill's launcher in rssync_kernels.hip (kernels/infill.hpp), called by infill_api.cpp.  Internal to
 * librssync_core.so like stabilize_hip.h, whose configuration it takes: cfg->cam holds the output camera with the zoom
 * applied, as for rship_stabilize_frames.
 */
#ifndef RSSYNC_INFILL_HIP_H
#define RSSYNC_INFILL_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "stabilize_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rship_stabilize_frames with every pixel whose source is outside its own frame looked up in the frames f - 1, f + 1, ..,
 * f - radius, f + radius of the call (radius 0 .. 8), in that order.  n_borrowed: NULL or n_frames counts (host).  A chunk
 * of output frames needs its input frames and `radius` more on each side: host frames are uploaded with that halo, device
 * frames are read in place.  budget_bytes: 0 = the default; a chunk is at least one output frame with its halo. */
int rship_infill_frames(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                        const double* frame_times, const double* targets, const rship_stabilize_cfg* cfg, uint8_t* out,
                        size_t out_pitch, size_t out_stride, uint64_t* n_outside, int32_t radius, uint64_t* n_borrowed,
                        size_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
