/*
 * zoom_hip.h -- the dynamic zoom's launchers in rssync_kernels.hip (kernels/zoom.hpp), called by zoom_api.cpp.  Internal
 * to librssync_core.so like stabilize_hip.h, whose configuration they take: cfg->cam holds the output camera at zoom 1
 * (as for rship_stabilize_coverage), the zooms come beside it.
 */
#ifndef RSSYNC_ZOOM_HIP_H
#define RSSYNC_ZOOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "stabilize_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zooms [n_frames], status [n_frames] or NULL (host): the bisection of include/rssync_zoom.h between lo and hi, `steps`
 * (1 .. 40) steps, one workgroup per frame.  One pipeline, one wait. */
int rship_zoom_fit(rship_ctx* c, const double* frame_times, uint32_t n_frames, const double* targets, const rship_stabilize_cfg* cfg,
                   double lo, double hi, int32_t steps, double* zooms, uint32_t* status);
/* rship_stabilize_frames with cam's fx, fy multiplied by zooms[f] (host, n_frames, finite and > 0) for frame f */
int rship_zoom_frames(rship_ctx* c, const uint8_t* frames, uint32_t n_frames, size_t pitch, size_t frame_stride,
                      const double* frame_times, const double* targets, const rship_stabilize_cfg* cfg, const double* zooms, uint8_t* out,
                      size_t out_pitch, size_t out_stride, uint64_t* n_outside, size_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
