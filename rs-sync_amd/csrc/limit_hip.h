/*
 * limit_hip.h -- the path limiter's launcher in rssync_kernels.hip (kernels/limit.hpp), called by limit_api.cpp.  Internal
 * to librssync_core.so like zoom_hip.h, whose configuration it takes: cfg->cam holds the output camera at zoom 1, the
 * zooms come beside it, one per frame.
 */
#ifndef RSSYNC_LIMIT_HIP_H
#define RSSYNC_LIMIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "stabilize_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* strengths [n_frames], status [n_frames] or NULL (host): the bisection of include/rssync_limit.h, `steps` (1 .. 40) steps,
 * one workgroup per frame.  targets: n_frames x 4 as the caller gave them (not normalised; finite and not zero), or NULL =
 * the path at cfg->sigma.  zooms: n_frames (host, finite and > 0).  One pipeline, one wait. */
int rship_limit_fit(rship_ctx* c, const double* frame_times, uint32_t n_frames, const double* targets, const rship_stabilize_cfg* cfg,
                    const double* zooms, int32_t steps, double* strengths, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
