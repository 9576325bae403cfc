// infill_math.hpp -- the one thing the infill (include/rssync_infill.h) has that the stabiliser does not: the order in which
// the frames of a call are asked for an output pixel of frame f.  Plain C++ for the host and the device (RS_LHD); compiled
// for the CPU by tests/cpu_device/infill_math_check.cpp.
//
//   order   step 0 is f itself; step 2 d - 1 is f - d and step 2 d is f + d, for d = 1 .. radius.  A step whose frame is
//           not one of 0 .. n_frames - 1 is skipped; the candidates are the steps that remain, in that order.
//
// The rows kernel finds the k-th candidate of a frame with infill_candidate, the render kernel walks the steps itself
// (infill_step_frame, infill_is_frame) with the candidate's table as a running pointer, and infill_candidates lists them
// for the CPU check: all read the order from here.  (The launcher needs only the span of a chunk's candidates, which is
// f0 - radius .. f0 + cnt - 1 + radius clipped to the call.)
#pragma once

#include <stdint.h>

#include "lens_math.hpp"

namespace rs {

constexpr int kInfillMaxRadius = 8;
constexpr int kInfillMaxCandidates = 2 * kInfillMaxRadius + 1;

// the frame of a step of the order, before the skip: may lie outside the call
RS_LHD int64_t infill_step_frame(int64_t f, int step) {
    const int64_t d = (step + 1) >> 1;
    return (step & 1) ? f - d : f + d;
}

RS_LHD bool infill_is_frame(int64_t g, int64_t n_frames) { return g >= 0 && g < n_frames; }

// the candidates of frame f in order -> their count; out holds kInfillMaxCandidates entries (2 radius + 1 are enough)
RS_LHD int infill_candidates(int64_t f, int64_t n_frames, int radius, int64_t* out) {
    int count = 0;
    for (int step = 0; step <= 2 * radius; ++step) {
        const int64_t g = infill_step_frame(f, step);
        if (infill_is_frame(g, n_frames)) out[count++] = g;
    }
    return count;
}

// the k-th candidate of frame f, -1 where it has fewer than k + 1
RS_LHD int64_t infill_candidate(int64_t f, int64_t n_frames, int radius, int k) {
    for (int step = 0; step <= 2 * radius; ++step) {
        const int64_t g = infill_step_frame(f, step);
        if (infill_is_frame(g, n_frames) && k-- == 0) return g;
    }
    return -1;
}

} // namespace rs
