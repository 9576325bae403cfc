// infill_api.cpp -- the public entry point of the infill (include/rssync_infill.h): argument checks and defaults, which are
// the stabiliser's (stabilize_host.hpp), and the radius.  The device work runs in rship_infill_frames (infill_hip.h).
//
// A file of its own, linked into the product library only, like stabilize_api.cpp.
#include "../../include/rssync_c.h"
#include "../../include/rssync_infill.h"
#include "host_errors.hpp"
#include "infill_hip.h"
#include "infill_math.hpp"
#include "stabilize_host.hpp"

#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;

using namespace rssync_stab_host;

static_assert(RSSYNC_INFILL_MAX_RADIUS == rs::kInfillMaxRadius, "the largest radius moved");

static void check_radius(int32_t radius) {
    if (radius < 0 || radius > rs::kInfillMaxRadius)
        panic("infill: radius " + std::to_string(radius) + " must be 0 .. " + std::to_string(rs::kInfillMaxRadius));
}

extern "C" {

int rssync_infill_stabilize(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                            size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                            const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                            size_t out_stride, uint64_t* n_outside, int32_t radius, uint64_t* n_borrowed) {
    return guarded([&] {
        // rssync_stabilize_frames' checks, in its order
        if (!frames) panic("stabilize: no frames");
        if (!out) panic("stabilize: null output pointer");
        if (!frame_times) panic("stabilize: no frame times");
        if (n_frames > 0xffffffffu) panic("stabilize: too many frames");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, false);
        if (pitch < width) panic("stabilize: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
        if (out_pitch < out_width) panic("stabilize: out_pitch " + std::to_string(out_pitch) + " < out_width " + std::to_string(out_width));
        if (n_frames > 1 && (frame_stride < pitch * height || out_stride < out_pitch * out_height))
            panic("stabilize: frame stride smaller than pitch * height");
        if (!n_frames) {
            check_radius(radius);
            return;
        }
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const uintptr_t a0 = (uintptr_t)frames, a1 = a0 + (n_frames - 1) * frame_stride + (height - 1) * pitch + width;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (n_frames - 1) * out_stride + (out_height - 1) * out_pitch + out_width;
        if (a0 < b1 && b0 < a1) panic("stabilize: out overlaps the frames");
        check_radius(radius);
        rship_ctx* c = device(p);
        if (rship_infill_frames(c, frames, (uint32_t)n_frames, pitch, frame_stride, frame_times, targets ? unit.data() : nullptr, &cfg, out,
                                out_pitch, out_stride, n_outside, radius, n_borrowed, 0))
            panic(std::string("hip: infill: ") + rship_last_error(c));
    });
}

} // extern "C"
