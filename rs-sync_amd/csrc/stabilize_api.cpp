// stabilize_api.cpp -- the public stabiliser entry points (include/rssync_stabilize.h): argument checks, defaults, the
// output camera, the caller's targets normalised, the check of a frame's row times against the gyro's knots.  The work
// runs in rship_stabilize_* (stabilize_hip.h).
//
// A file of its own, linked into the product library only, like rectify_api.cpp.
#include "../../include/rssync_c.h"
#include "../../include/rssync_stabilize.h"
#include "host_errors.hpp"
#include "stabilize_hip.h"
#include "stabilize_host.hpp"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;

using namespace rssync_stab_host;

extern "C" {

int rssync_stabilize_path(rssync_problem* p, const double* frame_times, size_t n, double ro, double delay, double sigma, double* quats) {
    return guarded([&] {
        if (n && !frame_times) panic("stabilize: no frame times");
        if (n && !quats) panic("stabilize: null output pointer");
        if (n > 0x7fffffffu) panic("stabilize: too many frames");
        check_sigma(sigma);
        rship_stabilize_cfg cfg{};
        resolve_gyro(p, ro, delay, cfg);
        cfg.sigma = sigma;
        for (size_t k = 0; k < n; ++k) check_frame_time(cfg, frame_times[k], k);
        rship_ctx* c = device(p);
        if (rship_stabilize_path(c, frame_times, n, &cfg, quats)) panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

int rssync_stabilize_map(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                         double frame_time, double delay, const double* target, const rssync_stabilize_params* params, float* map_xy) {
    return guarded([&] {
        if (!map_xy) panic("stabilize: null output pointer");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, false);
        check_frame_time(cfg, frame_time, 0);
        std::vector<double> unit;
        if (target) unit = unit_targets(target, 1);
        rship_ctx* c = device(p);
        if (rship_stabilize_map(c, frame_time, target ? unit.data() : nullptr, &cfg, map_xy)) panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

int rssync_stabilize_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                            size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                            const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                            size_t out_stride, uint64_t* n_outside) {
    return guarded([&] {
        if (!frames) panic("stabilize: no frames");
        if (!out) panic("stabilize: null output pointer");
        if (!frame_times) panic("stabilize: no frame times");
        if (n_frames > 0xffffffffu) panic("stabilize: too many frames");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, false);
        if (pitch < width) panic("stabilize: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
        if (out_pitch < out_width) panic("stabilize: out_pitch " + std::to_string(out_pitch) + " < out_width " + std::to_string(out_width));
        if (n_frames > 1 && (frame_stride < pitch * height || out_stride < out_pitch * out_height))
            panic("stabilize: frame stride smaller than pitch * height");
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        // the two extents, first to last byte
        const uintptr_t a0 = (uintptr_t)frames, a1 = a0 + (n_frames - 1) * frame_stride + (height - 1) * pitch + width;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (n_frames - 1) * out_stride + (out_height - 1) * out_pitch + out_width;
        if (a0 < b1 && b0 < a1) panic("stabilize: out overlaps the frames");
        rship_ctx* c = device(p);
        if (rship_stabilize_frames(c, frames, (uint32_t)n_frames, pitch, frame_stride, frame_times, targets ? unit.data() : nullptr, &cfg, out,
                                   out_pitch, out_stride, n_outside, 0))
            panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

int rssync_stabilize_coverage(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                              const double* frame_times, size_t n_frames, double delay, const double* targets,
                              const rssync_stabilize_params* params, const double* zooms, size_t n_zooms, uint32_t* outside) {
    return guarded([&] {
        if (!frame_times) panic("stabilize: no frame times");
        if (!zooms) panic("stabilize: no zooms");
        if (!outside) panic("stabilize: null output pointer");
        if (n_frames > 0xffffffffu) panic("stabilize: too many frames");
        if (n_zooms > 65535) panic("stabilize: more than 65535 zooms in one sweep");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, true);
        for (size_t z = 0; z < n_zooms; ++z) check_zoom(zooms[z], "every zoom of the sweep");
        if (!n_frames || !n_zooms) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        rship_ctx* c = device(p);
        if (rship_stabilize_coverage(c, frame_times, (uint32_t)n_frames, targets ? unit.data() : nullptr, &cfg, zooms, (uint32_t)n_zooms, outside))
            panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

} // extern "C"
