// zoom_api.cpp -- the public entry points of the dynamic zoom (include/rssync_zoom.h): argument checks and defaults, which
// are the stabiliser's (stabilize_host.hpp), the envelope on the host (zoom_math.hpp).  The device work runs in
// rship_zoom_* (zoom_hip.h).
//
// A file of its own, linked into the product library only, like stabilize_api.cpp.
#include "../../include/rssync_c.h"
#include "../../include/rssync_zoom.h"
#include "host_errors.hpp"
#include "stabilize_host.hpp"
#include "zoom_hip.h"
#include "zoom_math.hpp"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;

using namespace rssync_stab_host;

static_assert(RSSYNC_ZOOM_CLEAR == (int)rs::kZoomClear && RSSYNC_ZOOM_NOT_CLEAR == (int)rs::kZoomNotClear, "status values moved");

extern "C" {

int rssync_zoom_fit(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                    const double* frame_times, size_t n_frames, double delay, const double* targets,
                    const rssync_stabilize_params* params, double zoom_lo, double zoom_hi, int32_t steps, double* zooms,
                    uint32_t* status) {
    return guarded([&] {
        if (!frame_times) panic("zoom: no frame times");
        if (!zooms) panic("zoom: null output pointer");
        if (n_frames > 0xffffffffu) panic("zoom: too many frames");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, true);
        check_zoom(zoom_lo, "zoom_lo");
        check_zoom(zoom_hi, "zoom_hi");
        if (!(zoom_lo < zoom_hi)) panic("zoom: zoom_lo must be below zoom_hi");
        if (steps < 0 || steps > rs::kZoomMaxSteps) panic("zoom: steps must be 0 .. " + std::to_string(rs::kZoomMaxSteps));
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        rship_ctx* c = device(p);
        if (rship_zoom_fit(c, frame_times, (uint32_t)n_frames, targets ? unit.data() : nullptr, &cfg, zoom_lo, zoom_hi,
                           steps ? steps : rs::kZoomDefaultSteps, zooms, status))
            panic(std::string("hip: zoom: ") + rship_last_error(c));
    });
}

int rssync_zoom_smooth(rssync_problem* p, const double* frame_times, const double* zooms, size_t n, double window, double* out) {
    return guarded([&] {
        if (!p) panic("zoom: no problem");
        if (!std::isfinite(window) || window < 0) panic("zoom: window must be finite and >= 0");
        if (!n) return;
        if (!frame_times) panic("zoom: no frame times");
        if (!zooms) panic("zoom: no zooms");
        if (!out) panic("zoom: null output pointer");
        for (size_t k = 0; k < n; ++k) {
            if (!std::isfinite(frame_times[k])) panic("zoom: non-finite frame time at " + std::to_string(k));
            if (k && frame_times[k] < frame_times[k - 1]) panic("zoom: frame times must not decrease (at " + std::to_string(k) + ")");
            check_zoom(zooms[k], "every zoom of the curve");
        }
        std::vector<double> e(n), res(n); // (out may be zooms)
        rs::zoom_smooth(frame_times, zooms, n, window, e.data(), res.data());
        for (size_t k = 0; k < n; ++k) out[k] = res[k];
    });
}

int rssync_zoom_stabilize(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                          size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                          const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                          size_t out_stride, uint64_t* n_outside, const double* zooms) {
    return guarded([&] {
        // rssync_stabilize_frames' checks, in its order
        if (!frames) panic("stabilize: no frames");
        if (!out) panic("stabilize: null output pointer");
        if (!frame_times) panic("stabilize: no frame times");
        if (!zooms) panic("zoom: no zooms");
        if (n_frames > 0xffffffffu) panic("stabilize: too many frames");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, true);
        if (pitch < width) panic("stabilize: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
        if (out_pitch < out_width) panic("stabilize: out_pitch " + std::to_string(out_pitch) + " < out_width " + std::to_string(out_width));
        if (n_frames > 1 && (frame_stride < pitch * height || out_stride < out_pitch * out_height))
            panic("stabilize: frame stride smaller than pitch * height");
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) {
            check_frame_time(cfg, frame_times[k], k);
            check_zoom(zooms[k], "every zoom of the frames");
        }
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const uintptr_t a0 = (uintptr_t)frames, a1 = a0 + (n_frames - 1) * frame_stride + (height - 1) * pitch + width;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (n_frames - 1) * out_stride + (out_height - 1) * out_pitch + out_width;
        if (a0 < b1 && b0 < a1) panic("stabilize: out overlaps the frames");
        rship_ctx* c = device(p);
        if (rship_zoom_frames(c, frames, (uint32_t)n_frames, pitch, frame_stride, frame_times, targets ? unit.data() : nullptr, &cfg, zooms, out,
                              out_pitch, out_stride, n_outside, 0))
            panic(std::string("hip: zoom: ") + rship_last_error(c));
    });
}

} // extern "C"
