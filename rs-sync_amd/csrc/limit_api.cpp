// limit_api.cpp -- the public entry points of the path limiter (include/rssync_limit.h): argument checks and defaults,
// which are the stabiliser's (stabilize_host.hpp), the envelope and the blend on the host (limit_math.hpp).  The device work
// runs in rship_limit_fit (limit_hip.h) and rship_stabilize_path.
//
// A file of its own, linked into the product library only, like zoom_api.cpp.
#include "../../include/rssync_c.h"
#include "../../include/rssync_limit.h"
#include "host_errors.hpp"
#include "limit_hip.h"
#include "limit_math.hpp"
#include "stabilize_host.hpp"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;

using namespace rssync_stab_host;

static_assert(RSSYNC_LIMIT_CLEAR == (int)rs::kLimitClear && RSSYNC_LIMIT_NOT_CLEAR == (int)rs::kLimitNotClear, "status values moved");

namespace {

void check_strength(double a, size_t k) {
    if (!std::isfinite(a) || a < 0 || a > 1) panic("limit: strength " + std::to_string(k) + " must lie in [0, 1]");
}

} // namespace

extern "C" {

int rssync_limit_fit(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                     const double* frame_times, size_t n_frames, double delay, const double* targets,
                     const rssync_stabilize_params* params, const double* zooms, int32_t steps, double* strengths, uint32_t* status) {
    return guarded([&] {
        if (!frame_times) panic("limit: no frame times");
        if (!strengths) panic("limit: null output pointer");
        if (n_frames > 0xffffffffu) panic("limit: too many frames");
        // the camera at zoom 1, the zooms beside it, as the coverage sweep takes them
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, true);
        double zoom = 1.0;
        if (!zooms && params && params->zoom != 0) {
            check_zoom(params->zoom, "zoom");
            zoom = params->zoom;
        }
        if (steps < 0 || steps > rs::kLimitMaxSteps) panic("limit: steps must be 0 .. " + std::to_string(rs::kLimitMaxSteps));
        if (!n_frames) return;
        std::vector<double> z(n_frames, zoom);
        for (size_t k = 0; k < n_frames; ++k) {
            check_frame_time(cfg, frame_times[k], k);
            if (zooms) {
                check_zoom(zooms[k], "every zoom of the frames");
                z[k] = zooms[k];
            }
        }
        if (targets) (void)unit_targets(targets, n_frames); // (its checks; the goals go to the device as given)
        rship_ctx* c = device(p);
        if (rship_limit_fit(c, frame_times, (uint32_t)n_frames, targets, &cfg, z.data(), steps ? steps : rs::kLimitDefaultSteps, strengths,
                            status))
            panic(std::string("hip: limit: ") + rship_last_error(c));
    });
}

int rssync_limit_smooth(rssync_problem* p, const double* frame_times, const double* strengths, size_t n, double window, double* out) {
    return guarded([&] {
        if (!p) panic("limit: no problem");
        if (!std::isfinite(window) || window < 0) panic("limit: window must be finite and >= 0");
        if (!n) return;
        if (!frame_times) panic("limit: no frame times");
        if (!strengths) panic("limit: no strengths");
        if (!out) panic("limit: null output pointer");
        for (size_t k = 0; k < n; ++k) {
            if (!std::isfinite(frame_times[k])) panic("limit: non-finite frame time at " + std::to_string(k));
            if (k && frame_times[k] < frame_times[k - 1]) panic("limit: frame times must not decrease (at " + std::to_string(k) + ")");
            check_strength(strengths[k], k);
        }
        std::vector<double> e(n), res(n); // (out may be strengths)
        rs::limit_smooth(frame_times, strengths, n, window, e.data(), res.data());
        for (size_t k = 0; k < n; ++k) out[k] = res[k];
    });
}

int rssync_limit_targets(rssync_problem* p, const double* frame_times, size_t n_frames, double ro, double delay, const double* targets,
                         double sigma, const double* strengths, double* out_targets) {
    return guarded([&] {
        // rssync_stabilize_path's checks, in its order
        if (n_frames && !frame_times) panic("limit: no frame times");
        if (n_frames && !strengths) panic("limit: no strengths");
        if (n_frames && !out_targets) panic("limit: null output pointer");
        if (n_frames > 0x7fffffffu) panic("limit: too many frames");
        check_sigma(sigma);
        rship_stabilize_cfg cfg{};
        resolve_gyro(p, ro, delay, cfg);
        for (size_t k = 0; k < n_frames; ++k) {
            check_frame_time(cfg, frame_times[k], k);
            check_strength(strengths[k], k);
        }
        if (!n_frames) return;
        if (targets) (void)unit_targets(targets, n_frames);
        rship_ctx* c = device(p);
        std::vector<double> own(n_frames * 4), path;
        cfg.sigma = 0.0;
        if (rship_stabilize_path(c, frame_times, n_frames, &cfg, own.data())) panic(std::string("hip: limit: ") + rship_last_error(c));
        if (!targets) {
            path.resize(n_frames * 4);
            cfg.sigma = sigma;
            if (rship_stabilize_path(c, frame_times, n_frames, &cfg, path.data())) panic(std::string("hip: limit: ") + rship_last_error(c));
        }
        const double* goal = targets ? targets : path.data();
        std::vector<double> res(n_frames * 4); // (out_targets may be targets)
        for (size_t k = 0; k < n_frames; ++k) rs::limit_blend(own.data() + 4 * k, goal + 4 * k, strengths[k], res.data() + 4 * k);
        for (size_t k = 0; k < res.size(); ++k) out_targets[k] = res[k];
    });
}

} // extern "C"
