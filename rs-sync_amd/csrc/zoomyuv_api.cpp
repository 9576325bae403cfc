// zoomyuv_api.cpp -- the public entry points of the dynamic zoom for the 4:2:2 and 4:4:4 formats
// (include/rssync_zoomyuv.h): yuv_api.cpp's checks and defaults (color_host.hpp) in its order, then the zooms'.  The render
// runs in rship_zoomyuv_frames (zoomyuv_hip.h); the fit is two runs of rship_zoom_fit (zoom_hip.h), the luma's and the
// 4:2:2 chroma plane's as a camera of its own at the luma's frame times, and a maximum on the host.
//
// A file of its own, linked into the product library only, like colorzoom_api.cpp.
#include "../../include/rssync_zoomyuv.h"
#include "color_host.hpp"
#include "host_errors.hpp"
#include "zoom_hip.h"
#include "zoom_math.hpp"
#include "zoomyuv_hip.h"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;
using namespace rssync_stab_host;
using namespace rssync_color_host;

extern "C" {

int rssync_zoomyuv_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                             const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                             const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                             uint64_t* n_outside, const double* zooms) {
    return guarded([&] {
        // rssync_yuv_stabilize's checks, in its order
        if (!frame_times) panic("color: no frame times");
        if (n_frames > 0xffffffffu) panic("color: too many frames");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, false, true, true);
        const std::vector<Extent> a = check_image(in, format, width, height, n_frames, "frames"),
                                  b = check_image(out, format, out_width, out_height, n_frames, "out");
        if (!zooms) panic("zoomyuv: no zooms");
        if (!n_frames) return;
        for (const Extent& x : a)
            for (const Extent& y : b)
                if (x.first < y.last && y.first < x.last) panic("color: an output plane overlaps an input plane");
        for (size_t k = 0; k < n_frames; ++k) {
            check_frame_time(cfg.luma, frame_times[k], k);
            check_zoom(zooms[k], "every zoom of the frames");
        }
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const rship_color_image di = image_of(in), dout = image_of(out);
        rship_ctx* c = device(p);
        if (rship_zoomyuv_frames(c, &di, (uint32_t)n_frames, frame_times, targets ? unit.data() : nullptr, &cfg, zooms, &dout, n_outside, 0))
            panic(std::string("hip: zoomyuv: ") + rship_last_error(c));
    });
}

int rssync_zoomyuv_fit(rssync_problem* p, int format, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                       size_t out_height, const double* frame_times, size_t n_frames, double delay, const double* targets,
                       const rssync_color_params* params, double zoom_lo, double zoom_hi, int32_t steps, double* zooms, uint32_t* status) {
    return guarded([&] {
        // rssync_zoom_fit's checks, in its order, with these formats' configuration
        if (!frame_times) panic("zoom: no frame times");
        if (!zooms) panic("zoom: null output pointer");
        if (n_frames > 0xffffffffu) panic("zoom: too many frames");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, false, true, true);
        check_zoom(zoom_lo, "zoom_lo");
        check_zoom(zoom_hi, "zoom_hi");
        if (!(zoom_lo < zoom_hi)) panic("zoom: zoom_lo must be below zoom_hi");
        if (steps < 0 || steps > rs::kZoomMaxSteps) panic("zoom: steps must be 0 .. " + std::to_string(rs::kZoomMaxSteps));
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg.luma, frame_times[k], k); // (the luma's check alone)
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const int32_t n_steps = steps ? steps : rs::kZoomDefaultSteps;
        rship_ctx* c = device(p);
        // 1. plane 0
        if (rship_zoom_fit(c, frame_times, (uint32_t)n_frames, targets ? unit.data() : nullptr, &cfg.luma, zoom_lo, zoom_hi, n_steps, zooms, status))
            panic(std::string("hip: zoom: ") + rship_last_error(c));
        if (!is_422(format)) return; // 4:4:4: every plane has the luma's camera
        // 2. the 4:2:2 chroma plane as a camera of its own at the frames' own times (cfg.chroma_time is 0), against the
        // frames' targets: the caller's, or the path handed on as explicit targets (normalised as rssync_zoom_fit
        // normalises a caller's)
        if (!targets) {
            std::vector<double> path(4 * n_frames);
            if (rship_stabilize_path(c, frame_times, n_frames, &cfg.luma, path.data())) panic(std::string("hip: stabilize: ") + rship_last_error(c));
            unit = unit_targets(path.data(), n_frames);
        }
        std::vector<double> zooms_c(n_frames);
        std::vector<uint32_t> status_c(n_frames);
        if (rship_zoom_fit(c, frame_times, (uint32_t)n_frames, unit.data(), &cfg.chroma, zoom_lo, zoom_hi, n_steps, zooms_c.data(), status_c.data()))
            panic(std::string("hip: zoom: ") + rship_last_error(c));
        for (size_t k = 0; k < n_frames; ++k) {
            if (zooms_c[k] > zooms[k]) zooms[k] = zooms_c[k];
            if (status) status[k] |= status_c[k];
        }
    });
}

} // extern "C"
