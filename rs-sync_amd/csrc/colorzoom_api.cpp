// colorzoom_api.cpp -- the public entry points of the dynamic zoom in colour (include/rssync_colorzoom.h): the colour
// front's checks and defaults (color_host.hpp) in color_api.cpp's order, then the zooms'.  The render runs in
// rship_colorzoom_frames (colorzoom_hip.h); the fit is two runs of rship_zoom_fit (zoom_hip.h), the luma's and the chroma
// plane's as a camera of its own, and a maximum on the host.
//
// A file of its own, linked into the product library only, like color_api.cpp.
#include "../../include/rssync_colorzoom.h"
#include "color_host.hpp"
#include "colorzoom_hip.h"
#include "host_errors.hpp"
#include "zoom_hip.h"
#include "zoom_math.hpp"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;
using namespace rssync_stab_host;
using namespace rssync_color_host;

namespace {

bool known_format(int format) { return (format >= RSSYNC_COLOR_GRAY8 && format <= RSSYNC_COLOR_RGBA32) || is_16(format); }

} // namespace

extern "C" {

int rssync_colorzoom_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                               const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                               const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                               uint64_t* n_outside, const double* zooms) {
    return guarded([&] {
        // the defining call's checks, in its order
        if (!frame_times) panic("color: no frame times");
        if (n_frames > 0xffffffffu) panic("color: too many frames");
        if (!known_format(format)) panic("color: format must be one of RSSYNC_COLOR_* or RSSYNC_COLOR16_*");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, is_16(format), true);
        const std::vector<Extent> a = check_image(in, format, width, height, n_frames, "frames"),
                                  b = check_image(out, format, out_width, out_height, n_frames, "out");
        if (!zooms) panic("colorzoom: no zooms");
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
        if (rship_colorzoom_frames(c, &di, (uint32_t)n_frames, frame_times, targets ? unit.data() : nullptr, &cfg, zooms, &dout, n_outside, 0))
            panic(std::string("hip: colorzoom: ") + rship_last_error(c));
    });
}

int rssync_colorzoom_fit(rssync_problem* p, int format, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                         size_t out_height, const double* frame_times, size_t n_frames, double delay, const double* targets,
                         const rssync_color_params* params, double zoom_lo, double zoom_hi, int32_t steps, double* zooms,
                         uint32_t* status) {
    return guarded([&] {
        // rssync_zoom_fit's checks, in its order, with the colour front's configuration
        if (!frame_times) panic("zoom: no frame times");
        if (!zooms) panic("zoom: null output pointer");
        if (n_frames > 0xffffffffu) panic("zoom: too many frames");
        if (!known_format(format)) panic("color: format must be one of RSSYNC_COLOR_* or RSSYNC_COLOR16_*");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, is_16(format), true);
        check_zoom(zoom_lo, "zoom_lo");
        check_zoom(zoom_hi, "zoom_hi");
        if (!(zoom_lo < zoom_hi)) panic("zoom: zoom_lo must be below zoom_hi");
        if (steps < 0 || steps > rs::kZoomMaxSteps) panic("zoom: steps must be 0 .. " + std::to_string(rs::kZoomMaxSteps));
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg.luma, frame_times[k], k); // (the luma's check alone, as in rssync_color.h)
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const int32_t n_steps = steps ? steps : rs::kZoomDefaultSteps;
        rship_ctx* c = device(p);
        // 1. plane 0
        if (rship_zoom_fit(c, frame_times, (uint32_t)n_frames, targets ? unit.data() : nullptr, &cfg.luma, zoom_lo, zoom_hi, n_steps, zooms, status))
            panic(std::string("hip: zoom: ") + rship_last_error(c));
        if (!is_yuv(format)) return;
        // 2. the chroma plane as a camera of its own, against the frames' targets: the caller's, or the path at the LUMA
        // frame times handed on as explicit targets (normalised as rssync_zoom_fit normalises a caller's)
        if (!targets) {
            std::vector<double> path(4 * n_frames);
            if (rship_stabilize_path(c, frame_times, n_frames, &cfg.luma, path.data())) panic(std::string("hip: stabilize: ") + rship_last_error(c));
            unit = unit_targets(path.data(), n_frames);
        }
        std::vector<double> times_c(n_frames), zooms_c(n_frames);
        std::vector<uint32_t> status_c(n_frames);
        for (size_t k = 0; k < n_frames; ++k) times_c[k] = frame_times[k] + cfg.chroma_time;
        if (rship_zoom_fit(c, times_c.data(), (uint32_t)n_frames, unit.data(), &cfg.chroma, zoom_lo, zoom_hi, n_steps, zooms_c.data(), status_c.data()))
            panic(std::string("hip: zoom: ") + rship_last_error(c));
        for (size_t k = 0; k < n_frames; ++k) {
            if (zooms_c[k] > zooms[k]) zooms[k] = zooms_c[k];
            if (status) status[k] |= status_c[k];
        }
    });
}

} // extern "C"
