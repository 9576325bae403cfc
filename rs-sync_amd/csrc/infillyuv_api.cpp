// infillyuv_api.cpp -- the public entry point of the infill for 4:2:2 and 4:4:4 video (include/rssync_infillyuv.h):
// yuv_api.cpp's checks and defaults (color_host.hpp) in its order, then the radius.  params->stab.zoom is read: one zoom for
// the call.  The device work runs in rship_infillyuv_frames (infillyuv_hip.h).
//
// A file of its own, linked into the product library only, like yuv_api.cpp.
#include "../../include/rssync_infillyuv.h"
#include "color_host.hpp"
#include "color_math.hpp"
#include "host_errors.hpp"
#include "infill_math.hpp"
#include "infillyuv_hip.h"
#include "stabilize_host.hpp"

#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;
using namespace rssync_stab_host;
using namespace rssync_color_host;

static_assert(RSSYNC_INFILL_MAX_RADIUS == rs::kInfillMaxRadius, "the largest radius moved");

static void check_radius(int32_t radius) {
    if (radius < 0 || radius > rs::kInfillMaxRadius)
        panic("infillyuv: radius " + std::to_string(radius) + " must be 0 .. " + std::to_string(rs::kInfillMaxRadius));
}

extern "C" {

int rssync_infillyuv_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                               const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                               const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                               uint64_t* n_outside, int32_t radius, uint64_t* n_borrowed) {
    return guarded([&] {
        // the defining call's checks, in its order
        if (!frame_times) panic("color: no frame times");
        if (n_frames > 0xffffffffu) panic("color: too many frames");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, false, false, true);
        const std::vector<Extent> a = check_image(in, format, width, height, n_frames, "frames"),
                                  b = check_image(out, format, out_width, out_height, n_frames, "out");
        check_radius(radius);
        if (!n_frames) return;
        for (const Extent& x : a)
            for (const Extent& y : b)
                if (x.first < y.last && y.first < x.last) panic("color: an output plane overlaps an input plane");
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg.luma, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const rship_color_image di = image_of(in), dout = image_of(out);
        rship_ctx* c = device(p);
        if (rship_infillyuv_frames(c, &di, (uint32_t)n_frames, frame_times, targets ? unit.data() : nullptr, &cfg, &dout, n_outside, radius,
                                   n_borrowed, 0))
            panic(std::string("hip: infillyuv: ") + rship_last_error(c));
    });
}

} // extern "C"
