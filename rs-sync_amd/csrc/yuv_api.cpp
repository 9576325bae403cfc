// yuv_api.cpp -- the public entry points of the 4:2:2 and 4:4:4 formats (include/rssync_yuv.h): the colour front's checks
// and defaults (color_host.hpp, stabilize_host.hpp) with these formats' planes and the 4:2:2 chroma plane's lens and output
// camera (color_math.hpp).  The work runs in rship_yuv_* (yuv_hip.h).
//
// A file of its own, linked into the product library only, like color_api.cpp.
#include "../../include/rssync_yuv.h"
#include "color_host.hpp"
#include "color_math.hpp"
#include "stabilize_host.hpp"
#include "yuv_hip.h"

#include <cstddef>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;
using namespace rssync_stab_host;
using namespace rssync_color_host;

extern "C" {

int rssync_yuv_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                         const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                         const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                         uint64_t* n_outside) {
    return guarded([&] {
        if (!frame_times) panic("color: no frame times");
        if (n_frames > 0xffffffffu) panic("color: too many frames");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, false, false, true);
        const std::vector<Extent> a = check_image(in, format, width, height, n_frames, "frames"),
                                  b = check_image(out, format, out_width, out_height, n_frames, "out");
        if (!n_frames) return;
        for (const Extent& x : a)
            for (const Extent& y : b)
                if (x.first < y.last && y.first < x.last) panic("color: an output plane overlaps an input plane");
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg.luma, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        const rship_color_image di = image_of(in), dout = image_of(out);
        rship_ctx* c = device(p);
        if (rship_yuv_frames(c, &di, (uint32_t)n_frames, frame_times, targets ? unit.data() : nullptr, &cfg, &dout, n_outside, 0))
            panic(std::string("hip: yuv: ") + rship_last_error(c));
    });
}

int rssync_yuv_map(rssync_problem* p, int format, int plane, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                   size_t out_height, double frame_time, double delay, const double* target, const rssync_color_params* params,
                   float* map_xy) {
    return guarded([&] {
        if (!map_xy) panic("color: null output pointer");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, false, false, true);
        if (plane != 0 && plane != 1) panic("color: plane " + std::to_string(plane) + " does not exist in this format");
        check_frame_time(cfg.luma, frame_time, 0);
        std::vector<double> unit;
        if (target) unit = unit_targets(target, 1);
        rship_ctx* c = device(p);
        if (rship_yuv_map(c, plane, frame_time, target ? unit.data() : nullptr, &cfg, map_xy))
            panic(std::string("hip: yuv: ") + rship_last_error(c));
    });
}

} // extern "C"
