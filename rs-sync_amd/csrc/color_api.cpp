// color_api.cpp -- the public colour entry points (include/rssync_color.h, and include/rssync_color16.h for samples in
// 16-bit containers, which differ in the sample alone): the stabiliser's checks and defaults
// (stabilize_host.hpp), the fills, the chroma plane's lens, frame time and output camera (color_math.hpp), the planes'
// pitches, strides and overlaps (color_host.hpp).  The work runs in rship_color_* (color_hip.h).
//
// A file of its own, linked into the product library only, like stabilize_api.cpp.
#include "../../include/rssync_color.h"
#include "../../include/rssync_color16.h"
#include "color_hip.h"
#include "color_host.hpp"
#include "color_math.hpp"
#include "stabilize_host.hpp"

#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;
using namespace rssync_stab_host;
using namespace rssync_color_host;

namespace {

// both stabilise entry points: they differ in the formats they take
int stabilize_any(bool wide, rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                  const double* frame_times, const rssync_lens* lens, double delay, const double* targets, const rssync_color_params* params,
                  const rssync_color_image* out, size_t out_width, size_t out_height, uint64_t* n_outside) {
    return guarded([&] {
        if (!frame_times) panic("color: no frame times");
        if (n_frames > 0xffffffffu) panic("color: too many frames");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params, wide);
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
        if (rship_color_frames(c, &di, (uint32_t)n_frames, frame_times, targets ? unit.data() : nullptr, &cfg, &dout, n_outside, 0))
            panic(std::string("hip: color: ") + rship_last_error(c));
    });
}

} // namespace

extern "C" {

int rssync_color_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                           const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                           const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                           uint64_t* n_outside) {
    return stabilize_any(false, p, format, in, n_frames, width, height, frame_times, lens, delay, targets, params, out, out_width, out_height,
                         n_outside);
}

int rssync_color16_stabilize(rssync_problem* p, int format, const rssync_color_image* in, size_t n_frames, size_t width, size_t height,
                             const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                             const rssync_color_params* params, const rssync_color_image* out, size_t out_width, size_t out_height,
                             uint64_t* n_outside) {
    return stabilize_any(true, p, format, in, n_frames, width, height, frame_times, lens, delay, targets, params, out, out_width, out_height,
                         n_outside);
}

int rssync_color_map(rssync_problem* p, int format, int plane, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                     size_t out_height, double frame_time, double delay, const double* target, const rssync_color_params* params,
                     float* map_xy) {
    return guarded([&] {
        if (!map_xy) panic("color: null output pointer");
        const rship_color_cfg cfg = resolve_color(p, format, width, height, lens, out_width, out_height, delay, params);
        if (plane != 0 && !(plane == 1 && is_yuv(format))) panic("color: plane " + std::to_string(plane) + " does not exist in this format");
        check_frame_time(cfg.luma, frame_time, 0);
        std::vector<double> unit;
        if (target) unit = unit_targets(target, 1);
        rship_ctx* c = device(p);
        if (rship_color_map(c, plane, frame_time, target ? unit.data() : nullptr, &cfg, map_xy))
            panic(std::string("hip: color: ") + rship_last_error(c));
    });
}

} // extern "C"
