// color_api.cpp -- the public colour entry points (include/rssync_color.h, and include/rssync_color16.h for samples in
// 16-bit containers, which differ in the sample alone): the stabiliser's checks and defaults
// (stabilize_host.hpp), the fills, the chroma plane's lens, frame time and output camera (color_math.hpp), the planes'
// pitches, strides and overlaps.  The work runs in rship_color_* (color_hip.h).
//
// A file of its own, linked into the product library only, like stabilize_api.cpp.
#include "../../include/rssync_color.h"
#include "../../include/rssync_color16.h"
#include "color_hip.h"
#include "color_math.hpp"
#include "stabilize_host.hpp"

#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

// the stabiliser's struct leads the colour parameters: its new last field must not have moved what follows
static_assert(offsetof(rssync_color_params, chroma_site) == 64 && sizeof(rssync_color_params) == 88, "rssync_color_params moved");

using rssync_host::guarded;
using rssync_host::panic;
using namespace rssync_stab_host;

namespace {

bool is_16(int format) { return format >= RSSYNC_COLOR16_GRAY16 && format <= RSSYNC_COLOR16_I010; }

// the 8-bit format whose planes and geometry a 16-bit format has
int sibling(int format) {
    switch (format) {
    case RSSYNC_COLOR16_GRAY16: return RSSYNC_COLOR_GRAY8;
    case RSSYNC_COLOR16_P010:
    case RSSYNC_COLOR16_P016: return RSSYNC_COLOR_NV12;
    case RSSYNC_COLOR16_I010: return RSSYNC_COLOR_I420;
    default: return format;
    }
}

// bits of a sample value
int depth(int format) { return !is_16(format) ? 8 : (format == RSSYNC_COLOR16_P010 || format == RSSYNC_COLOR16_I010) ? 10 : 16; }

bool is_yuv(int format) { return sibling(format) == RSSYNC_COLOR_NV12 || sibling(format) == RSSYNC_COLOR_I420; }

struct Plane {
    size_t row_bytes, rows;
};

// the planes of a width x height frame -> their number; a 16-bit format's rows are twice its sibling's bytes
int planes_of(int format, size_t w, size_t h, Plane* pl) {
    const size_t b = is_16(format) ? 2 : 1;
    switch (sibling(format)) {
    case RSSYNC_COLOR_GRAY8: pl[0] = {b * w, h}; return 1;
    case RSSYNC_COLOR_NV12: pl[0] = {b * w, h}; pl[1] = {b * w, h / 2}; return 2;
    case RSSYNC_COLOR_I420: pl[0] = {b * w, h}; pl[1] = pl[2] = {b * (w / 2), h / 2}; return 3;
    default: pl[0] = {4 * w, h}; return 1;
    }
}

// format, sizes, parameters -> the configuration of both cameras.  wide: the call came through rssync_color16.h, whose
// formats are the only ones it takes (and which the 8-bit entry points do not take)
rship_color_cfg resolve_color(rssync_problem* p, int format, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                              size_t out_height, double delay, const rssync_color_params* params, bool wide = false) {
    if (wide && !is_16(format)) panic("color: format must be one of RSSYNC_COLOR16_*");
    if (!wide && (format < RSSYNC_COLOR_GRAY8 || format > RSSYNC_COLOR_RGBA32)) panic("color: format must be one of RSSYNC_COLOR_*");
    const int bits = depth(format), top = (1 << bits) - 1;
    rssync_color_params q = params ? *params : rssync_color_params{};
    if (q.chroma_site != RSSYNC_CHROMA_CENTER && q.chroma_site != RSSYNC_CHROMA_LEFT)
        panic("color: chroma_site must be RSSYNC_CHROMA_CENTER or RSSYNC_CHROMA_LEFT");
    rship_color_cfg c{};
    c.format = format;
    if (q.fill_set) {
        for (int k = 0; k < 4; ++k) {
            if (q.fill[k] < 0 || q.fill[k] > top) panic("color: fill " + std::to_string(k) + " must be 0 .. " + std::to_string(top));
            c.fill[k] = q.fill[k];
        }
        q.stab.fill = 0; // (not read)
    }
    if (is_yuv(format)) {
        if ((width | height | out_width | out_height) & 1)
            panic("color: 4:2:0 frames need an even width and height (" + std::to_string(width) + " x " + std::to_string(height) + " -> " +
                  std::to_string(out_width) + " x " + std::to_string(out_height) + ")");
        if (width < 4 || height < 4 || out_width < 4 || out_height < 4) panic("color: a 4:2:0 frame is too small (4 x 4 at least)");
    }
    c.luma = resolve(p, width, height, lens, out_width, out_height, delay, &q.stab, false);
    if (!q.fill_set) {
        const int f = c.luma.fill;
        const int by_format[4][4] = {{f, 0, 0, 0}, {f, 128, 128, 0}, {f, 128, 128, 0}, {f, f, f, 255}};
        for (int k = 0; k < 4; ++k) c.fill[k] = by_format[sibling(format)][k] << (bits - 8);
    }
    c.luma.fill = wide ? 0 : c.fill[0]; // (a 16-bit fill goes to the kernels from fill[] alone)
    c.chroma = c.luma;
    if (is_yuv(format)) {
        double ox, oy;
        rs::color_chroma_offset(q.chroma_site, &ox, &oy);
        c.chroma.width = c.luma.width / 2;
        c.chroma.height = c.luma.height / 2;
        c.chroma.out_width = c.luma.out_width / 2;
        c.chroma.out_height = c.luma.out_height / 2;
        rs::color_chroma_camera(&c.luma.lens[1], ox, oy, &c.chroma.lens[1]);
        rs::color_chroma_camera(c.luma.cam, ox, oy, c.chroma.cam);
        c.chroma_time = rs::color_chroma_time(0.0, c.luma.lens[0], oy, (double)height); // (0 + x is x: the launcher adds it to T)
    }
    return c;
}

struct Extent {
    uintptr_t first, last; // first byte, one past the last
};

// pitches, strides and NULL planes of an image -> the bytes each plane spans
std::vector<Extent> check_image(const rssync_color_image* img, int format, size_t w, size_t h, size_t n_frames, const char* what) {
    if (!img) panic(std::string("color: no ") + what);
    Plane pl[3];
    const int np = planes_of(format, w, h, pl);
    std::vector<Extent> ext;
    for (int k = 0; k < np; ++k) {
        const std::string name = std::string(what) + " plane " + std::to_string(k);
        if (!img->plane[k]) panic("color: " + name + " is NULL");
        if (is_16(format) && (((uintptr_t)img->plane[k] | img->pitch[k]) & 1 || (n_frames > 1 && (img->stride[k] & 1))))
            panic("color: alignment: pointer, pitch and frame stride of " + name + " must be multiples of 2");
        if (img->pitch[k] < pl[k].row_bytes)
            panic("color: pitch " + std::to_string(img->pitch[k]) + " of " + name + " < its row of " + std::to_string(pl[k].row_bytes) + " bytes");
        if (n_frames > 1 && img->stride[k] < img->pitch[k] * pl[k].rows) panic("color: frame stride of " + name + " smaller than pitch * rows");
        const uintptr_t a = (uintptr_t)img->plane[k];
        ext.push_back({a, a + (n_frames ? (n_frames - 1) * img->stride[k] + (pl[k].rows - 1) * img->pitch[k] + pl[k].row_bytes : 0)});
    }
    return ext;
}

rship_color_image image_of(const rssync_color_image* img) {
    rship_color_image r{};
    for (int k = 0; k < 3; ++k) {
        r.plane[k] = img->plane[k];
        r.pitch[k] = img->pitch[k];
        r.stride[k] = img->stride[k];
    }
    return r;
}

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
