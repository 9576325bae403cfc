// color_host.hpp -- what the colour front's public entry points do before the device runs: the formats' planes, the fills,
// the chroma plane's lens, frame time and output camera (color_math.hpp), the planes' pitches, strides and extents.  Shared
// by color_api.cpp, colorzoom_api.cpp (include/rssync_colorzoom.h resolves a call exactly as the colour front does) and
// yuv_api.cpp and zoomyuv_api.cpp (include/rssync_yuv.h and include/rssync_zoomyuv.h: the 4:2:2 and 4:4:4 formats, which only
// their entry points take).
#pragma once

#include "../../include/rssync_color.h"
#include "../../include/rssync_color16.h"
#include "../../include/rssync_yuv.h"
#include "color_hip.h"
#include "color_math.hpp"
#include "stabilize_host.hpp"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// the stabiliser's struct leads the colour parameters: its new last field must not have moved what follows
static_assert(offsetof(rssync_color_params, chroma_site) == 64 && sizeof(rssync_color_params) == 88, "rssync_color_params moved");

namespace rssync_color_host {

using rssync_host::panic;
using namespace rssync_stab_host;

inline bool is_16(int format) { return format >= RSSYNC_COLOR16_GRAY16 && format <= RSSYNC_COLOR16_I010; }

// include/rssync_yuv.h's formats, and those of them in 16-bit containers
inline bool is_yuv4(int format) {
    return (format >= RSSYNC_YUV_I422 && format <= RSSYNC_YUV_I444) || (format >= RSSYNC_YUV_I210 && format <= RSSYNC_YUV_I410);
}
inline bool is_wide(int format) { return is_16(format) || (format >= RSSYNC_YUV_I210 && format <= RSSYNC_YUV_I410); }

// the 8-bit format whose planes and geometry a 16-bit format has
inline int sibling(int format) {
    switch (format) {
    case RSSYNC_COLOR16_GRAY16: return RSSYNC_COLOR_GRAY8;
    case RSSYNC_COLOR16_P010:
    case RSSYNC_COLOR16_P016: return RSSYNC_COLOR_NV12;
    case RSSYNC_COLOR16_I010: return RSSYNC_COLOR_I420;
    case RSSYNC_YUV_I210: return RSSYNC_YUV_I422;
    case RSSYNC_YUV_P210:
    case RSSYNC_YUV_P216: return RSSYNC_YUV_NV16;
    case RSSYNC_YUV_I410: return RSSYNC_YUV_I444;
    default: return format;
    }
}

// bits of a sample value
inline int depth(int format) {
    if (!is_wide(format)) return 8;
    return (format == RSSYNC_COLOR16_GRAY16 || format == RSSYNC_COLOR16_P016 || format == RSSYNC_YUV_P216) ? 16 : 10;
}

inline bool is_yuv(int format) { return sibling(format) == RSSYNC_COLOR_NV12 || sibling(format) == RSSYNC_COLOR_I420; }
inline bool is_422(int format) { return sibling(format) == RSSYNC_YUV_I422 || sibling(format) == RSSYNC_YUV_NV16; }
inline bool is_444(int format) { return sibling(format) == RSSYNC_YUV_I444; }

struct Plane {
    size_t row_bytes, rows;
};

// the planes of a width x height frame -> their number; a 16-bit format's rows are twice its sibling's bytes
inline int planes_of(int format, size_t w, size_t h, Plane* pl) {
    const size_t b = is_wide(format) ? 2 : 1;
    switch (sibling(format)) {
    case RSSYNC_COLOR_GRAY8: pl[0] = {b * w, h}; return 1;
    case RSSYNC_COLOR_NV12: pl[0] = {b * w, h}; pl[1] = {b * w, h / 2}; return 2;
    case RSSYNC_COLOR_I420: pl[0] = {b * w, h}; pl[1] = pl[2] = {b * (w / 2), h / 2}; return 3;
    case RSSYNC_YUV_I422: pl[0] = {b * w, h}; pl[1] = pl[2] = {b * (w / 2), h}; return 3;
    case RSSYNC_YUV_NV16: pl[0] = pl[1] = {b * w, h}; return 2;
    case RSSYNC_YUV_I444: pl[0] = pl[1] = pl[2] = {b * w, h}; return 3;
    default: pl[0] = {4 * w, h}; return 1;
    }
}

// format, sizes, parameters -> the configuration of both cameras.  wide: the call came through rssync_color16.h, whose
// formats are the only ones it takes (and which the 8-bit entry points do not take); zoom_one: params->stab.zoom is not
// read (the zooms come beside the call: colorzoom_api.cpp); yuv4: the call came through rssync_yuv.h, whose formats are
// the only ones it takes, whatever `wide` says
inline rship_color_cfg resolve_color(rssync_problem* p, int format, size_t width, size_t height, const rssync_lens* lens, size_t out_width,
                              size_t out_height, double delay, const rssync_color_params* params, bool wide = false,
                              bool zoom_one = false, bool yuv4 = false) {
    if (yuv4) {
        if (!is_yuv4(format)) panic("color: format must be one of RSSYNC_YUV_*");
        wide = is_wide(format);
    } else {
        if (wide && !is_16(format)) panic("color: format must be one of RSSYNC_COLOR16_*");
        if (!wide && (format < RSSYNC_COLOR_GRAY8 || format > RSSYNC_COLOR_RGBA32)) panic("color: format must be one of RSSYNC_COLOR_*");
    }
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
    if (is_422(format)) {
        if ((width | out_width) & 1)
            panic("color: 4:2:2 frames need an even width (" + std::to_string(width) + " -> " + std::to_string(out_width) + ")");
        if (width < 4 || out_width < 4) panic("color: a 4:2:2 frame is too small (4 pixels wide at least)");
    }
    c.luma = resolve(p, width, height, lens, out_width, out_height, delay, &q.stab, zoom_one);
    if (!q.fill_set) {
        const int f = c.luma.fill;
        const int by_format[4][4] = {{f, 0, 0, 0}, {f, 128, 128, 0}, {f, 128, 128, 0}, {f, f, f, 255}};
        for (int k = 0; k < 4; ++k) c.fill[k] = by_format[is_422(format) || is_444(format) ? 1 : sibling(format)][k] << (bits - 8);
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
    if (is_422(format)) {
        double ox;
        rs::color_chroma422_offset(q.chroma_site, &ox);
        c.chroma.width = c.luma.width / 2;
        c.chroma.out_width = c.luma.out_width / 2;
        rs::color_chroma422_camera(&c.luma.lens[1], ox, &c.chroma.lens[1]);
        rs::color_chroma422_camera(c.luma.cam, ox, c.chroma.cam);
        c.chroma_time = rs::color_chroma422_time(0.0);
    }
    return c;
}

struct Extent {
    uintptr_t first, last; // first byte, one past the last
};

// pitches, strides and NULL planes of an image -> the bytes each plane spans
inline std::vector<Extent> check_image(const rssync_color_image* img, int format, size_t w, size_t h, size_t n_frames, const char* what) {
    if (!img) panic(std::string("color: no ") + what);
    Plane pl[3];
    const int np = planes_of(format, w, h, pl);
    std::vector<Extent> ext;
    for (int k = 0; k < np; ++k) {
        const std::string name = std::string(what) + " plane " + std::to_string(k);
        if (!img->plane[k]) panic("color: " + name + " is NULL");
        if (is_wide(format) && (((uintptr_t)img->plane[k] | img->pitch[k]) & 1 || (n_frames > 1 && (img->stride[k] & 1))))
            panic("color: alignment: pointer, pitch and frame stride of " + name + " must be multiples of 2");
        if (img->pitch[k] < pl[k].row_bytes)
            panic("color: pitch " + std::to_string(img->pitch[k]) + " of " + name + " < its row of " + std::to_string(pl[k].row_bytes) + " bytes");
        if (n_frames > 1 && img->stride[k] < img->pitch[k] * pl[k].rows) panic("color: frame stride of " + name + " smaller than pitch * rows");
        const uintptr_t a = (uintptr_t)img->plane[k];
        ext.push_back({a, a + (n_frames ? (n_frames - 1) * img->stride[k] + (pl[k].rows - 1) * img->pitch[k] + pl[k].row_bytes : 0)});
    }
    return ext;
}

inline rship_color_image image_of(const rssync_color_image* img) {
    rship_color_image r{};
    for (int k = 0; k < 3; ++k) {
        r.plane[k] = img->plane[k];
        r.pitch[k] = img->pitch[k];
        r.stride[k] = img->stride[k];
    }
    return r;
}

} // namespace rssync_color_host
