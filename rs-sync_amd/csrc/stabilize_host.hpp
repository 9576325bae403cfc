// stabilize_host.hpp -- what the stabiliser's public entry points do before the device runs: the checks, the defaults,
// the output camera, the caller's targets normalised, the check of a frame's row times against the gyro's knots.  Shared by
// stabilize_api.cpp and color_api.cpp (include/rssync_color.h resolves a call exactly as the stabiliser does).
#pragma once

#include "../../include/rssync_c.h"
#include "../../include/rssync_stabilize.h"
#include "host_errors.hpp"
#include "limit_math.hpp"
#include "stabilize_hip.h"

#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

// `filter` took the place of tail padding: callers built against the nine-field struct keep working and pass 0 there
// only if they zero-filled it, as the header's "all zeros = all defaults" demands
static_assert(sizeof(rssync_stabilize_params) == 64 && offsetof(rssync_stabilize_params, filter) == 60, "rssync_stabilize_params moved");
static_assert(sizeof(rship_stabilize_cfg) == 176 && offsetof(rship_stabilize_cfg, filter) == 172, "rship_stabilize_cfg moved");

namespace rssync_stab_host {

using rssync_host::panic;

// the gyro table's part of a configuration, ro and delay
inline void resolve_gyro(rssync_problem* p, double ro, double delay, rship_stabilize_cfg& c) {
    if (!p) panic("stabilize: no problem");
    if (!std::isfinite(ro)) panic("stabilize: non-finite readout time");
    if (ro < 0) panic("stabilize: negative readout time");
    if (!std::isfinite(delay)) panic("stabilize: non-finite delay");
    c.lens[0] = ro;
    c.delay = delay;
    size_t n_knots = 0;
    rssync_ext_sample_rate(p, &c.fs, &c.start, &n_knots);
    if (n_knots < 2) panic("stabilize: no gyro data was set");
    rssync_host::ensure_gyro_table(p);
    c.n_knots = (uint32_t)n_knots;
}

inline void check_sigma(double sigma) {
    if (!std::isfinite(sigma) || sigma < 0) panic("stabilize: sigma must be finite and >= 0");
}

inline void check_zoom(double zoom, const char* what) {
    if (!std::isfinite(zoom) || zoom <= 0) panic(std::string("stabilize: ") + what + " must be finite and > 0");
}

// everything but the frames and the targets.  zoom_one: the coverage sweep brings its own zooms, params->zoom is not read
inline rship_stabilize_cfg resolve(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                            double delay, const rssync_stabilize_params* params, bool zoom_one) {
    if (!p) panic("stabilize: no problem");
    if (!lens) panic("stabilize: no lens");
    if (width < 2 || height < 2) panic("stabilize: a " + std::to_string(width) + " x " + std::to_string(height) + " frame is too small (2 x 2 at least)");
    if (out_width < 2 || out_height < 2)
        panic("stabilize: a " + std::to_string(out_width) + " x " + std::to_string(out_height) + " output is too small (2 x 2 at least)");
    if (width > 65536 || height > 65536 || out_width > 65536 || out_height > 65536)
        panic("stabilize: frames of more than 65536 pixels a side are not supported");
    const double L[9] = {lens->ro, lens->fx, lens->fy, lens->cx, lens->cy, lens->k1, lens->k2, lens->k3, lens->k4};
    for (double v : L)
        if (!std::isfinite(v)) panic("stabilize: non-finite lens parameter");
    if (lens->fx == 0 || lens->fy == 0) panic("stabilize: zero focal length");
    const rssync_stabilize_params q = params ? *params : rssync_stabilize_params{};
    rship_stabilize_cfg c{};
    resolve_gyro(p, lens->ro, delay, c);
    c.width = (uint32_t)width;
    c.height = (uint32_t)height;
    c.out_width = (uint32_t)out_width;
    c.out_height = (uint32_t)out_height;
    for (int i = 0; i < 9; ++i) c.lens[i] = L[i];
    check_sigma(q.sigma);
    c.sigma = q.sigma;
    double zoom = 1.0;
    if (!zoom_one && q.zoom != 0) {
        check_zoom(q.zoom, "zoom");
        zoom = q.zoom;
    }
    const double cam[4] = {q.fx, q.fy, q.cx, q.cy};
    const int given = (q.fx != 0) + (q.fy != 0) + (q.cx != 0) + (q.cy != 0);
    if (given == 0) {
        // the lens's camera scaled to the output: the factors are exactly 1 when the sizes agree
        const double sx = (double)out_width / (double)width, sy = (double)out_height / (double)height;
        c.cam[0] = lens->fx * sx;
        c.cam[1] = lens->fy * sy;
        c.cam[2] = lens->cx * sx;
        c.cam[3] = lens->cy * sy;
    } else {
        if (given != 4) panic("stabilize: fx, fy, cx, cy must be given together (or all left 0)");
        for (int i = 0; i < 4; ++i) {
            if (!std::isfinite(cam[i])) panic("stabilize: non-finite output camera");
            c.cam[i] = cam[i];
        }
    }
    c.cam[0] = c.cam[0] * zoom;
    c.cam[1] = c.cam[1] * zoom;
    if (q.camera != RSSYNC_CAMERA_LENS && q.camera != RSSYNC_CAMERA_PINHOLE) panic("stabilize: camera must be RSSYNC_CAMERA_LENS or RSSYNC_CAMERA_PINHOLE");
    c.camera = q.camera;
    if (q.filter != RSSYNC_FILTER_BILINEAR && q.filter != RSSYNC_FILTER_BICUBIC)
        panic("stabilize: filter must be RSSYNC_FILTER_BILINEAR or RSSYNC_FILTER_BICUBIC");
    c.filter = q.filter;
    c.iterations = q.iterations ? q.iterations : 3;
    if (c.iterations < 1 || c.iterations > 8) panic("stabilize: iterations must be 1 .. 8");
    if (q.fill < 0 || q.fill > 255) panic("stabilize: fill must be 0 .. 255");
    c.fill = q.fill;
    return c;
}

// a frame's rows 0 .. rows must lie inside the knots: nothing is extrapolated (the path's taps alone are clamped)
inline void check_frame_time(const rship_stabilize_cfg& c, double t, size_t k) {
    if (!std::isfinite(t)) panic("stabilize: non-finite frame time at " + std::to_string(k));
    const double x0 = (t + c.delay - c.start) * c.fs, x1 = (t + c.lens[0] + c.delay - c.start) * c.fs;
    if (!(x0 >= 0 && x1 <= (double)(c.n_knots - 1)))
        panic("stabilize: frame " + std::to_string(k) + " at " + std::to_string(t) + " s + delay " + std::to_string(c.delay) +
              " s leaves the gyro data (" + std::to_string(c.start) + " .. " + std::to_string(c.start + (c.n_knots - 1) / c.fs) + " s)");
}

// the caller's targets as unit quaternions, fp64
inline std::vector<double> unit_targets(const double* targets, size_t n) {
    std::vector<double> u(n * 4);
    for (size_t k = 0; k < n; ++k) {
        // (rs::limit_unit: the one normalisation, which the path limiter's kernel applies to its candidates as well)
        const double norm = rs::limit_unit(targets + 4 * k, u.data() + 4 * k);
        if (!std::isfinite(norm) || !(norm > 0)) panic("stabilize: target " + std::to_string(k) + " is zero or not finite");
    }
    return u;
}

inline rship_ctx* device(rssync_problem* p) {
    rship_ctx* c = (rship_ctx*)rssync_ext_device_context(p);
    if (!c) panic("stabilize: no device");
    return c;
}


} // namespace rssync_stab_host
