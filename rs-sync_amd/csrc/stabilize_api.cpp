// stabilize_api.cpp -- the public stabiliser entry points (include/rssync_stabilize.h): argument checks, defaults, the
// output camera, the caller's targets normalised, the check of a frame's row times against the gyro's knots.  The work
// runs in rship_stabilize_* (stabilize_hip.h).
//
// A file of its own, linked into the product library only, like rectify_api.cpp.
#include "../../include/rssync_c.h"
#include "../../include/rssync_stabilize.h"
#include "host_errors.hpp"
#include "stabilize_hip.h"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;

namespace {

// the gyro table's part of a configuration, ro and delay
void resolve_gyro(rssync_problem* p, double ro, double delay, rship_stabilize_cfg& c) {
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

void check_sigma(double sigma) {
    if (!std::isfinite(sigma) || sigma < 0) panic("stabilize: sigma must be finite and >= 0");
}

void check_zoom(double zoom, const char* what) {
    if (!std::isfinite(zoom) || zoom <= 0) panic(std::string("stabilize: ") + what + " must be finite and > 0");
}

// everything but the frames and the targets.  zoom_one: the coverage sweep brings its own zooms, params->zoom is not read
rship_stabilize_cfg resolve(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
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
    c.iterations = q.iterations ? q.iterations : 3;
    if (c.iterations < 1 || c.iterations > 8) panic("stabilize: iterations must be 1 .. 8");
    if (q.fill < 0 || q.fill > 255) panic("stabilize: fill must be 0 .. 255");
    c.fill = q.fill;
    return c;
}

// a frame's rows 0 .. rows must lie inside the knots: nothing is extrapolated (the path's taps alone are clamped)
void check_frame_time(const rship_stabilize_cfg& c, double t, size_t k) {
    if (!std::isfinite(t)) panic("stabilize: non-finite frame time at " + std::to_string(k));
    const double x0 = (t + c.delay - c.start) * c.fs, x1 = (t + c.lens[0] + c.delay - c.start) * c.fs;
    if (!(x0 >= 0 && x1 <= (double)(c.n_knots - 1)))
        panic("stabilize: frame " + std::to_string(k) + " at " + std::to_string(t) + " s + delay " + std::to_string(c.delay) +
              " s leaves the gyro data (" + std::to_string(c.start) + " .. " + std::to_string(c.start + (c.n_knots - 1) / c.fs) + " s)");
}

// the caller's targets as unit quaternions, fp64
std::vector<double> unit_targets(const double* targets, size_t n) {
    std::vector<double> u(n * 4);
    for (size_t k = 0; k < n; ++k) {
        const double* q = targets + 4 * k;
        const double norm = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        if (!std::isfinite(norm) || !(norm > 0)) panic("stabilize: target " + std::to_string(k) + " is zero or not finite");
        for (int i = 0; i < 4; ++i) u[4 * k + i] = q[i] / norm;
    }
    return u;
}

rship_ctx* device(rssync_problem* p) {
    rship_ctx* c = (rship_ctx*)rssync_ext_device_context(p);
    if (!c) panic("stabilize: no device");
    return c;
}

} // namespace

extern "C" {

int rssync_stabilize_path(rssync_problem* p, const double* frame_times, size_t n, double ro, double delay, double sigma, double* quats) {
    return guarded([&] {
        if (n && !frame_times) panic("stabilize: no frame times");
        if (n && !quats) panic("stabilize: null output pointer");
        if (n > 0x7fffffffu) panic("stabilize: too many frames");
        check_sigma(sigma);
        rship_stabilize_cfg cfg{};
        resolve_gyro(p, ro, delay, cfg);
        cfg.sigma = sigma;
        for (size_t k = 0; k < n; ++k) check_frame_time(cfg, frame_times[k], k);
        rship_ctx* c = device(p);
        if (rship_stabilize_path(c, frame_times, n, &cfg, quats)) panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

int rssync_stabilize_map(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                         double frame_time, double delay, const double* target, const rssync_stabilize_params* params, float* map_xy) {
    return guarded([&] {
        if (!map_xy) panic("stabilize: null output pointer");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, false);
        check_frame_time(cfg, frame_time, 0);
        std::vector<double> unit;
        if (target) unit = unit_targets(target, 1);
        rship_ctx* c = device(p);
        if (rship_stabilize_map(c, frame_time, target ? unit.data() : nullptr, &cfg, map_xy)) panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

int rssync_stabilize_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                            size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay, const double* targets,
                            const rssync_stabilize_params* params, uint8_t* out, size_t out_width, size_t out_height, size_t out_pitch,
                            size_t out_stride, uint64_t* n_outside) {
    return guarded([&] {
        if (!frames) panic("stabilize: no frames");
        if (!out) panic("stabilize: null output pointer");
        if (!frame_times) panic("stabilize: no frame times");
        if (n_frames > 0xffffffffu) panic("stabilize: too many frames");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, false);
        if (pitch < width) panic("stabilize: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
        if (out_pitch < out_width) panic("stabilize: out_pitch " + std::to_string(out_pitch) + " < out_width " + std::to_string(out_width));
        if (n_frames > 1 && (frame_stride < pitch * height || out_stride < out_pitch * out_height))
            panic("stabilize: frame stride smaller than pitch * height");
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        // the two extents, first to last byte
        const uintptr_t a0 = (uintptr_t)frames, a1 = a0 + (n_frames - 1) * frame_stride + (height - 1) * pitch + width;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (n_frames - 1) * out_stride + (out_height - 1) * out_pitch + out_width;
        if (a0 < b1 && b0 < a1) panic("stabilize: out overlaps the frames");
        rship_ctx* c = device(p);
        if (rship_stabilize_frames(c, frames, (uint32_t)n_frames, pitch, frame_stride, frame_times, targets ? unit.data() : nullptr, &cfg, out,
                                   out_pitch, out_stride, n_outside, 0))
            panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

int rssync_stabilize_coverage(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, size_t out_width, size_t out_height,
                              const double* frame_times, size_t n_frames, double delay, const double* targets,
                              const rssync_stabilize_params* params, const double* zooms, size_t n_zooms, uint32_t* outside) {
    return guarded([&] {
        if (!frame_times) panic("stabilize: no frame times");
        if (!zooms) panic("stabilize: no zooms");
        if (!outside) panic("stabilize: null output pointer");
        if (n_frames > 0xffffffffu) panic("stabilize: too many frames");
        if (n_zooms > 65535) panic("stabilize: more than 65535 zooms in one sweep");
        const rship_stabilize_cfg cfg = resolve(p, width, height, lens, out_width, out_height, delay, params, true);
        for (size_t z = 0; z < n_zooms; ++z) check_zoom(zooms[z], "every zoom of the sweep");
        if (!n_frames || !n_zooms) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        std::vector<double> unit;
        if (targets) unit = unit_targets(targets, n_frames);
        rship_ctx* c = device(p);
        if (rship_stabilize_coverage(c, frame_times, (uint32_t)n_frames, targets ? unit.data() : nullptr, &cfg, zooms, (uint32_t)n_zooms, outside))
            panic(std::string("hip: stabilize: ") + rship_last_error(c));
    });
}

} // extern "C"
