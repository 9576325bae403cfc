// track_api.cpp -- the public tracker entry points (include/rssync_track.h): argument checks, defaults, the grid
// in fp64, and the hand-over to rssync_ext_set_track_pixels.  The work runs in rship_track_frames (track_hip.h).
//
// A file of its own, linked into the product library only: sync_problem.cpp is also linked against the CPU test double
// of the device ABI, which has no tracker.
#include "../../include/rssync_c.h"
#include "../../include/rssync_track.h"
#include "host_errors.hpp"
#include "track_hip.h"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;

namespace rssync_host {

rship_track_cfg resolve_track_params(const rssync_track_params* p, size_t width, size_t height) {
    rssync_track_params q = p ? *p : rssync_track_params{};
    rship_track_cfg c{};
    if (q.grid_step < 0 || q.window < 0 || q.levels < 0 || q.max_iters < 0 || !(q.epsilon >= 0) || !(q.min_eig >= 0))
        panic("track: negative or non-finite parameter");
    c.width = (uint32_t)width;
    c.height = (uint32_t)height;
    c.step = q.grid_step ? (uint32_t)q.grid_step : 200;
    c.window = q.window ? (uint32_t)q.window : 21;
    c.levels = q.levels ? (uint32_t)q.levels : 4;
    c.max_iters = q.max_iters ? (uint32_t)q.max_iters : 30;
    c.epsilon = q.epsilon ? (float)q.epsilon : 0.01f;
    c.min_eig = q.min_eig ? (float)q.min_eig : 1e-4f;
    if (c.window < 3 || c.window > 21 || !(c.window & 1)) panic("track: window must be odd, 3 .. 21");
    if (c.levels > 8) panic("track: at most 8 pyramid levels");
    if (!std::isfinite(q.epsilon) || !std::isfinite(q.min_eig)) panic("track: non-finite parameter");
    uint32_t w = c.width, h = c.height;
    for (uint32_t l = 0; l < c.levels; ++l) {
        if (l) { w = (w + 1) / 2; h = (h + 1) / 2; }
        if (w < 3 || h < 3)
            panic("track: a " + std::to_string(width) + " x " + std::to_string(height) + " frame is too small for " +
                  std::to_string(c.levels) + " pyramid levels");
    }
    return c;
}

} // namespace rssync_host

namespace {

using rssync_host::resolve_track_params;

struct Tracked {
    size_t n_points = 0;
    std::vector<float> flow;
    std::vector<uint8_t> status;
    std::vector<float> residual;
    rship_track_cfg cfg{};
};

Tracked track(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
              size_t frame_stride, const rssync_track_params* params) {
    if (!p) panic("track: no problem");
    if (!frames) panic("track: no frames");
    if (n_frames < 2) panic("track: need at least 2 frames");
    if (n_frames > 0xffffffffu || width > 0x7fffffffu || height > 0x7fffffffu) panic("track: too many frames or pixels");
    if (params && params->grid_step < 0) panic("track: grid step must be >= 1");
    if (pitch < width) panic("track: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
    if (n_frames > 1 && frame_stride < pitch * height) panic("track: frame stride smaller than pitch * height");
    Tracked t;
    t.cfg = resolve_track_params(params, width, height);
    t.n_points = (size_t)((width - 1) / t.cfg.step) * ((height - 1) / t.cfg.step);
    const size_t n = (n_frames - 1) * t.n_points;
    t.flow.resize(2 * n);
    t.status.resize(n);
    t.residual.resize(n);
    rship_ctx* c = (rship_ctx*)rssync_ext_device_context(p);
    if (!c) panic("track: no device");
    if (n && rship_track_frames(c, frames, (uint32_t)n_frames, pitch, frame_stride, &t.cfg, t.flow.data(), t.status.data(), t.residual.data()))
        panic(std::string("hip: track: ") + rship_last_error(c));
    return t;
}

// the driver's grid (core_testcode.cpp:124-132): i over x outside, j over y inside
void grid(const rship_track_cfg& c, double* out) {
    size_t k = 0;
    for (uint32_t i = c.step; i < c.width; i += c.step)
        for (uint32_t j = c.step; j < c.height; j += c.step) {
            out[2 * k] = i;
            out[2 * k + 1] = j;
            ++k;
        }
}

} // namespace

extern "C" {

int rssync_track_points(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                        size_t frame_stride, const rssync_track_params* params, double* points_a, double* points_b,
                        uint8_t* status, float* residual, size_t cap, size_t* n_points) {
    return guarded([&] {
        if (!points_a || !points_b || !status || !residual) panic("track: null output pointer");
        if (params && params->grid_step < 0) panic("track: grid step must be >= 1");
        const size_t step = params && params->grid_step ? (size_t)params->grid_step : 200;
        const size_t want = width && height ? ((width - 1) / step) * ((height - 1) / step) : 0;
        if (n_points) *n_points = want; // (also when the room is too small: the caller learns what it needs)
        if (want > cap) panic("track: output room for " + std::to_string(cap) + " points, the grid has " + std::to_string(want));
        Tracked t = track(p, frames, n_frames, width, height, pitch, frame_stride, params);
        grid(t.cfg, points_a);
        const size_t P = t.n_points;
        for (size_t k = 0; k + 1 < n_frames; ++k)
            for (size_t i = 0; i < P; ++i) {
                const size_t o = k * P + i;
                points_b[2 * o] = points_a[2 * i] + (double)t.flow[2 * o];
                points_b[2 * o + 1] = points_a[2 * i + 1] + (double)t.flow[2 * o + 1];
            }
        std::copy(t.status.begin(), t.status.end(), status);
        std::copy(t.residual.begin(), t.residual.end(), residual);
    });
}

int rssync_track_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                        size_t frame_stride, const double* frame_times, int64_t first_frame, const rssync_lens* lens,
                        const rssync_track_params* params) {
    int rc = guarded([&] {
        if (!lens) panic("track: no lens");
        if (!frame_times) panic("track: no frame times");
        for (size_t k = 0; k < n_frames; ++k)
            if (!std::isfinite(frame_times[k])) panic("track: non-finite frame time at " + std::to_string(k));
    });
    if (rc) return rc;
    Tracked t;
    rc = guarded([&] { t = track(p, frames, n_frames, width, height, pitch, frame_stride, params); });
    if (rc) return rc;
    const size_t P = t.n_points;
    std::vector<double> a(2 * P), b(2 * P);
    grid(t.cfg, a.data());
    for (size_t k = 0; k + 1 < n_frames; ++k) {
        for (size_t i = 0; i < P; ++i) {
            b[2 * i] = a[2 * i] + (double)t.flow[2 * (k * P + i)];
            b[2 * i + 1] = a[2 * i + 1] + (double)t.flow[2 * (k * P + i) + 1];
        }
        rc = rssync_ext_set_track_pixels(p, first_frame + (int64_t)k, frame_times[k], frame_times[k + 1], a.data(), b.data(), P, lens,
                                         (double)height);
        if (rc) return rc;
    }
    return 0;
}

} // extern "C"
