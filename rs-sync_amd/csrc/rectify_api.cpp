// rectify_api.cpp -- the public rectifier entry points (include/rssync_rectify.h): argument checks, defaults, the
// check of a frame's row times against the gyro's knots.  The work runs in rship_rectify_* (rectify_hip.h).
//
// A file of its own, linked into the product library only, like track_api.cpp: sync_problem.cpp is also linked against
// the CPU test double of the device ABI, which has no rectifier.
#include "../../include/rssync_c.h"
#include "../../include/rssync_rectify.h"
#include "host_errors.hpp"
#include "rectify_hip.h"

#include <cmath>
#include <string>

using rssync_host::guarded;
using rssync_host::panic;

namespace {

// everything but the frames: the problem's gyro table, the lens, the parameters with their defaults
rship_rectify_cfg resolve(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, double delay,
                          const rssync_rectify_params* params) {
    if (!p) panic("rectify: no problem");
    if (!lens) panic("rectify: no lens");
    if (width < 2 || height < 2) panic("rectify: a " + std::to_string(width) + " x " + std::to_string(height) + " frame is too small (2 x 2 at least)");
    if (width > 65536 || height > 65536) panic("rectify: frames of more than 65536 pixels a side are not supported");
    const double L[9] = {lens->ro, lens->fx, lens->fy, lens->cx, lens->cy, lens->k1, lens->k2, lens->k3, lens->k4};
    for (double v : L)
        if (!std::isfinite(v)) panic("rectify: non-finite lens parameter");
    if (lens->ro < 0) panic("rectify: negative readout time");
    if (lens->fx == 0 || lens->fy == 0) panic("rectify: zero focal length");
    if (!std::isfinite(delay)) panic("rectify: non-finite delay");
    rssync_rectify_params q = params ? *params : rssync_rectify_params{};
    if (q.ref_row == 0 && q.iterations == 0 && q.fill == 0) q.ref_row = -1; // (all zeros: all defaults, rssync_rectify.h)
    rship_rectify_cfg c{};
    c.width = (uint32_t)width;
    c.height = (uint32_t)height;
    for (int i = 0; i < 9; ++i) c.lens[i] = L[i];
    c.delay = delay;
    if (std::isnan(q.ref_row)) panic("rectify: ref_row is not a number");
    c.ref_row = q.ref_row < 0 ? 0.5 * (double)height : q.ref_row;
    if (c.ref_row > (double)height) panic("rectify: ref_row " + std::to_string(q.ref_row) + " outside [0, " + std::to_string(height) + "]");
    c.iterations = q.iterations ? q.iterations : 3;
    if (c.iterations < 1 || c.iterations > 8) panic("rectify: iterations must be 1 .. 8");
    if (q.fill < 0 || q.fill > 255) panic("rectify: fill must be 0 .. 255");
    c.fill = q.fill;
    size_t n_knots = 0;
    rssync_ext_sample_rate(p, &c.fs, &c.start, &n_knots);
    if (n_knots < 2) panic("rectify: no gyro data was set");
    rssync_host::ensure_gyro_table(p);
    c.n_knots = (uint32_t)n_knots;
    return c;
}

// a frame's rows 0 .. rows (and with them ref_row) must lie inside the knots: nothing is extrapolated
void check_frame_time(const rship_rectify_cfg& c, double t, size_t k) {
    if (!std::isfinite(t)) panic("rectify: non-finite frame time at " + std::to_string(k));
    const double x0 = (t + c.delay - c.start) * c.fs, x1 = (t + c.lens[0] + c.delay - c.start) * c.fs;
    if (!(x0 >= 0 && x1 <= (double)(c.n_knots - 1)))
        panic("rectify: frame " + std::to_string(k) + " at " + std::to_string(t) + " s + delay " + std::to_string(c.delay) +
              " s leaves the gyro data (" + std::to_string(c.start) + " .. " + std::to_string(c.start + (c.n_knots - 1) / c.fs) + " s)");
}

rship_ctx* device(rssync_problem* p) {
    rship_ctx* c = (rship_ctx*)rssync_ext_device_context(p);
    if (!c) panic("rectify: no device");
    return c;
}

} // namespace

extern "C" {

int rssync_rectify_map(rssync_problem* p, size_t width, size_t height, const rssync_lens* lens, double frame_time, double delay,
                       const rssync_rectify_params* params, float* map_xy) {
    return guarded([&] {
        if (!map_xy) panic("rectify: null output pointer");
        const rship_rectify_cfg cfg = resolve(p, width, height, lens, delay, params);
        check_frame_time(cfg, frame_time, 0);
        rship_ctx* c = device(p);
        if (rship_rectify_map(c, frame_time, &cfg, map_xy)) panic(std::string("hip: rectify: ") + rship_last_error(c));
    });
}

int rssync_rectify_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                          size_t frame_stride, const double* frame_times, const rssync_lens* lens, double delay,
                          const rssync_rectify_params* params, uint8_t* out, size_t out_pitch, size_t out_stride, uint64_t* n_outside) {
    return guarded([&] {
        if (!frames) panic("rectify: no frames");
        if (!out) panic("rectify: null output pointer");
        if (!frame_times) panic("rectify: no frame times");
        if (n_frames > 0xffffffffu) panic("rectify: too many frames");
        const rship_rectify_cfg cfg = resolve(p, width, height, lens, delay, params);
        if (pitch < width) panic("rectify: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
        if (out_pitch < width) panic("rectify: out_pitch " + std::to_string(out_pitch) + " < width " + std::to_string(width));
        if (n_frames > 1 && (frame_stride < pitch * height || out_stride < out_pitch * height))
            panic("rectify: frame stride smaller than pitch * height");
        if (!n_frames) return;
        for (size_t k = 0; k < n_frames; ++k) check_frame_time(cfg, frame_times[k], k);
        // the two extents, first to last byte
        const uintptr_t a0 = (uintptr_t)frames, a1 = a0 + (n_frames - 1) * frame_stride + (height - 1) * pitch + width;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (n_frames - 1) * out_stride + (height - 1) * out_pitch + width;
        if (a0 < b1 && b0 < a1) panic("rectify: out overlaps the frames");
        rship_ctx* c = device(p);
        if (rship_rectify_frames(c, frames, (uint32_t)n_frames, pitch, frame_stride, frame_times, &cfg, out, out_pitch, out_stride, n_outside, 0))
            panic(std::string("hip: rectify: ") + rship_last_error(c));
    });
}

int rssync_rectify_points(rssync_problem* p, const double* points, size_t count, size_t width, size_t height,
                          const rssync_lens* lens, double frame_time, double delay, const rssync_rectify_params* params, double* out) {
    return guarded([&] {
        if (count && (!points || !out)) panic("rectify: null pointer");
        const rship_rectify_cfg cfg = resolve(p, width, height, lens, delay, params);
        check_frame_time(cfg, frame_time, 0);
        rship_ctx* c = device(p);
        if (rship_rectify_points(c, points, count, frame_time, &cfg, out)) panic(std::string("hip: rectify: ") + rship_last_error(c));
    });
}

} // extern "C"
