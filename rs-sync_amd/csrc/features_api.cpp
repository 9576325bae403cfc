// features_api.cpp -- the public feature-tracker entry points (include/rssync_features.h): argument checks, defaults,
// points in fp64, and the hand-over of the kept tracks to rssync_ext_set_track_pixels.  The work runs in
// rship_features_track (track_hip.h).
//
// Linked into the product library only, like track_api.cpp: the CPU test double of the device ABI has no tracker.
#include "../../include/rssync_c.h"
#include "../../include/rssync_features.h"
#include "host_errors.hpp"
#include "track_hip.h"

#include <cmath>
#include <string>
#include <vector>

using rssync_host::guarded;
using rssync_host::panic;
using rssync_host::resolve_track_params;

namespace {

struct Resolved {
    rship_feature_cfg cfg{};
    uint32_t min_tracks = 8;
    size_t n_cells = 0;
};

Resolved resolve(const rssync_feature_params* p, size_t width, size_t height) {
    rssync_feature_params q = p ? *p : rssync_feature_params{};
    Resolved r;
    if (q.lk.grid_step != 0) panic("features: lk.grid_step must be 0 (features replace the grid)");
    const int32_t cell = q.cell ? q.cell : 64, block = q.block ? q.block : 5;
    if (cell < 16 || cell > 128) panic("features: cell must be 16 .. 128 px, not " + std::to_string(cell));
    if (block < 3 || block > 9 || !(block & 1)) panic("features: block must be odd, 3 .. 9, not " + std::to_string(block));
    const double quality = q.quality == 0.0 ? 0.01 : q.quality;
    if (!(quality > 0.0 && quality <= 1.0)) panic("features: quality must be in (0, 1]");
    if (!(q.max_fb_error >= 0.0) || !std::isfinite(q.max_fb_error)) panic("features: max_fb_error must be finite and >= 0");
    if (q.min_tracks < 0) panic("features: min_tracks must be >= 0");
    const uint32_t b = (uint32_t)block / 2 + 1;
    if (width < 2 * b + 1 || height < 2 * b + 1)
        panic("features: a " + std::to_string(width) + " x " + std::to_string(height) + " frame is too small for block " +
              std::to_string(block));
    r.cfg.lk = resolve_track_params(&q.lk, width, height);
    r.cfg.cell = (uint32_t)cell;
    r.cfg.block = (uint32_t)block;
    r.cfg.quality = quality;
    r.cfg.max_fb_error = q.max_fb_error == 0.0 ? 0.5f : (float)q.max_fb_error;
    r.min_tracks = q.min_tracks ? (uint32_t)q.min_tracks : 8;
    r.n_cells = ((width + cell - 1) / cell) * ((height + cell - 1) / cell);
    return r;
}

struct Tracked {
    size_t S = 0;                  // slots per pair
    std::vector<int32_t> points;   // [k][S] {x, y}
    std::vector<uint32_t> counts;
    std::vector<float> flow, flow_b, fb;
    std::vector<uint8_t> status;
    Resolved r;
};

Tracked track(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
              size_t frame_stride, const rssync_feature_params* params) {
    if (!p) panic("features: no problem");
    if (!frames) panic("features: no frames");
    if (n_frames < 2) panic("features: need at least 2 frames");
    if (n_frames > 0xffffffffu || width > 0x7fffffffu || height > 0x7fffffffu) panic("features: too many frames or pixels");
    if (pitch < width) panic("features: pitch " + std::to_string(pitch) + " < width " + std::to_string(width));
    if (frame_stride < pitch * height) panic("features: frame stride smaller than pitch * height");
    Tracked t;
    t.r = resolve(params, width, height);
    t.S = t.r.n_cells;
    const size_t n = (n_frames - 1) * t.S;
    t.points.resize(2 * n);
    t.counts.resize(n_frames - 1);
    t.flow.resize(2 * n);
    t.flow_b.resize(2 * n);
    t.fb.resize(n);
    t.status.resize(n);
    rship_ctx* c = (rship_ctx*)rssync_ext_device_context(p);
    if (!c) panic("features: no device");
    if (rship_features_track(c, frames, (uint32_t)n_frames, pitch, frame_stride, &t.r.cfg, t.points.data(), t.counts.data(), t.flow.data(),
                             t.flow_b.data(), t.status.data(), t.fb.data()))
        panic(std::string("hip: features: ") + rship_last_error(c));
    return t;
}

} // namespace

extern "C" {

int rssync_features_track(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                          size_t frame_stride, const rssync_feature_params* params, double* points_a, double* points_b,
                          uint8_t* status, float* fb_error, uint32_t* counts, size_t cap, size_t* n_cells) {
    return guarded([&] {
        if (!points_a || !points_b || !status || !fb_error || !counts) panic("features: null output pointer");
        const Resolved r = resolve(params, width, height);
        if (n_cells) *n_cells = r.n_cells; // (also when the room is too small: the caller learns what it needs)
        if (r.n_cells > cap)
            panic("features: output room for " + std::to_string(cap) + " features per pair, the frame has " + std::to_string(r.n_cells) +
                  " cells");
        Tracked t = track(p, frames, n_frames, width, height, pitch, frame_stride, params);
        for (size_t k = 0; k + 1 < n_frames; ++k) {
            counts[k] = t.counts[k];
            for (size_t i = 0; i < t.counts[k]; ++i) {
                const size_t s = k * t.S + i, o = k * cap + i;
                const double ax = t.points[2 * s], ay = t.points[2 * s + 1];
                points_a[2 * o] = ax;
                points_a[2 * o + 1] = ay;
                points_b[2 * o] = ax + (double)t.flow[2 * s];
                points_b[2 * o + 1] = ay + (double)t.flow[2 * s + 1];
                status[o] = t.status[s];
                fb_error[o] = t.fb[s];
            }
        }
    });
}

int rssync_features_frames(rssync_problem* p, const uint8_t* frames, size_t n_frames, size_t width, size_t height, size_t pitch,
                           size_t frame_stride, const double* frame_times, int64_t first_frame, const rssync_lens* lens,
                           const rssync_feature_params* params, size_t* n_set) {
    if (n_set) *n_set = 0;
    int rc = guarded([&] {
        if (!lens) panic("features: no lens");
        if (!frame_times) panic("features: no frame times");
        for (size_t k = 0; k < n_frames; ++k)
            if (!std::isfinite(frame_times[k])) panic("features: non-finite frame time at " + std::to_string(k));
    });
    if (rc) return rc;
    Tracked t;
    rc = guarded([&] { t = track(p, frames, n_frames, width, height, pitch, frame_stride, params); });
    if (rc) return rc;
    std::vector<double> a, b;
    for (size_t k = 0; k + 1 < n_frames; ++k) {
        a.clear();
        b.clear();
        for (size_t i = 0; i < t.counts[k]; ++i) {
            const size_t s = k * t.S + i;
            if (t.status[s] != RSSYNC_TRACK_OK) continue;
            const double ax = t.points[2 * s], ay = t.points[2 * s + 1];
            a.insert(a.end(), {ax, ay});
            b.insert(b.end(), {ax + (double)t.flow[2 * s], ay + (double)t.flow[2 * s + 1]});
        }
        const size_t kept = a.size() / 2;
        if (kept < t.r.min_tracks || kept == 0) continue; // (too few to fit a frame: the frame index keeps what it had)
        rc = rssync_ext_set_track_pixels(p, first_frame + (int64_t)k, frame_times[k], frame_times[k + 1], a.data(), b.data(), kept, lens,
                                         (double)height);
        if (rc) return rc;
        if (n_set) ++*n_set;
    }
    return 0;
}

} // extern "C"
