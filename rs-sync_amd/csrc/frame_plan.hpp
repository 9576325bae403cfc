// frame_plan.hpp -- how a call of a frame front door (rectify, stabilise, zoom, colour, infill) is cut into chunks and
// where a chunk's row tables and planes lie in its slot (the host side of DESIGN.md "The frame pipeline").  Pure
// arithmetic on plain numbers, no HIP: included by rssync_kernels.hip (frame_pipeline runs the plan) and compiled on its
// own by tests/test_frame_plan.py.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace rs {

// Device bytes a call may hold for host frames on their way in and out and for the row tables: two chunk slots (the one
// the kernels work in, the one the next upload fills) share it.  Not a knob of the product: a chunk is as many frames as
// fit, at least one (the front doors' budget_bytes exists for the tests).
constexpr size_t kRectBudget = 256ull << 20;
constexpr uint32_t kRectMaxChunk = 32768; // frames of a chunk are the grid's z

struct FramePlane {
    size_t row_bytes = 0;
    uint32_t rows = 0;
    size_t bytes() const { return row_bytes * rows; }
};

// what a front door asks for (n_frames >= 1, tab[0] > 0)
struct FrameLayout {
    uint32_t n_frames = 0;
    size_t budget = 0;       // device bytes for both slots; 0: kRectBudget
    size_t tab[2] = {0, 0};  // bytes of one row table of each region (4:2:0: luma, chroma); 0: no such region
    uint32_t tabs = 1;       // tables per output frame and region (infill: one per place, 2 radius + 1)
    int n_in = 0, n_out = 0; // planes that pass through the slot; 0: that side is device memory, read or written in place
    FramePlane in[3], out[3];
    uint32_t radius = 0;     // input frames a chunk reads on each side of its own (infill's halo)
};

// a slot: the table regions, each rounded up to 256 bytes; the input planes, packed [held][rows][row_bytes]; the
// output planes, packed [chunk][rows][row_bytes]
struct FramePlan : FrameLayout {
    uint32_t chunk = 0;      // output frames of a chunk
    uint32_t held = 0;       // input frames a slot holds: the chunk's and its halo's
    size_t off_tab[2] = {0, 0}, off_in[3] = {0, 0, 0}, off_out[3] = {0, 0, 0};
    size_t slot_bytes = 0;
    bool two_slots = false;  // the call has more than one chunk
};

// A chunk is as many output frames as half the budget pays for, at least one: a frame costs its tables and every plane
// that passes through the slot, and a slot the halo's input frames besides.
inline FramePlan plan_frames(const FrameLayout& q) {
    FramePlan p;
    static_cast<FrameLayout&>(p) = q;
    size_t in_bytes = 0, out_bytes = 0;
    for (int k = 0; k < q.n_in; ++k) in_bytes += q.in[k].bytes();
    for (int k = 0; k < q.n_out; ++k) out_bytes += q.out[k].bytes();
    const size_t per_frame = q.tabs * (q.tab[0] + q.tab[1]) + in_bytes + out_bytes;
    const size_t halo = (size_t)std::min<uint64_t>(2 * (uint64_t)q.radius, q.n_frames - 1) * in_bytes;
    const size_t half = (q.budget ? q.budget : kRectBudget) / 2;
    p.chunk = (uint32_t)std::min<uint64_t>(std::min(q.n_frames, kRectMaxChunk), std::max<uint64_t>(1, (half > halo ? half - halo : 0) / per_frame));
    p.held = (uint32_t)std::min<uint64_t>(q.n_frames, (uint64_t)p.chunk + 2 * (uint64_t)q.radius);
    size_t off = 0;
    for (int i = 0; i < 2; ++i) { p.off_tab[i] = off; off += ((size_t)p.chunk * q.tabs * q.tab[i] + 255) / 256 * 256; }
    for (int k = 0; k < q.n_in; ++k) { p.off_in[k] = off; off += (size_t)p.held * q.in[k].bytes(); }
    for (int k = 0; k < q.n_out; ++k) { p.off_out[k] = off; off += (size_t)p.chunk * q.out[k].bytes(); }
    p.slot_bytes = off;
    p.two_slots = q.n_frames > p.chunk;
    return p;
}

} // namespace rs
