// resample_math.hpp -- the bicubic sampler of the stabiliser and the colour front (include/rssync_stabilize.h, "Sampling";
// RSSYNC_FILTER_BICUBIC): Keys' cubic convolution with a = -0.5 (Catmull-Rom) over 4 x 4 taps with replicated edges.
// RS_LHD and contraction off like color_math.hpp: every operation below is ONE fp32 operation rounded on its own, in the
// order written, no fmaf -- the order the numpy float32 restatement (tests/resample_reference.py) repeats bit for bit.
// The kernels (kernels/resample.hpp) load and unpack the taps; all arithmetic on them is here.
//
//   taps     ix = min(floor(x), width - 2), tx = x - ix (in [0, 1], 1 on the last column only); columns
//            clamp(ix + d, 0, width - 1), d = -1 .. 2; rows likewise                                  (cubic_taps)
//   weights  w0 = ((1 - 0.5 t) t - 0.5) t     w1 = ((1.5 t - 2.5) t) t + 1
//            w2 = ((2 - 1.5 t) t + 0.5) t     w3 = ((0.5 t - 0.5) t) t                                 (cubic_weights)
//            t = 0: (-0, 1, 0, 0), t = 1: (0, 0, 1, 0) exactly: an integer position returns its sample
//   row      r_j = (wx0 p_j0 + wx1 p_j1) + (wx2 p_j2 + wx3 p_j3)                                       (cubic_row)
//   value    rint(min(max((wy0 r_0 + wy1 r_1) + (wy2 r_2 + wy3 r_3), 0), vmax))                        (cubic_finish)
//
// The eight weights belong to the position: every channel sampled there (U and V, R G B A) shares them.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "color_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rs {

RS_LHD void cubic_weights(float t, float* w) {
    w[0] = ((1.0f - 0.5f * t) * t - 0.5f) * t;
    w[1] = ((1.5f * t - 2.5f) * t) * t + 1.0f;
    w[2] = ((2.0f - 1.5f * t) * t + 0.5f) * t;
    w[3] = ((0.5f * t - 0.5f) * t) * t;
}

// the taps of an inside position: four clamped columns, four clamped rows, the weights of both axes
struct CubicTaps {
    int x[4], y[4];
    float wx[4], wy[4];
};

RS_LHD int cubic_clamp(int v, int last) { return v < 0 ? 0 : (v > last ? last : v); }

RS_LHD CubicTaps cubic_taps(int width, int height, float x, float y) {
    int ix = (int)floorf(x), iy = (int)floorf(y);
    ix = ix < width - 2 ? ix : width - 2;
    iy = iy < height - 2 ? iy : height - 2;
    CubicTaps t;
    for (int d = 0; d < 4; ++d) {
        t.x[d] = cubic_clamp(ix + d - 1, width - 1);
        t.y[d] = cubic_clamp(iy + d - 1, height - 1);
    }
    cubic_weights(x - (float)ix, t.wx);
    cubic_weights(y - (float)iy, t.wy);
    return t;
}

// one row of taps
RS_LHD float cubic_row(float p0, float p1, float p2, float p3, const float* wx) {
    return (wx[0] * p0 + wx[1] * p1) + (wx[2] * p2 + wx[3] * p3);
}

// the four rows -> the sample value, clamped to 0 .. vmax (the kernel overshoots) and rounded to even
RS_LHD uint32_t cubic_finish(float r0, float r1, float r2, float r3, const float* wy, float vmax) {
    float val = (wy[0] * r0 + wy[1] * r1) + (wy[2] * r2 + wy[3] * r3);
    val = fminf(fmaxf(val, 0.0f), vmax);
    return (uint32_t)rintf(val);
}

// one plane of bytes at an inside position.  img: the plane's first byte, rows `pitch` bytes apart
RS_LHD uint8_t cubic_sample(const uint8_t* img, size_t pitch, int width, int height, float x, float y) {
    const CubicTaps t = cubic_taps(width, height, x, y);
    float r[4];
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = img + (size_t)t.y[j] * pitch;
        r[j] = cubic_row((float)p[t.x[0]], (float)p[t.x[1]], (float)p[t.x[2]], (float)p[t.x[3]], t.wx);
    }
    return (uint8_t)cubic_finish(r[0], r[1], r[2], r[3], t.wy, 255.0f);
}

RS_LHD uint32_t cubic_load16(const uint8_t* p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// one plane of 16-bit words (rows `pitch` BYTES apart) with the taps given: value = word >> SHIFT, the result's word =
// value << SHIFT (SHIFT 6: P010's container, color_math.hpp).  vmax: 1023 (P010, I010) or 65535 (GRAY16, P016)
template <int SHIFT>
RS_LHD uint32_t cubic_sample16(const uint8_t* img, size_t pitch, const CubicTaps& t, float vmax) {
    float r[4];
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = img + (size_t)t.y[j] * pitch;
        r[j] = cubic_row((float)(cubic_load16(p + 2 * (size_t)t.x[0]) >> SHIFT), (float)(cubic_load16(p + 2 * (size_t)t.x[1]) >> SHIFT),
                         (float)(cubic_load16(p + 2 * (size_t)t.x[2]) >> SHIFT), (float)(cubic_load16(p + 2 * (size_t)t.x[3]) >> SHIFT), t.wx);
    }
    return cubic_finish(r[0], r[1], r[2], r[3], t.wy, vmax) << SHIFT;
}

} // namespace rs

// (end of the contraction-off region, as in color_math.hpp)
#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif
