// colorsample.hpp -- the samplers of the colour front: every load and every tap of the kernels that render colour frames
// (kernels/color.hpp, color16.hpp, resample.hpp, colorzoom.hpp, colorinfill.hpp).  Part of the single HIP translation unit
// rssync_kernels.hip, before kernels/color.hpp.  A sampler takes the plane of the frame it reads, the plane's pitch in bytes
// and size in samples, and an inside position; which frame that is and how the position was found is the caller's.  All
// arithmetic on the taps is color_math.hpp's (FILTER 0, bilinear) and resample_math.hpp's (FILTER 1, bicubic).
//
//   color_load16 / 32, color_store16 / 32  byte copies of that width: rows and pointers of a caller's planes need no
//                                          alignment, the target issues one access whatever the address
//   color16_sample<SHIFT>                  four taps of a plane of 16-bit words -> the stored word; SHIFT 6 is P010's
//                                          container (the value in the ten high bits), 0 everything else
//   cubic8_sample                          sixteen taps of a plane of bytes
//   cubic16_pairs<SHIFT>                   sixteen taps of a plane of pairs of 16-bit words, every tap one 32-bit load
//   sample_luma8<F>, sample_luma16<SH, F>  one sample of a plane of bytes / of 16-bit words
//   sample_uv8<NV12, F>                    U and V at one position: NV12 every tap one 16-bit load of the interleaved pair,
//                                          I420 two planes
//   sample_uv16<SEMI, SH, F>               the same for 16-bit words: SEMI (P010, P016) every tap one 32-bit load of the
//                                          pair, planar (I010) two planes
//   sample_rgba8<F>                        every tap one 32-bit load, the four channels on one set of weights
//
// Bicubic taps are per-thread loads through four clamped column offsets and four clamped row pointers, each computed once
// per position, not an LDS tile ("Bicubic taps").  One path for every inside pixel: the clamps are two
// instructions per offset, and one path means one set of bits.  The blends run row by row -- a row's four taps become one
// float per channel before the next row is touched -- so a position holds four floats per channel, and no kernel needs scratch.
#pragma once

namespace {

__device__ inline uint32_t color_load16(const uint8_t* p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}
__device__ inline uint32_t color_load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ inline void color_store16(uint8_t* p, uint32_t v) {
    const uint16_t s = (uint16_t)v;
    __builtin_memcpy(p, &s, 2);
}
__device__ inline void color_store32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// the four taps of one plane of 16-bit words at an inside position -> the stored word of the result
template <int SHIFT>
__device__ inline uint32_t color16_sample(const uint8_t* plane, uint64_t pitch, const rs::ColorTaps& t) {
    const uint8_t* p = plane + (size_t)t.y0 * pitch + 2 * (size_t)t.x0;
    const uint32_t p00 = color_load16(p) >> SHIFT, p01 = color_load16(p + 2) >> SHIFT;
    const uint32_t p10 = color_load16(p + pitch) >> SHIFT, p11 = color_load16(p + pitch + 2) >> SHIFT;
    return (uint32_t)rs::color_blend16((float)p00, (float)p01, (float)p10, (float)p11, t.fx, t.fy) << SHIFT;
}

// one plane of bytes, the taps given
__device__ inline uint32_t cubic8_sample(const uint8_t* plane, uint64_t pitch, const rs::CubicTaps& t) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = plane + (size_t)t.y[j] * pitch;
        r[j] = rs::cubic_row((float)p[t.x[0]], (float)p[t.x[1]], (float)p[t.x[2]], (float)p[t.x[3]], t.wx);
    }
    return rs::cubic_finish(r[0], r[1], r[2], r[3], t.wy, 255.0f);
}

// a plane of pairs of 16-bit words (P010 / P016 chroma), every tap one 32-bit load -> the two results' stored words
template <int SHIFT>
__device__ inline void cubic16_pairs(const uint8_t* plane, uint64_t pitch, const rs::CubicTaps& t, float vmax, uint32_t* lo, uint32_t* hi) {
    float a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t* p = plane + (size_t)t.y[j] * pitch;
        const uint32_t p0 = color_load32(p + 4 * (size_t)t.x[0]), p1 = color_load32(p + 4 * (size_t)t.x[1]);
        const uint32_t p2 = color_load32(p + 4 * (size_t)t.x[2]), p3 = color_load32(p + 4 * (size_t)t.x[3]);
        a[j] = rs::cubic_row((float)((p0 & 0xffffu) >> SHIFT), (float)((p1 & 0xffffu) >> SHIFT), (float)((p2 & 0xffffu) >> SHIFT),
                             (float)((p3 & 0xffffu) >> SHIFT), t.wx);
        b[j] = rs::cubic_row((float)(p0 >> (16 + SHIFT)), (float)(p1 >> (16 + SHIFT)), (float)(p2 >> (16 + SHIFT)), (float)(p3 >> (16 + SHIFT)),
                             t.wx);
    }
    *lo = rs::cubic_finish(a[0], a[1], a[2], a[3], t.wy, vmax) << SHIFT;
    *hi = rs::cubic_finish(b[0], b[1], b[2], b[3], t.wy, vmax) << SHIFT;
}

template <int FILTER>
__device__ __forceinline__ uint32_t sample_luma8(const uint8_t* src, uint64_t pitch, int w, int h, float x, float y) {
    if (FILTER == 0) return rs::rect_sample(src, (size_t)pitch, w, h, x, y);
    return cubic8_sample(src, pitch, rs::cubic_taps(w, h, x, y));
}

// U and V of an 8-bit chroma plane pair: pu the interleaved plane (NV12) or U's, pv V's
template <bool NV12, int FILTER>
__device__ __forceinline__ void sample_uv8(const uint8_t* pu, uint64_t pitch_u, const uint8_t* pv, uint64_t pitch_v, int cw, int ch, float x,
                                           float y, uint32_t* cb, uint32_t* cr) {
    if (FILTER == 0) {
        const rs::ColorTaps t = rs::color_taps(cw, ch, x, y);
        if (NV12) {
            const uint8_t* p = pu + (size_t)t.y0 * pitch_u + 2 * (size_t)t.x0;
            const uint32_t p00 = color_load16(p), p01 = color_load16(p + 2);
            const uint32_t p10 = color_load16(p + pitch_u), p11 = color_load16(p + pitch_u + 2);
            *cb = rs::color_blend((float)(p00 & 255u), (float)(p01 & 255u), (float)(p10 & 255u), (float)(p11 & 255u), t.fx, t.fy);
            *cr = rs::color_blend((float)(p00 >> 8), (float)(p01 >> 8), (float)(p10 >> 8), (float)(p11 >> 8), t.fx, t.fy);
        } else {
            const uint8_t* p = pu + (size_t)t.y0 * pitch_u + t.x0;
            const uint8_t* q = pv + (size_t)t.y0 * pitch_v + t.x0;
            *cb = rs::color_blend((float)p[0], (float)p[1], (float)p[pitch_u], (float)p[pitch_u + 1], t.fx, t.fy);
            *cr = rs::color_blend((float)q[0], (float)q[1], (float)q[pitch_v], (float)q[pitch_v + 1], t.fx, t.fy);
        }
    } else {
        const rs::CubicTaps t = rs::cubic_taps(cw, ch, x, y);
        if (NV12) {
            float a[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t* p = pu + (size_t)t.y[j] * pitch_u;
                const uint32_t p0 = color_load16(p + 2 * (size_t)t.x[0]), p1 = color_load16(p + 2 * (size_t)t.x[1]);
                const uint32_t p2 = color_load16(p + 2 * (size_t)t.x[2]), p3 = color_load16(p + 2 * (size_t)t.x[3]);
                a[j] = rs::cubic_row((float)(p0 & 255u), (float)(p1 & 255u), (float)(p2 & 255u), (float)(p3 & 255u), t.wx);
                b[j] = rs::cubic_row((float)(p0 >> 8), (float)(p1 >> 8), (float)(p2 >> 8), (float)(p3 >> 8), t.wx);
            }
            *cb = rs::cubic_finish(a[0], a[1], a[2], a[3], t.wy, 255.0f);
            *cr = rs::cubic_finish(b[0], b[1], b[2], b[3], t.wy, 255.0f);
        } else {
            *cb = cubic8_sample(pu, pitch_u, t);
            *cr = cubic8_sample(pv, pitch_v, t);
        }
    }
}

template <int SHIFT, int FILTER>
__device__ __forceinline__ uint32_t sample_luma16(const uint8_t* src, uint64_t pitch, int w, int h, float x, float y, float vmax) {
    if (FILTER == 0) return color16_sample<SHIFT>(src, pitch, rs::color_taps(w, h, x, y));
    return rs::cubic_sample16<SHIFT>(src, (size_t)pitch, rs::cubic_taps(w, h, x, y), vmax);
}

// U and V of a 16-bit chroma plane pair -> their stored words
template <bool SEMI, int SHIFT, int FILTER>
__device__ __forceinline__ void sample_uv16(const uint8_t* pu, uint64_t pitch_u, const uint8_t* pv, uint64_t pitch_v, int cw, int ch, float x,
                                            float y, float vmax, uint32_t* cb, uint32_t* cr) {
    if (FILTER == 0) {
        const rs::ColorTaps t = rs::color_taps(cw, ch, x, y);
        if (SEMI) {
            const uint8_t* p = pu + (size_t)t.y0 * pitch_u + 4 * (size_t)t.x0;
            const uint32_t p00 = color_load32(p), p01 = color_load32(p + 4);
            const uint32_t p10 = color_load32(p + pitch_u), p11 = color_load32(p + pitch_u + 4);
            *cb = (uint32_t)rs::color_blend16((float)((p00 & 0xffffu) >> SHIFT), (float)((p01 & 0xffffu) >> SHIFT),
                                              (float)((p10 & 0xffffu) >> SHIFT), (float)((p11 & 0xffffu) >> SHIFT), t.fx, t.fy)
                  << SHIFT;
            *cr = (uint32_t)rs::color_blend16((float)(p00 >> (16 + SHIFT)), (float)(p01 >> (16 + SHIFT)), (float)(p10 >> (16 + SHIFT)),
                                              (float)(p11 >> (16 + SHIFT)), t.fx, t.fy)
                  << SHIFT;
        } else {
            *cb = color16_sample<SHIFT>(pu, pitch_u, t);
            *cr = color16_sample<SHIFT>(pv, pitch_v, t);
        }
    } else {
        const rs::CubicTaps t = rs::cubic_taps(cw, ch, x, y);
        if (SEMI) {
            cubic16_pairs<SHIFT>(pu, pitch_u, t, vmax, cb, cr);
        } else {
            *cb = rs::cubic_sample16<SHIFT>(pu, (size_t)pitch_u, t, vmax);
            *cr = rs::cubic_sample16<SHIFT>(pv, (size_t)pitch_v, t, vmax);
        }
    }
}

// the four channels of an RGBA32 pixel on one set of weights
template <int FILTER>
__device__ __forceinline__ uint32_t sample_rgba8(const uint8_t* plane, uint64_t pitch, int w, int h, float x, float y) {
    uint32_t px = 0;
    if (FILTER == 0) {
        const rs::ColorTaps t = rs::color_taps(w, h, x, y);
        const uint8_t* p = plane + (size_t)t.y0 * pitch + 4 * (size_t)t.x0;
        const uint32_t p00 = color_load32(p), p01 = color_load32(p + 4);
        const uint32_t p10 = color_load32(p + pitch), p11 = color_load32(p + pitch + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 8 * k;
            px |= (uint32_t)rs::color_blend((float)((p00 >> s) & 255u), (float)((p01 >> s) & 255u), (float)((p10 >> s) & 255u),
                                            (float)((p11 >> s) & 255u), t.fx, t.fy)
                  << s;
        }
    } else {
        const rs::CubicTaps t = rs::cubic_taps(w, h, x, y);
        float r[4][4]; // [channel][row]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t* p = plane + (size_t)t.y[j] * pitch;
            const uint32_t p0 = color_load32(p + 4 * (size_t)t.x[0]), p1 = color_load32(p + 4 * (size_t)t.x[1]);
            const uint32_t p2 = color_load32(p + 4 * (size_t)t.x[2]), p3 = color_load32(p + 4 * (size_t)t.x[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 8 * k;
                r[k][j] = rs::cubic_row((float)((p0 >> s) & 255u), (float)((p1 >> s) & 255u), (float)((p2 >> s) & 255u),
                                        (float)((p3 >> s) & 255u), t.wx);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) px |= rs::cubic_finish(r[k][0], r[k][1], r[k][2], r[k][3], t.wy, 255.0f) << (8 * k);
    }
    return px;
}

} // namespace
