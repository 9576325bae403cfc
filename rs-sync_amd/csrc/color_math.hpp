// color_math.hpp -- the arithmetic of colour stabilisation (include/rssync_color.h) that the stabiliser does not already
// have: where a 4:2:0 chroma sample looks, and the rectifier's bilinear sampler taken apart so that one position serves
// several channels.  RS_LHD and contraction off like stabilize_math.hpp, whose functions do the rest (stab_row_matrix,
// stab_pinhole_ray, stab_start_row, rect_map_pixel, rect_inside): the host (color_api.cpp) forms the chroma camera with
// these functions, the kernels (kernels/color.hpp) sample with them.
//
//   siting  chroma sample (cu, cv) sits at luma position (2 cu + ox, 2 cv + oy): CENTER (0.5, 0.5), LEFT (0, 0.5)
//   lens    fx * 0.5, fy * 0.5, (cx - ox) * 0.5, (cy - oy) * 0.5; ro, k1 .. k4 unchanged        fp64 (color_chroma_camera)
//   time    T_c = T + ro * (oy / height)                                                       fp64 (color_chroma_time)
//   4:2:2   (2 cu + ox, cv): fx * 0.5, fy, (cx - ox) * 0.5, cy; T_c = T                        fp64 (color_chroma422_*)
//   sample  rect_sample's taps and weights (color_taps) and its blend of four values (color_blend): bit for bit
//   16 bit  the same blend on uint16 sample values (color_blend16), and P010's container: value = word >> 6, word = value << 6
#pragma once

#include <math.h>
#include <stdint.h>

#include "stabilize_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rs {

// the offset of chroma sample (0, 0) in luma pixels: site 0 = centre, 1 = left
RS_LHD void color_chroma_offset(int site, double* ox, double* oy) {
    *ox = site == 1 ? 0.0 : 0.5;
    *oy = 0.5;
}

// a camera (fx, fy, cx, cy) of the luma grid as the camera of the chroma grid
RS_LHD void color_chroma_camera(const double* cam, double ox, double oy, double* out) {
    out[0] = cam[0] * 0.5;
    out[1] = cam[1] * 0.5;
    out[2] = (cam[2] - ox) * 0.5;
    out[3] = (cam[3] - oy) * 0.5;
}

// the frame time of the chroma plane: its row 0 lies oy luma rows below the frame's
RS_LHD double color_chroma_time(double frame_time, double ro, double oy, double height) { return frame_time + ro * (oy / height); }

// 4:2:2 (include/rssync_yuv.h): chroma sample (cu, cv) sits at luma position (2 cu + ox, cv), the plane is halved in x alone
RS_LHD void color_chroma422_offset(int site, double* ox) { *ox = site == 1 ? 0.0 : 0.5; }

// a camera (fx, fy, cx, cy) of the luma grid as the camera of the 4:2:2 chroma grid: x halved, y kept
RS_LHD void color_chroma422_camera(const double* cam, double ox, double* out) {
    out[0] = cam[0] * 0.5;
    out[1] = cam[1];
    out[2] = (cam[2] - ox) * 0.5;
    out[3] = cam[3];
}

// the frame time of a 4:2:2 chroma plane: its rows are the luma's
RS_LHD double color_chroma422_time(double frame_time) { return frame_time; }

// rect_sample's taps of an inside position: the upper left tap and the two weights
struct ColorTaps {
    int x0, y0;
    float fx, fy;
};

RS_LHD ColorTaps color_taps(int width, int height, float x, float y) {
    int x0 = (int)floorf(x), y0 = (int)floorf(y);
    x0 = x0 < width - 2 ? x0 : width - 2;
    y0 = y0 < height - 2 ? y0 : height - 2;
    return ColorTaps{x0, y0, x - (float)x0, y - (float)y0};
}

// ... and its blend of the four taps' values, every operation rounded on its own
RS_LHD uint8_t color_blend(float p00, float p01, float p10, float p11, float fx, float fy) {
    const float top = p00 + fx * (p01 - p00);
    const float bot = p10 + fx * (p11 - p10);
    const float val = top + fy * (bot - top);
    return (uint8_t)rintf(val);
}

// the blend on the sample values of a 16-bit container (include/rssync_color16.h): color_blend's three operations in its
// order.  Every operation is monotone in its rounding, so the result lies within the four taps' range: no clamp.
RS_LHD uint16_t color_blend16(float p00, float p01, float p10, float p11, float fx, float fy) {
    const float top = p00 + fx * (p01 - p00);
    const float bot = p10 + fx * (p11 - p10);
    const float val = top + fy * (bot - top);
    return (uint16_t)rintf(val);
}

// P010: ten bits in the high end of the word; the low six are ignored on input and zero on output
RS_LHD uint32_t color_p010_unpack(uint32_t word) { return word >> 6; }
RS_LHD uint32_t color_p010_pack(uint32_t value) { return value << 6; }

} // namespace rs

// (end of the contraction-off region, as in rectify_math.hpp)
#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif
