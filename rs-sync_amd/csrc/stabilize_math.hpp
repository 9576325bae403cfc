// stabilize_math.hpp -- the arithmetic of frame stabilisation (include/rssync_stabilize.h) that the rectifier does not
// already have: the smoothed path, the row table against a free target, the output camera's pinhole ray, the start row of
// an output of another size.  RS_LHD and contraction off like rectify_math.hpp, whose functions do the rest (rect_orientation,
// rect_pixel_ray, rect_map_pixel, rect_inside, rect_sample): every fused multiply-add is spelled fma / fmaf.
//
//   path    T_c = T + ro * 0.5 + delay;  t_k = clamp(T_c + k sigma / 64) for k = -192 .. 192;  q_k = q(t_k);
//           acc = sum_k w_k s_k q_k with w_k = exp(-0.5 (k / 64)^2) (tabulated by the host), s_k = -1 where q_k . q_0 < 0;
//           q_s = acc / |acc|                                                    fp64 (stab_tap, stab_finish)
//   table   M_j = R(q(T + ro j / rows + delay)) R(q_target)^T, j = 0 .. rows       fp64, stored fp32 x 9 (stab_row_matrix)
//   ray     LENS: rect_pixel_ray of the output camera;  PINHOLE: stab_pinhole_ray  fp32
//   start   y = v * (rows / out_rows), the factor an fp32 division of the HOST (stab_start_row)
#pragma once

#include <math.h>
#include <stdint.h>

#include "rectify_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rs {

constexpr int kStabHalfTaps = 192;                // taps k = -192 .. 192: three sigma at 64 taps per sigma
constexpr int kStabTaps = 2 * kStabHalfTaps + 1;  // 385
constexpr double kStabTapsPerSigma = 64.0;

// the centre time of a frame: the time of its middle row.  ro * 0.5 is what row_time makes of the rectifier's default
// ref_row, rows / 2 -- (rows / 2) / rows is exactly 0.5 -- so q(T_c) is the rectifier's q_ref to the bit.
RS_LHD double stab_centre_time(double frame_time, double ro, double delay) { return (frame_time + ro * 0.5) + delay; }

// tap i = k + 192 of the path around centre time tc: its weighted, sign-aligned orientation is added to acc[4].
// q0 = q(tc); w = the tap's weight; t_lo, t_hi: the first and last knot time.
RS_LHD void stab_tap(const double* table, int n_knots, double start, double fs, double t_lo, double t_hi, double tc, double sigma, int i,
                     double w, const RectQuat& q0, double* acc) {
    double t = tc + (double)(i - kStabHalfTaps) * sigma / kStabTapsPerSigma;
    if (t < t_lo) t = t_lo;
    if (t > t_hi) t = t_hi;
    const RectQuat q = rect_orientation(table, n_knots, start, fs, t);
    const double dot = ((q.w * q0.w + q.x * q0.x) + q.y * q0.y) + q.z * q0.z;
    const double ws = dot < 0.0 ? -w : w;
    acc[0] = fma(ws, q.w, acc[0]);
    acc[1] = fma(ws, q.x, acc[1]);
    acc[2] = fma(ws, q.y, acc[2]);
    acc[3] = fma(ws, q.z, acc[3]);
}

// acc / |acc|
RS_LHD RectQuat stab_finish(const double* acc) {
    const double n = sqrt(((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]) + acc[3] * acc[3]);
    const double inv = n > 0.0 ? 1.0 / n : 0.0;
    return RectQuat{acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv};
}

// entry `row` of a frame's row table against the unit target qt: R(q(row time + delay)) R(qt)^T as nine fp32 values.
// The rectifier's rect_row_matrix with q_ref replaced: with qt = q(T_c) the same bits.
RS_LHD void stab_row_matrix(const double* table, int n_knots, double start, double fs, double ro, double frame_time, double rows,
                            double delay, const RectQuat& qt, double row, float* out9) {
    const RectQuat q = rect_orientation(table, n_knots, start, fs, row_time(ro, row, frame_time, rows) + delay);
    double m[9];
    rect_quat_matrix(rect_quat_mul_conj(q, qt), m);
    for (int k = 0; k < 9; ++k) out9[k] = (float)m[k];
}

// the output camera in fp32 (zoom already in fx, fy)
struct StabCamF { float fx, fy, cx, cy; };

// unit ray of output pixel (u, v) of a pinhole camera, fp32, every operation rounded on its own:
// x = (u - cx) / fx, y = (v - cy) / fy, n = sqrt((x x + y y) + 1), ray = (x / n, y / n, 1 / n)
RS_LHD void stab_pinhole_ray(const StabCamF& cam, float u, float v, float* rx, float* ry, float* rz) {
    const float x = (u - cam.cx) / cam.fx;
    const float y = (v - cam.cy) / cam.fy;
    const float n = sqrtf((x * x + y * y) + 1.0f);
    *rx = x / n;
    *ry = y / n;
    *rz = 1.0f / n;
}

// the row of the input frame the iteration starts from: y_scale = (float)rows / (float)out_rows, divided on the host
// (exactly 1 when the sizes agree, and then the start is v as in the rectifier)
RS_LHD float stab_start_row(float v, float y_scale) { return v * y_scale; }

// border pixel b of a width x height image, b in [0, 2 (width + height) - 4): the top row, the bottom row, then the
// left and the right column without their corners
RS_LHD void stab_border_pixel(uint32_t b, uint32_t width, uint32_t height, uint32_t* u, uint32_t* v) {
    if (b < width) { *u = b; *v = 0; return; }
    b -= width;
    if (b < width) { *u = b; *v = height - 1; return; }
    b -= width;
    if (b < height - 2) { *u = 0; *v = b + 1; return; }
    b -= height - 2;
    *u = width - 1;
    *v = b + 1;
}

} // namespace rs

// (end of the contraction-off region, as in rectify_math.hpp)
#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif
