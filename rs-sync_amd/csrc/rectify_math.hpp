// rectify_math.hpp -- the arithmetic of rolling-shutter rectification (include/rssync_rectify.h), one function per
// step of the map.  RS_LHD like lens_math.hpp: the kernels (kernels/rectify.hpp) inline these, and a CPU build can
// compile the same text with g++.  Contraction is off for the whole header; where a fused multiply-add is meant it is
// spelled fma / fmaf, so the bits do not depend on a compiler's choice of what to fuse.
//
// Conventions (the solver's own):
//   orientation  core_private.cpp:24-28: the componentwise cubic spline through the gyro knots, renormalised; a camera ray
//                c at time t sees the world direction R(q(t))^T c (rs::rotate_inv, synth.rotate_inv)
//   row time     rs::row_time: frame_time + ro * (row / rows)
//   lens         rs::Lens; pixel -> ray by rs::pixel_to_ray (the driver's Newton inverse) polished with the true derivative
//                (rect_pixel_ray), ray -> pixel by the closed-form fisheye model
//                theta_d = theta (1 + k1 theta^2 + ... + k4 theta^8) (synth.project)
//
// The map of an output pixel (u, v) of the rectified frame (a global-shutter camera at q_ref):
//   r      = ray(u, v)                                           fp64, stored fp32   (rect_pixel_ray)
//   M_j    = R(q(T + ro j / rows + delay)) R(q_ref)^T, j = 0 .. rows   fp64, stored fp32 x 9 (rect_row_matrix)
//   y <- v;  repeat:  M = lerp(M_floor(y), M_floor(y)+1);  (x, y) = project(M r)     fp32 (rect_map_pixel)
// and the forward direction for a tracked point, closed form in fp64 (rect_forward_point).
#pragma once

#include <math.h>
#include <stdint.h>

#include "lens_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rs {

struct RectQuat { double w, x, y, z; };

// unit orientation at gyro time t: row ci = floor(x) of the fp64 spline table (4 x {w, x, y, z} per knot: value and the
// three polynomial coefficients), x = (t - start) * fs.  x is clamped to the knots [0, n - 1] -- the callers have checked
// that a frame's row times lie inside them, the clamp keeps a stray point's read inside the table -- so no extrapolation
// branch of the reference's spline is ever taken.
RS_LHD RectQuat rect_orientation(const double* table, int n_knots, double start, double fs, double t) {
    double x = (t - start) * fs;
    if (!(x > 0.0)) x = 0.0;
    if (x > (double)(n_knots - 1)) x = (double)(n_knots - 1);
    int ci = (int)floor(x);
    if (ci > n_knots - 2) ci = n_knots - 2;
    const double h = x - (double)ci;
    const double* c = table + (size_t)ci * 16;
    double q[4];
    for (int k = 0; k < 4; ++k) q[k] = fma(fma(fma(c[12 + k], h, c[8 + k]), h, c[4 + k]), h, c[k]);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double inv = n > 0.0 ? 1.0 / n : 0.0;
    return RectQuat{q[0] * inv, q[1] * inv, q[2] * inv, q[3] * inv};
}

// a * conj(b): the rotation R(a) R(b)^T
RS_LHD RectQuat rect_quat_mul_conj(const RectQuat& a, const RectQuat& b) {
    return RectQuat{a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z,
                    -a.w * b.x + a.x * b.w - a.y * b.z + a.z * b.y,
                    -a.w * b.y + a.x * b.z + a.y * b.w - a.z * b.x,
                    -a.w * b.z - a.x * b.y + a.y * b.x + a.z * b.w};
}

// R(p) of a unit quaternion, row-major
RS_LHD void rect_quat_matrix(const RectQuat& p, double* m) {
    const double xx = p.x * p.x, yy = p.y * p.y, zz = p.z * p.z;
    const double xy = p.x * p.y, xz = p.x * p.z, yz = p.y * p.z;
    const double wx = p.w * p.x, wy = p.w * p.y, wz = p.w * p.z;
    m[0] = 1.0 - 2.0 * (yy + zz); m[1] = 2.0 * (xy - wz);       m[2] = 2.0 * (xz + wy);
    m[3] = 2.0 * (xy + wz);       m[4] = 1.0 - 2.0 * (xx + zz); m[5] = 2.0 * (yz - wx);
    m[6] = 2.0 * (xz - wy);       m[7] = 2.0 * (yz + wx);       m[8] = 1.0 - 2.0 * (xx + yy);
}

// entry `row` of a frame's row table: R(q(row time + delay)) R(q_ref)^T as nine fp32 values
RS_LHD void rect_row_matrix(const double* table, int n_knots, double start, double fs, double ro, double frame_time, double rows,
                            double delay, double ref_row, double row, float* out9) {
    const RectQuat q = rect_orientation(table, n_knots, start, fs, row_time(ro, row, frame_time, rows) + delay);
    const RectQuat qr = rect_orientation(table, n_knots, start, fs, row_time(ro, ref_row, frame_time, rows) + delay);
    double m[9];
    rect_quat_matrix(rect_quat_mul_conj(q, qr), m);
    for (int k = 0; k < 9; ++k) out9[k] = (float)m[k];
}

// unit ray of a pixel position.  The driver's undistortion answers the image CENTRE for the pixel position (0, 0) itself
// (core_testcode.cpp:64 tests the pixel, not the centred position); a map has that pixel, so it is asked for as pixel
// (1, 0) of the same lens with its centre one pixel further right: the same centred position.
//
// The driver's nine steps use a slope with 8 k4 where the derivative has 9 k4, so for a lens with a large k4 they stop short
// of the fixed point (1.3e-2 px at the border of a 1520 x 2704 image with k = 0.03, 0.06, -0.06, 0.02), and for a position
// the lens cannot image -- rd beyond the model's largest value on [0, pi/2] -- they park theta near pi/2.  A map needs the
// inverse of rect_project_*, so theta is polished here with kRectPolishSteps plain Newton steps on the true derivative
// and the ray rebuilt from it: on the CPU, over every pixel of eight lenses at 1520 x 2704, two steps leave
// |model(theta) - rd| * max(fx, fy) <= 7.5e-13 px and a third changes nothing; three are taken.  A position whose polished
// theta lies outside (0, pi/2), or whose residual stays above kRectRayResidualPx, gets a NaN ray: rect_map_pixel and
// rect_project_d carry the NaN, and rect_inside is false for it.  kRectRayResidualPx = 1e-10 px lies between what fp64
// converges to (1e-12 px above) and what an fp32 pixel coordinate resolves (7.6e-6 px at 64 .. 128); positions the lens
// cannot image miss it by orders of magnitude (their residual is rd - max model, in pixels).  Within 1e-9 of the centre
// (the driver's own branch: the ray is (xn, yn, 1) normalised whatever theta is) nothing is polished.
constexpr int kRectPolishSteps = 3;
constexpr double kRectRayResidualPx = 1e-10;

RS_LHD void rect_pixel_ray(const Lens& lens, double px, double py, double* ray) {
    double ts;
    Lens l = lens;
    if (px == 0.0 && py == 0.0) {
        px = 1.0;
        l.cx = lens.cx + 1.0;
    }
    pixel_to_ray(l, px, py, 0.0, 1.0, ray, &ts);
    const double xn = (px - l.cx) / l.fx, yn = (py - l.cy) / l.fy;
    const double rd = sqrt(xn * xn + yn * yn);
    if (rd < 1e-9) return;
    double th = atan2(sqrt(ray[0] * ray[0] + ray[1] * ray[1]), ray[2]);
    for (int step = 0; step < kRectPolishSteps; ++step) {
        const double q = th * th;
        const double model = th * (1. + q * (l.k1 + q * (l.k2 + q * (l.k3 + q * l.k4))));
        const double slope = 1. + q * (3. * l.k1 + q * (5. * l.k2 + q * (7. * l.k3 + q * (9. * l.k4))));
        th = th - (model - rd) / slope;
    }
    const double q = th * th;
    const double res = fabs(th * (1. + q * (l.k1 + q * (l.k2 + q * (l.k3 + q * l.k4)))) - rd);
    const double fmax_ = fabs(l.fx) > fabs(l.fy) ? fabs(l.fx) : fabs(l.fy);
    if (!(th > 0.0 && th < 1.57079632679489661923 && res * fmax_ <= kRectRayResidualPx)) {
        ray[0] = ray[1] = ray[2] = NAN;
        return;
    }
    const double s = sin(th) / rd;
    ray[0] = xn * s;
    ray[1] = yn * s;
    ray[2] = cos(th);
}

// the lens in fp32, for the iteration
struct RectLensF { float fx, fy, cx, cy, k1, k2, k3, k4; };

// camera ray -> pixel position, closed form, fp32
RS_LHD void rect_project_f(const RectLensF& L, float rx, float ry, float rz, float* x, float* y) {
    const float h = sqrtf(rx * rx + ry * ry);
    const float th = atan2f(h, rz);
    const float t2 = th * th;
    const float thd = th * (1.0f + t2 * (L.k1 + t2 * (L.k2 + t2 * (L.k3 + t2 * L.k4))));
    const float s = h > 0.0f ? thd / h : 0.0f;
    *x = L.fx * (s * rx) + L.cx;
    *y = L.fy * (s * ry) + L.cy;
}

// ... and in fp64 (the forward direction of tracked points)
RS_LHD void rect_project_d(const Lens& L, double rx, double ry, double rz, double* x, double* y) {
    const double h = sqrt(rx * rx + ry * ry);
    const double th = atan2(h, rz);
    const double t2 = th * th;
    const double thd = th * (1.0 + t2 * (L.k1 + t2 * (L.k2 + t2 * (L.k3 + t2 * L.k4))));
    const double s = h > 0.0 ? thd / h : 0.0;
    *x = L.fx * (s * rx) + L.cx;
    *y = L.fy * (s * ry) + L.cy;
}

// source position of the output pixel on row v whose ray is (rx, ry, rz): `iterations` rounds of "the matrix of the row
// the position lies on, then project".  rows_tab: the frame's rows + 1 matrices.
RS_LHD void rect_map_pixel(const float* rows_tab, int rows, const RectLensF& L, int iterations, float v, float rx, float ry, float rz,
                           float* sx, float* sy) {
    float x = 0.0f, y = v;
    const float top = (float)(rows - 1);
    for (int it = 0; it < iterations; ++it) {
        float yc = y < top ? y : top;   // (a NaN, or a NaN ray, takes the last row: its position is NaN and is outside)
        yc = yc > 0.0f ? yc : 0.0f;
        const float fl = floorf(yc);
        const float f = yc - fl;
        const float* a = rows_tab + (size_t)(int)fl * 9;
        const float m0 = a[0] + f * (a[9] - a[0]), m1 = a[1] + f * (a[10] - a[1]), m2 = a[2] + f * (a[11] - a[2]);
        const float m3 = a[3] + f * (a[12] - a[3]), m4 = a[4] + f * (a[13] - a[4]), m5 = a[5] + f * (a[14] - a[5]);
        const float m6 = a[6] + f * (a[15] - a[6]), m7 = a[7] + f * (a[16] - a[7]), m8 = a[8] + f * (a[17] - a[8]);
        const float cx = (m0 * rx + m1 * ry) + m2 * rz;
        const float cy = (m3 * rx + m4 * ry) + m5 * rz;
        const float cz = (m6 * rx + m7 * ry) + m8 * rz;
        rect_project_f(L, cx, cy, cz, &x, &y);
    }
    *sx = x;
    *sy = y;
}

RS_LHD bool rect_inside(float x, float y, int width, int height) {
    return x >= 0.0f && x <= (float)(width - 1) && y >= 0.0f && y <= (float)(height - 1);
}

// bilinear sample of an inside position, in the ONE order the float32 restatement uses (tests/rectify_reference.py):
// every operation rounded on its own.  img: the frame's first byte, rows `pitch` bytes apart.
RS_LHD uint8_t rect_sample(const uint8_t* img, size_t pitch, int width, int height, float x, float y) {
    int x0 = (int)floorf(x), y0 = (int)floorf(y);
    x0 = x0 < width - 2 ? x0 : width - 2;
    y0 = y0 < height - 2 ? y0 : height - 2;
    const float fx = x - (float)x0, fy = y - (float)y0;
    const uint8_t* p = img + (size_t)y0 * pitch + x0;
    const float p00 = p[0], p01 = p[1], p10 = p[pitch], p11 = p[pitch + 1];
    const float top = p00 + fx * (p01 - p00);
    const float bot = p10 + fx * (p11 - p10);
    const float val = top + fy * (bot - top);
    return (uint8_t)rintf(val);
}

// rolling-shutter pixel (x, y) of a frame -> its position in the rectified frame:
// project(R(q_ref) R(q(row time of y + delay))^T ray(x, y)), closed form in fp64
RS_LHD void rect_forward_point(const double* table, int n_knots, double start, double fs, const Lens& lens, double frame_time,
                               double rows, double delay, double ref_row, double px, double py, double* ox, double* oy) {
    double ray[3];
    rect_pixel_ray(lens, px, py, ray);
    const RectQuat q = rect_orientation(table, n_knots, start, fs, row_time(lens.ro, py, frame_time, rows) + delay);
    const RectQuat qr = rect_orientation(table, n_knots, start, fs, row_time(lens.ro, ref_row, frame_time, rows) + delay);
    double m[9];
    rect_quat_matrix(rect_quat_mul_conj(qr, q), m); // R(q_ref) R(q)^T
    rect_project_d(lens, m[0] * ray[0] + m[1] * ray[1] + m[2] * ray[2], m[3] * ray[0] + m[4] * ray[1] + m[5] * ray[2],
                   m[6] * ray[0] + m[7] * ray[1] + m[8] * ray[2], ox, oy);
}

} // namespace rs

// (end of the contraction-off region: only the HIP translation unit switches fusion back on, see device_math.hpp)
#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif
