// lens_math.hpp -- pixel -> (unit ray, row time) for one tracked point, in fp64.
//
// The step upstream of SetTrackResult in the reference driver:
//   undistort_point   src/core_testcode.cpp:63-95  (Newton inverse of the 4-coefficient fisheye
//                     polynomial, 9 iterations from pi/4, halving back into (0, pi/2); written
//                     here in Horner form, see the function)
//   row_time          :144-145  ts = frame_time + readout * (pixel_y / image_rows)
//   unit_ray          :147-152  normalise([x_u, y_u, 1])
// RS_HD like device_math.hpp: the kernel (pack_frames_kernel's pixel branch) inlines these, the CPU
// test double compiles the same text with g++.  Contraction is switched off so that device and
// test double perform the same IEEE operations in the same order; between them only the libm
// behind tan/cos differs.  The oracle restates the reference's text instead (expanded powers,
// error * (1 / slope) where this file has Horner's rule and (model - rd) / slope), so its rays
// are NOT the same operations: measured on the CPU over 200 000 points per lens, the fp64 unit
// rays of the two differ by at most 6.9e-16 inside the image (8.9e-16 in a margin of half an
// image) and no fp32 component differs inside the image; beyond the model's range, where z is
// ~1e-10, up to 1.2 % of the points differ in fp32 bits, by at most 1.5e-11.  row_time IS the
// same operations as the oracle's and its results compare bit for bit; knot_offset has no
// counterpart in the oracle (every route of the library goes through it), so its fp32 results
// are compared bit for bit with a numpy restatement that rounds every operation on its own
// (tests/test_pixel_front_door.py, tests/pixel_cases.py: restated_offsets).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_LHD __host__ __device__ inline
#else
#define RS_LHD inline
#endif

namespace rs {

struct Lens { // core_testcode.cpp:55-61
    double ro;             // rolling-shutter readout time of a frame, seconds
    double fx, fy, cx, cy; // pinhole part, pixels
    double k1, k2, k3, k4; // fisheye polynomial
};

// Inverse of the fisheye model  rd = th * (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8)  by the
// reference's fixed schedule (core_testcode.cpp:63-95): nine Newton steps from pi/4, each step
// pulled back towards the previous iterate by halving while it lies outside (0, pi/2).  Both
// polynomials are evaluated by Horner's rule in q = th^2 (the reference expands the powers
// th^2 .. th^9 one by one; the two forms agree to a few fp64 ulps, far below the fp32 result).
// The slope polynomial keeps the reference's coefficient 8 on k4 (:80; the exact derivative has
// 9): it changes the path of the iteration, not its fixed point.
RS_LHD void undistort_point(const Lens& lens, double px, double py, double* ux, double* uy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double kPi = 3.14159265358979323846;
    *ux = 0;
    *uy = 0;
    if (sqrt(px * px + py * py) < 1e-8) return; // :64 tests the PIXEL position, not the centred one
    const double xn = (px - lens.cx) / lens.fx, yn = (py - lens.cy) / lens.fy;
    const double rd = sqrt(xn * xn + yn * yn); // distorted angle the model must reproduce
    double th = kPi / 4.;
    for (int step = 0; step < 9; ++step) {
        const double q = th * th;
        const double model = th * (1. + q * (lens.k1 + q * (lens.k2 + q * (lens.k3 + q * lens.k4))));
        const double slope = 1. + q * (3. * lens.k1 + q * (5. * lens.k2 + q * (7. * lens.k3 + q * (8. * lens.k4))));
        double next = th - (model - rd) / slope;
        // the midpoints approach th, which lies inside the interval, and reach it exactly after at
        // most ~1100 halvings of a finite fp64 distance: the bound only guarantees that a wave leaves
        for (int guard = 0; guard < 1200 && (next <= 0. || next >= kPi / 2.); ++guard) next = 0.5 * (next + th);
        th = next;
    }
    // (x, y) scaled from distorted radius rd to tan(th); at the image centre the ratio is taken as 1 / cos (:91-93)
    const double gain = (rd < 1e-9) ? 1. / cos(th) : tan(th) / rd;
    *ux = xn * gain;
    *uy = yn * gain;
}

// absolute capture time of a point on image row py (:144-145): the frame's time plus the readout's share of the rows
// above it.  The one expression of it: the packing kernel, the re-timing kernel (a new readout, rays unchanged) and the
// CPU test double all evaluate this text, so that a re-timed stream has the bits of a repacked one.
RS_LHD double row_time(double ro, double py, double frame_time_s, double image_rows) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return frame_time_s + ro * (py / image_rows);
}

// one end of a track: pixel -> unit ray (:147-152) and absolute row time (:144-145)
RS_LHD void pixel_to_ray(const Lens& lens, double px, double py, double frame_time_s, double image_rows,
                         double* ray, double* ts) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double ux, uy;
    undistort_point(lens, px, py, &ux, &uy);
    const double n = sqrt(ux * ux + uy * uy + 1.);
    const double inv = n > 0 ? n : 1.; // arma::normalise leaves a zero vector alone; cannot happen with z = 1
    ray[0] = ux / inv;
    ray[1] = uy / inv;
    ray[2] = 1. / inv;
    *ts = row_time(lens.ro, py, frame_time_s, image_rows);
}

// spline parameter of a row time relative to the frame's integer base knot
// (sync_problem.cpp pack_frames: (ts - start) * fs - base, core_private.cpp:19-20 without the delay)
RS_LHD double knot_offset(double ts, double start, double fs, double base) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (ts - start) * fs - base;
}

} // namespace rs
