// zoom_math.hpp -- the arithmetic of the dynamic zoom (include/rssync_zoom.h) that the stabiliser does not already have:
// the bisection that finds a frame's smallest clear zoom, and the envelope that smooths the fitted curve.  Plain C++ for
// the host and the device (RS_LHD), contraction off like stabilize_math.hpp; compiled for the CPU by
// tests/cpu_device/zoom_math_check.cpp.
//
//   fit     clear(hi) false: hi, status 1;  clear(lo): lo;  else `steps` times mid = 0.5 (lo + hi), clear(mid) ? hi = mid
//           : lo = mid; the result is hi.  The procedure defines the result: nothing assumes that clear is monotone
//           (zoom_bisect; the kernel and the CPU check run this one function with predicates of their own)
//   smooth  e[f] = max of z over W(f) = { g : |t_g - t_f| <= window };  s[f] = sum_W k e / sum_W k, ascending g, with
//           k(d) = exp(-0.5 (3 d / window)^2);  out[f] = max(min(s[f], max_W e), z[f]): a mean of the e lies between z[f]
//           and their maximum, and the two clamps take away what rounding adds    fp64, host only (zoom_smooth)
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "lens_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rs {

constexpr int kZoomDefaultSteps = 12, kZoomMaxSteps = 40;
constexpr uint32_t kZoomClear = 0, kZoomNotClear = 1;   // RSSYNC_ZOOM_CLEAR, RSSYNC_ZOOM_NOT_CLEAR

// the step rule
RS_LHD double zoom_mid(double lo, double hi) { return 0.5 * (lo + hi); }

// the smallest clear zoom of one frame in [lo, hi] as the header defines it.  clear(z) -> bool; on the device every
// thread of the workgroup calls this with the same arguments and a predicate that is uniform over the workgroup.
template <class Clear>
RS_LHD double zoom_bisect(Clear&& clear, double lo, double hi, int steps, uint32_t* status) {
    // one call site of the predicate (on the device it is the whole map of a border, inlined): step -2 asks hi, step -1
    // asks lo, steps 0 .. steps - 1 ask the middle
    *status = kZoomClear;
    double z = hi;
    for (int s = -2; s < steps; ++s) {
        const bool ok = clear(z);
        if (s == -2) {
            if (!ok) {
                *status = kZoomNotClear;
                return hi;
            }
            z = lo;
            continue;
        }
        if (s == -1) {
            if (ok) return lo;
        } else if (ok) {
            hi = z;
        } else {
            lo = z;
        }
        z = zoom_mid(lo, hi);
    }
    return hi;
}

// the weight of a frame d seconds away (window > 0)
inline double zoom_weight(double d, double window) {
    const double x = 3.0 * d / window;
    return exp(-0.5 * (x * x));
}

// the envelope of n zooms at non-decreasing times t: never below z, equal to it where window == 0
inline void zoom_smooth(const double* t, const double* z, size_t n, double window, double* e, double* out) {
    if (!(window > 0.0)) {
        for (size_t f = 0; f < n; ++f) out[f] = z[f];
        return;
    }
    // W(f) = [a, b): the times do not decrease, so both ends only move forward
    size_t a = 0, b = 0;
    for (size_t f = 0; f < n; ++f) {
        while (fabs(t[a] - t[f]) > window) ++a;
        if (b < f + 1) b = f + 1;
        while (b < n && fabs(t[b] - t[f]) <= window) ++b;
        double m = z[a];
        for (size_t g = a + 1; g < b; ++g) m = z[g] > m ? z[g] : m;
        e[f] = m;
    }
    a = b = 0;
    for (size_t f = 0; f < n; ++f) {
        while (fabs(t[a] - t[f]) > window) ++a;
        if (b < f + 1) b = f + 1;
        while (b < n && fabs(t[b] - t[f]) <= window) ++b;
        double num = 0.0, den = 0.0, top = e[a];
        for (size_t g = a; g < b; ++g) {
            const double k = zoom_weight(t[g] - t[f], window);
            num = num + k * e[g];
            den = den + k;
            top = e[g] > top ? e[g] : top;
        }
        double s = num / den;
        s = s < top ? s : top;
        out[f] = s > z[f] ? s : z[f];
    }
}

} // namespace rs

// (end of the contraction-off region, as in stabilize_math.hpp)
#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif
