// limit_math.hpp -- the arithmetic of the path limiter (include/rssync_limit.h) that the stabiliser and the dynamic zoom do
// not already have: the candidate target between a frame's own orientation and its goal, the normalisation every entry
// point applies to a target, the bisection over the strength, and the lower envelope of a strength curve.  Plain C++ for
// the host and the device (RS_LHD), contraction off like zoom_math.hpp; compiled for the CPU by
// tests/cpu_device/limit_math_check.cpp.
//
//   blend   c(0) = r, c(1) = g, copied;  else d = ((r.w g.w + r.x g.x) + r.y g.y) + r.z g.z, s = d < 0 ? -1 : 1,
//           c_i = (1 - a) r_i + (s a) g_i: five operations a component, each rounded on its own, not normalised (limit_blend)
//   unit    n = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3), u_i = q_i / n: what stabilize_host.hpp's unit_targets does to a
//           caller's target, and what the kernel does to a candidate: one function, so the two cannot drift apart (limit_unit)
//   fit     clear(1): 1;  not clear(0): 0, status 1;  else lo = 0, hi = 1 and `steps` times mid = 0.5 (lo + hi),
//           clear(mid) ? lo = mid : hi = mid; the result is lo.  The procedure defines the result: nothing assumes that
//           clear is monotone (limit_bisect; the kernel and the CPU check run this one function with predicates of their own)
//   smooth  e[f] = min of a over W(f) = { g : |t_g - t_f| <= window };  s[f] = sum_W k e / sum_W k, ascending g, with the
//           zoom envelope's k (zoom_weight);  out[f] = min(max(s[f], min_W e), a[f]): zoom_smooth mirrored
//           fp64, host only (limit_smooth)
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "lens_math.hpp"
#include "zoom_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rs {

constexpr int kLimitDefaultSteps = 12, kLimitMaxSteps = 40;
constexpr uint32_t kLimitClear = 0, kLimitNotClear = 1;   // RSSYNC_LIMIT_CLEAR, RSSYNC_LIMIT_NOT_CLEAR

// the candidate target at strength a in [0, 1] between the frame's own orientation r and its goal g ({w, x, y, z} each)
RS_LHD void limit_blend(const double* r, const double* g, double a, double* c) {
    if (a == 0.0) {
        for (int i = 0; i < 4; ++i) c[i] = r[i];
        return;
    }
    if (a == 1.0) {
        for (int i = 0; i < 4; ++i) c[i] = g[i];
        return;
    }
    const double d = ((r[0] * g[0] + r[1] * g[1]) + r[2] * g[2]) + r[3] * g[3];
    const double s = d < 0.0 ? -1.0 : 1.0;
    const double wr = 1.0 - a, wg = s * a;
    for (int i = 0; i < 4; ++i) c[i] = wr * r[i] + wg * g[i];
}

// u = q / |q|; returns |q| (the host refuses a target whose norm is zero or not finite)
RS_LHD double limit_unit(const double* q, double* u) {
    const double norm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) u[i] = q[i] / norm;
    return norm;
}

// the step rule
RS_LHD double limit_mid(double lo, double hi) { return 0.5 * (lo + hi); }

// the largest clear strength of one frame as the header defines it.  clear(a) -> bool; on the device every thread of the
// workgroup calls this with the same arguments and a predicate that is uniform over the workgroup.
template <class Clear>
RS_LHD double limit_bisect(Clear&& clear, int steps, uint32_t* status) {
    // one call site of the predicate (on the device it is a table rebuild and the whole map of a border, inlined): step
    // -2 asks 1, step -1 asks 0, steps 0 .. steps - 1 ask the middle
    *status = kLimitClear;
    double lo = 0.0, hi = 1.0, a = 1.0;
    for (int s = -2; s < steps; ++s) {
        const bool ok = clear(a);
        if (s == -2) {
            if (ok) return 1.0;
            a = 0.0;
            continue;
        }
        if (s == -1) {
            if (!ok) {
                *status = kLimitNotClear;
                return 0.0;
            }
        } else if (ok) {
            lo = a;
        } else {
            hi = a;
        }
        a = limit_mid(lo, hi);
    }
    return lo;
}

// the lower envelope of n strengths at non-decreasing times t: never above a, equal to it where window == 0
inline void limit_smooth(const double* t, const double* a, size_t n, double window, double* e, double* out) {
    if (!(window > 0.0)) {
        for (size_t f = 0; f < n; ++f) out[f] = a[f];
        return;
    }
    // W(f) = [lo, hi): the times do not decrease, so both ends only move forward
    size_t lo = 0, hi = 0;
    for (size_t f = 0; f < n; ++f) {
        while (fabs(t[lo] - t[f]) > window) ++lo;
        if (hi < f + 1) hi = f + 1;
        while (hi < n && fabs(t[hi] - t[f]) <= window) ++hi;
        double m = a[lo];
        for (size_t g = lo + 1; g < hi; ++g) m = a[g] < m ? a[g] : m;
        e[f] = m;
    }
    lo = hi = 0;
    for (size_t f = 0; f < n; ++f) {
        while (fabs(t[lo] - t[f]) > window) ++lo;
        if (hi < f + 1) hi = f + 1;
        while (hi < n && fabs(t[hi] - t[f]) <= window) ++hi;
        double num = 0.0, den = 0.0, bottom = e[lo];
        for (size_t g = lo; g < hi; ++g) {
            const double k = zoom_weight(t[g] - t[f], window);
            num = num + k * e[g];
            den = den + k;
            bottom = e[g] < bottom ? e[g] : bottom;
        }
        double s = num / den;
        s = s > bottom ? s : bottom;
        out[f] = s < a[f] ? s : a[f];
    }
}

} // namespace rs

// (end of the contraction-off region, as in stabilize_math.hpp)
#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif
