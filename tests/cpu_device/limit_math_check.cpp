// limit_math_check.cpp -- csrc/limit_math.hpp compiled for the CPU (tests/test_limit_cpu.py): the bisection driver on
// threshold predicates, the blend and the normalisation on fixed quaternions, and the lower envelope on a fitted curve,
// printed as hex floats for the comparison with the numpy restatement (tests/limit_reference.py).  No arguments.
//   b <steps> <c> <strength> <status>           the bisection with clear(a) = a <= c (c = -1: the predicate that is not monotone)
//   m <pair> <a> <c.w> <c.x> <c.y> <c.z>        the blend of pair `pair` of the quaternions below at strength a
//   u <pair> <a> <u.w> <u.x> <u.y> <u.z> <n>    ... normalised, and its norm
//   w <strength>                                the envelope of the curve below at window 0.1 s, one line per frame
//   c <strength>                                ... at window 0: the copy
//   k <strength>                                the envelope of a constant curve
#include <cstdio>
#include <vector>

#include "../../rs-sync_amd/csrc/limit_math.hpp"

int main() {
    const double cs[] = {-0.25, 0.0, 0.0009765625, 0.3, 0.4023437, 0.5, 0.630859375, 0.87, 0.9999, 1.0, 1.5};
    for (int steps : {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 40})
        for (double c : cs) {
            uint32_t status = 7;
            const double a = rs::limit_bisect([&](double v) { return v <= c; }, steps, &status);
            printf("b %d %a %a %u\n", steps, c, a, status);
        }
    // a predicate that is not monotone: the procedure, not a search for the edge, defines the result
    for (int steps : {3, 10}) {
        uint32_t status = 7;
        const double a = rs::limit_bisect([&](double v) { return v <= 0.2 || (v >= 0.6 && v < 0.7); }, steps, &status);
        printf("b %d %a %a %u\n", steps, -1.0, a, status);
    }
    // own orientation, goal: a pair on one side, the goal with the opposite sign, and a goal that is not a unit quaternion
    const double pairs[3][2][4] = {
        {{0.9238795325112867, 0.1, -0.2, 0.31}, {0.88, 0.17, -0.29, 0.33}},
        {{0.9238795325112867, 0.1, -0.2, 0.31}, {-0.88, -0.17, 0.29, -0.33}},
        {{0.3, -0.7, 0.2, 0.61}, {0.66, -1.3, 0.5, 1.1}},
    };
    for (int p = 0; p < 3; ++p)
        for (double a : {0.0, 1.0, 0.5, 0.630859375, 0.0009765625, 0.9990234375}) {
            double c[4], u[4];
            rs::limit_blend(pairs[p][0], pairs[p][1], a, c);
            const double n = rs::limit_unit(c, u);
            printf("m %d %a %a %a %a %a\n", p, a, c[0], c[1], c[2], c[3]);
            printf("u %d %a %a %a %a %a %a\n", p, a, u[0], u[1], u[2], u[3], n);
        }
    const double curve[9] = {1.0, 0.85546875, 0.732421875, 0.783203125, 1.0, 1.0, 1.0, 0.7412109375, 0.6201171875};
    std::vector<double> t(9), e(9), out(9);
    for (int k = 0; k < 9; ++k) t[k] = (double)(31 + k) / 30.0;
    rs::limit_smooth(t.data(), curve, 9, 0.1, e.data(), out.data());
    for (double v : out) printf("w %a\n", v);
    rs::limit_smooth(t.data(), curve, 9, 0.0, e.data(), out.data());
    for (double v : out) printf("c %a\n", v);
    const double flat[9] = {0.625, 0.625, 0.625, 0.625, 0.625, 0.625, 0.625, 0.625, 0.625};
    rs::limit_smooth(t.data(), flat, 9, 0.1, e.data(), out.data());
    for (double v : out) printf("k %a\n", v);
    return 0;
}
