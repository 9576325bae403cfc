// zoom_math_check.cpp -- csrc/zoom_math.hpp compiled for the CPU (tests/test_zoom_cpu.py): the bisection driver on
// threshold predicates and the envelope on a fitted curve, printed as hex floats for the comparison with the numpy
// restatement (tests/zoom_reference.py).  No arguments.
//   b <lo> <hi> <steps> <c> <zoom> <status>     the bisection with clear(z) = z >= c
//   w <zoom>                                    the envelope of the curve below at window 0.1 s, one line per frame
//   c <zoom>                                    ... at window 0: the copy
#include <cstdio>
#include <vector>

#include "../../rs-sync_amd/csrc/zoom_math.hpp"

int main() {
    const double ranges[][2] = {{1.0, 1.5}, {0.5, 1.5}, {0.3, 0.7}};
    const double cs[] = {0.2, 0.5, 0.75, 0.9111328125, 1.0, 1.0419921875, 1.06, 1.0693359375, 1.2499, 1.4999999, 1.5, 1.6};
    for (const auto& r : ranges)
        for (int steps : {1, 10, 12, 40})
            for (double c : cs) {
                uint32_t status = 7;
                const double z = rs::zoom_bisect([&](double v) { return v >= c; }, r[0], r[1], steps, &status);
                printf("b %a %a %d %a %a %u\n", r[0], r[1], steps, c, z, status);
            }
    // a predicate that is not monotone: the procedure, not a search for the edge, defines the result
    for (int steps : {3, 10}) {
        uint32_t status = 7;
        const double z = rs::zoom_bisect([&](double v) { return v >= 1.4 || (v >= 1.1 && v < 1.2); }, 1.0, 1.5, steps, &status);
        printf("b %a %a %d %a %a %u\n", 1.0, 1.5, steps, -1.0, z, status);
    }
    const double curve[9] = {1.0419921875, 1.0693359375, 1.08203125, 1.0771484375, 1.05517578125,
                             1.037109375, 1.05810546875, 1.07861328125, 1.09423828125};
    std::vector<double> t(9), e(9), out(9);
    for (int k = 0; k < 9; ++k) t[k] = (double)(31 + k) / 30.0;
    rs::zoom_smooth(t.data(), curve, 9, 0.1, e.data(), out.data());
    for (double v : out) printf("w %a\n", v);
    rs::zoom_smooth(t.data(), curve, 9, 0.0, e.data(), out.data());
    for (double v : out) printf("c %a\n", v);
    return 0;
}
