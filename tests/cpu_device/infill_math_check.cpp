// infill_math_check.cpp -- csrc/infill_math.hpp compiled for the CPU (tests/test_infill_cpu.py): the candidate lists for
// n = 1 .. 20 frames, every frame f and every radius 0 .. 8, printed for the comparison with the numpy restatement
// (tests/infill_reference.py).  No arguments.
//   c <n> <f> <radius> : <g0> <g1> ..      rs::infill_candidates; rs::infill_candidate must agree entry by entry and
//                                           return -1 past the end, or the program prints a line starting with "mismatch"
#include <cstdio>
#include <vector>

#include "../../rs-sync_amd/csrc/infill_math.hpp"

int main() {
    for (int n = 1; n <= 20; ++n)
        for (int f = 0; f < n; ++f)
            for (int radius = 0; radius <= rs::kInfillMaxRadius; ++radius) {
                std::vector<int64_t> out(2 * radius + 1);       // exactly what the header promises to need
                const int count = rs::infill_candidates(f, n, radius, out.data());
                printf("c %d %d %d :", n, f, radius);
                for (int k = 0; k < count; ++k) {
                    printf(" %lld", (long long)out[k]);
                    if (rs::infill_candidate(f, n, radius, k) != out[k]) printf("\nmismatch at %d %d %d entry %d\n", n, f, radius, k);
                }
                printf("\n");
                for (int k = count; k <= rs::kInfillMaxCandidates; ++k)
                    if (rs::infill_candidate(f, n, radius, k) != -1) printf("mismatch at %d %d %d past the end %d\n", n, f, radius, k);
            }
    return 0;
}
