// color16_math_check.cpp -- the 16-bit sampler of csrc/color_math.hpp compiled for the CPU (tests/test_color16_cpu.py):
// color_blend16 against color_blend on 8-bit taps, its result against the range of its taps at the extremes of ten and
// sixteen bits, and P010's container.  No arguments; one line per check: name, cases, failures.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <initializer_list>

#include "../../rs-sync_amd/csrc/color_math.hpp"

int main() {
    // weights: 0, 1, the float below 1, the smallest positive ones, and a sweep
    float w[40];
    int nw = 0;
    w[nw++] = 0.0f;
    w[nw++] = 1.0f;
    w[nw++] = nextafterf(1.0f, 0.0f);
    w[nw++] = nextafterf(0.0f, 1.0f);
    w[nw++] = 0.5f;
    w[nw++] = nextafterf(0.5f, 1.0f);
    w[nw++] = nextafterf(0.5f, 0.0f);
    for (int k = 1; k < 32; ++k) w[nw++] = (float)k / 32.0f + (k % 3 == 1 ? 0.0113f : 0.0f);
    // 1: on taps of at most 255 the 16-bit blend gives color_blend's value
    long n = 0, bad = 0;
    uint32_t s = 2463534242u;
    for (int rep = 0; rep < 4000; ++rep) {
        float p[4];
        for (float& v : p) v = (float)((s = s * 1664525u + 1013904223u) >> 24);
        if (rep < 16)
            for (int k = 0; k < 4; ++k) p[k] = (rep >> k) & 1 ? 255.0f : 0.0f;
        for (int i = 0; i < nw; ++i)
            for (int j = 0; j < nw; ++j) {
                bad += (uint32_t)rs::color_blend16(p[0], p[1], p[2], p[3], w[i], w[j]) != (uint32_t)rs::color_blend(p[0], p[1], p[2], p[3], w[i], w[j]);
                ++n;
            }
    }
    printf("blend8 %ld %ld\n", n, bad);
    // 2: the result lies within the range of the four taps: all 0, all max and mixed extremes, then random taps, at 1023 and 65535
    n = bad = 0;
    for (uint32_t top : {1023u, 65535u}) {
        for (int rep = 0; rep < 4000; ++rep) {
            uint32_t p[4];
            for (uint32_t& v : p) v = ((s = s * 1664525u + 1013904223u) >> 8) % (top + 1);
            if (rep < 16)
                for (int k = 0; k < 4; ++k) p[k] = (rep >> k) & 1 ? top : 0u;
            else if (rep < 48)
                for (int k = 0; k < 4; ++k) p[k] = (rep >> k) & 1 ? top - (rep >= 32) : (uint32_t)(rep >= 32);
            uint32_t lo = p[0], hi = p[0];
            for (uint32_t v : p) {
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            for (int i = 0; i < nw; ++i)
                for (int j = 0; j < nw; ++j) {
                    const uint32_t got = rs::color_blend16((float)p[0], (float)p[1], (float)p[2], (float)p[3], w[i], w[j]);
                    bad += got < lo || got > hi;
                    ++n;
                }
        }
    }
    printf("range %ld %ld\n", n, bad);
    // 3: P010's container
    n = bad = 0;
    for (uint32_t word = 0; word < 65536u; ++word) {
        bad += rs::color_p010_unpack(word) != (word >> 6);
        bad += word < 1024u && (rs::color_p010_pack(word) != (word << 6) || rs::color_p010_unpack(rs::color_p010_pack(word)) != word);
        ++n;
    }
    printf("p010 %ld %ld\n", n, bad);
    return 0;
}
