// resample_math_check.cpp -- csrc/resample_math.hpp compiled for the CPU (tests/test_resample_cpu.py): the bicubic sampler
// on every position of a sweep over a 9 x 7 plane of 8-bit, 10-bit (as words and in P010's container) and 16-bit values,
// printed for the byte-for-byte comparison with the numpy restatement (tests/resample_reference.py).  No arguments.
//   plane <tag> <63 stored words>            the plane, row by row
//   s <tag> <x> <y> <stored word>            one line per position (hex floats)
//   weights <t> <w0> <w1> <w2> <w3>          the weights at a few t
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rs-sync_amd/csrc/resample_math.hpp"

namespace {

constexpr int W = 9, H = 7;

// every quarter position, every integer among them, the four edges exactly, and positions within 1e-3 of the edges
std::vector<float> axis(int n) {
    std::vector<float> v;
    for (int k = 0; k <= 4 * (n - 1); ++k) v.push_back((float)k * 0.25f);
    const float last = (float)(n - 1);
    for (float e : {1e-3f, 4e-4f, 1e-6f}) {
        v.push_back(e);
        v.push_back(last - e);
    }
    v.push_back(1.0f - 1e-3f);
    v.push_back(last - 1.0f + 1e-3f);
    v.push_back(2.37f);
    return v;
}

template <int SHIFT>
int sweep16(const char* tag, uint32_t seed, uint32_t top, float vmax) {
    const size_t pitch = 2 * W + 6; // bytes
    std::vector<uint8_t> img(pitch * H);
    uint32_t s = seed;
    printf("plane %s", tag);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            s = s * 1664525u + 1013904223u;
            // P010 carries junk in its low six bits, which the sampler must ignore
            const uint32_t value = y < 3 ? (x < 4 ? 0u : top) : (s >> 8) % (top + 1); // rows 0 .. 2: a step edge, for both clamps
            const uint16_t word = (uint16_t)((value << SHIFT) | (SHIFT ? (s >> 26) : 0u));
            __builtin_memcpy(&img[y * pitch + 2 * x], &word, 2);
            printf(" %u", (unsigned)word);
        }
    printf("\n");
    for (float y : axis(H))
        for (float x : axis(W)) {
            if (!rs::rect_inside(x, y, W, H)) return 3;
            const uint32_t got = rs::cubic_sample16<SHIFT>(img.data(), pitch, rs::cubic_taps(W, H, x, y), vmax);
            printf("s %s %a %a %u\n", tag, x, y, got);
        }
    return 0;
}

} // namespace

int main() {
    const size_t pitch = 11;
    std::vector<uint8_t> img(pitch * H);
    uint32_t s = 12345;
    printf("plane u8");
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            s = s * 1664525u + 1013904223u;
            img[y * pitch + x] = y < 3 ? (x < 4 ? 0 : 255) : (uint8_t)(s >> 24); // rows 0 .. 2: a step edge, for both clamps
            printf(" %u", (unsigned)img[y * pitch + x]);
        }
    printf("\n");
    for (float y : axis(H))
        for (float x : axis(W)) {
            if (!rs::rect_inside(x, y, W, H)) return 3;
            printf("s u8 %a %a %u\n", x, y, (unsigned)rs::cubic_sample(img.data(), pitch, W, H, x, y));
        }
    if (int r = sweep16<0>("i010", 777u, 1023u, 1023.0f)) return r;
    if (int r = sweep16<6>("p010", 4242u, 1023u, 1023.0f)) return r;
    if (int r = sweep16<0>("u16", 99u, 65535u, 65535.0f)) return r;
    for (float t : {0.0f, 1.0f, 0.5f, 0.25f, 1e-3f, 0.999f, 0.3333333f}) {
        float w[4];
        rs::cubic_weights(t, w);
        printf("weights %a %a %a %a %a\n", t, w[0], w[1], w[2], w[3]);
    }
    return 0;
}
