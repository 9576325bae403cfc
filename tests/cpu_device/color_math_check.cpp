// color_math_check.cpp -- csrc/color_math.hpp compiled for the CPU (tests/test_color_cpu.py): the sampler taken apart
// against rect_sample on every position of a sweep, and the chroma camera and frame time as hex floats for the comparison
// with the numpy restatement.  Arguments: site ro fx fy cx cy height frame_time.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rs-sync_amd/csrc/color_math.hpp"

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const int site = atoi(argv[1]);
    const double ro = strtod(argv[2], nullptr), cam[4] = {strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr), strtod(argv[6], nullptr)};
    const double height = strtod(argv[7], nullptr), frame_time = strtod(argv[8], nullptr);
    double ox, oy, out[4];
    rs::color_chroma_offset(site, &ox, &oy);
    rs::color_chroma_camera(cam, ox, oy, out);
    printf("camera %a %a %a %a\n", out[0], out[1], out[2], out[3]);
    printf("time %a\n", rs::color_chroma_time(frame_time, ro, oy, height));
    printf("offset %a\n", rs::color_chroma_time(0.0, ro, oy, height));
    // a 13 x 9 image with a pitch of 17, positions over the whole inside range (the edges and the last row and column included)
    const int w = 13, h = 9, pitch = 17;
    std::vector<uint8_t> img((size_t)pitch * h);
    uint32_t s = 12345;
    for (uint8_t& b : img) b = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    long bad = 0, n = 0;
    for (int iy = 0; iy <= 8 * (h - 1); ++iy)
        for (int ix = 0; ix <= 8 * (w - 1); ++ix) {
            const float x = (float)ix * 0.125f + (ix % 3 == 1 && ix < 8 * (w - 1) ? 0.0371f : 0.0f);
            const float y = (float)iy * 0.125f + (iy % 5 == 2 && iy < 8 * (h - 1) ? 0.0113f : 0.0f);
            if (!rs::rect_inside(x, y, w, h)) return 3;
            const rs::ColorTaps t = rs::color_taps(w, h, x, y);
            const uint8_t* p = img.data() + (size_t)t.y0 * pitch + t.x0;
            const uint8_t got = rs::color_blend((float)p[0], (float)p[1], (float)p[pitch], (float)p[pitch + 1], t.fx, t.fy);
            bad += got != rs::rect_sample(img.data(), pitch, w, h, x, y);
            ++n;
        }
    printf("sampler %ld positions %ld differ\n", n, bad);
    return 0;
}
