// yuv_math_check.cpp -- the 4:2:2 functions of csrc/color_math.hpp compiled for the CPU (tests/test_yuv_cpu.py): the chroma
// offset, camera and frame time as hex floats for the comparison with the numpy restatement, and the 4:2:0 functions'
// results beside them (they must not have moved).  Arguments: site fx fy cx cy frame_time.
#include <cstdio>
#include <cstdlib>

#include "../../rs-sync_amd/csrc/color_math.hpp"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int site = atoi(argv[1]);
    const double cam[4] = {strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr)};
    const double frame_time = strtod(argv[6], nullptr);
    double ox, out[4];
    rs::color_chroma422_offset(site, &ox);
    rs::color_chroma422_camera(cam, ox, out);
    printf("offset %a\n", ox);
    printf("camera %a %a %a %a\n", out[0], out[1], out[2], out[3]);
    printf("time %a\n", rs::color_chroma422_time(frame_time));
    double ox0, oy0, out0[4];
    rs::color_chroma_offset(site, &ox0, &oy0);
    rs::color_chroma_camera(cam, ox0, oy0, out0);
    printf("camera420 %a %a %a %a\n", out0[0], out0[1], out0[2], out0[3]);
    return 0;
}
