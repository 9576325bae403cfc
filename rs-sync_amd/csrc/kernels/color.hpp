// color.hpp -- colour frames stabilised in one pass per frame (include/rssync_color.h): NV12, I420 and RGBA32.  Part of
// the single HIP translation unit rssync_kernels.hip, after kernels/stabilize.hpp, whose map it evaluates per plane with
// that plane's camera, and after kernels/colorsample.hpp, whose samplers read the taps; the arithmetic is color_math.hpp's.
// GRAY8 runs stabilize_kernel itself.  This file holds the two 8-bit thread shapes of every colour family, each once:
//
//   yuv8<NV12, F>(A, pos)    one thread per chroma sample of the output.  It finds the chroma position once and samples U
//                            and V there -- NV12: the result one 16-bit store of the interleaved pair; I420: two planes --,
//                            then renders the 2 x 2 luma pixels the sample covers, two adjacent bytes of a row as one 16-bit
//                            store.  A wave covers 128 x 2 luma pixels.
//   rgba8<F>(A, pos)         one thread per output pixel: one position, the four channels of the result one 32-bit store.
//
// F is the sampler (0 bilinear, 1 bicubic).  `pos` is the family: a position policy with two members, luma(f, u, v, &x, &y)
// and chroma(f, u, v, &x, &y), that find the source position of output sample (u, v) of chunk frame f in that plane and
// answer whether it is inside the plane.  A body knows nothing else of its family.  (The infill's kernels, which sample another
// frame's plane where the own one has nothing, have bodies of their own in kernels/colorinfill.hpp on the same samplers
// and counters.)
//
//   ColorPos<C>              the constant camera: color_map<C> on A.luma / A.chroma
//   color_rows_kernel        the luma and the chroma row table of every frame of a chunk in one launch: entries
//                            0 .. rows of the luma table, then 0 .. rows_c of the chroma table (stab_row_matrix with the
//                            chroma plane's rows and frame time, against the frame's one target): color_rows_entry
//   color_yuv_kernel<C, NV>  yuv8<NV, 0> with ColorPos<C>
//   color_rgba_kernel<C>     rgba8<0> with ColorPos<C>
//
// A sample whose position is outside is the fill.  Such samples are counted as the stabiliser counts them, and for the
// infill the samples that came from another frame beside them: ballots of a wave, one atomic per counter and wave that has
// any (color_count4, color_count1).  The bodies here never borrow and say so with constants, so those ballots fold away.
// The 4:2:0 bodies set their flags without a branch; only the sampler stands under the inside test.
#pragma once

namespace {

struct ColorRowsArgs {
    const double* table;
    const double* times;    // luma frame times of the chunk's frames
    const double* times_c;  // chroma frame times
    const double* targets;  // [n_frames][4] unit quaternions: one per frame for all planes
    float* rows_tab;        // [n_frames][rows + 1][9]
    float* rows_tab_c;      // [n_frames][rows_c + 1][9]
    double start, fs, ro, delay;
    uint32_t n_knots, rows, rows_c, n_frames; // rows_c == 0: no chroma plane
};

// Entry j of a launch's row -- 0 .. rows the luma table's, then 0 .. rows_c the chroma table's -- for a (time, target) pair:
// the plane's time of frame g against the target of frame f, written to table `slot` of the plane's region.
template <class ROWS_ARGS>
__device__ __forceinline__ void color_rows_entry(const ROWS_ARGS& A, uint32_t j, size_t g, size_t f, size_t slot) {
    const bool chroma = j > A.rows;
    if (chroma) {
        j -= A.rows + 1;
        if (!A.rows_c || j > A.rows_c) return;
    }
    const uint32_t rows = chroma ? A.rows_c : A.rows;
    const double time = chroma ? A.times_c[g] : A.times[g];
    const double* t = A.targets + f * 4;
    float m[9];
    rs::stab_row_matrix(A.table, (int)A.n_knots, A.start, A.fs, A.ro, time, (double)rows, A.delay, rs::RectQuat{t[0], t[1], t[2], t[3]},
                        (double)j, m);
    float* out = (chroma ? A.rows_tab_c : A.rows_tab) + (slot * (rows + 1) + j) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = m[k];
}

__global__ __launch_bounds__(256) void color_rows_kernel(ColorRowsArgs A) {
    const size_t f = blockIdx.y;
    color_rows_entry(A, blockIdx.x * 256 + threadIdx.x, f, f, f);
}

// one camera of a colour call: the plane's output camera and input lens
struct ColorCam {
    const float4* rays;     // LENS: the ray map of the plane's output camera, [out rows][out cols]
    const float* rows_tab;  // the chunk's tables of the plane, rows + 1 entries per frame
    rs::RectLensF lens;     // the plane's input lens
    rs::StabCamF cam;       // PINHOLE: the plane's output camera
    float y_scale;          // (float)rows / (float)out rows of the plane
};

struct ColorArgs {
    ColorCam luma, chroma;       // (RGBA32: luma alone)
    const uint8_t* src[3];       // frame 0 of the chunk, per plane
    uint8_t* dst[3];
    uint64_t src_pitch[3], src_stride[3], dst_pitch[3], dst_stride[3];
    unsigned long long* outside;   // per frame of the chunk: filled pixels of plane 0
    unsigned long long* outside_c; // ... and filled chroma samples
    uint32_t width, height, out_width, out_height; // of plane 0
    int32_t iterations;
    uint32_t fill;               // the fill values as bytes: Y, U, V or R, G, B, A from the lowest
};

// plane k of frame f of the chunk
__device__ __forceinline__ const uint8_t* color_plane(const ColorArgs& A, int k, uint32_t f) {
    return A.src[k] + (size_t)f * A.src_stride[k];
}

// the source position of output pixel (u, v) of frame f in a plane of `rows` rows
template <int CAMERA>
__device__ inline void color_map(const ColorCam& C, uint32_t f, uint32_t rows, uint32_t out_cols, int iterations, uint32_t u, uint32_t v,
                                 float* x, float* y) {
    float rx, ry, rz;
    if (CAMERA == 0) {
        const float4 r = C.rays[(size_t)v * out_cols + u];
        rx = r.x; ry = r.y; rz = r.z;
    } else {
        rs::stab_pinhole_ray(C.cam, (float)u, (float)v, &rx, &ry, &rz);
    }
    rs::rect_map_pixel(C.rows_tab + (size_t)f * (rows + 1) * 9, (int)rows, C.lens, iterations, rs::stab_start_row((float)v, C.y_scale), rx, ry,
                       rz, x, y);
}

// the constant camera
template <int CAMERA>
struct ColorPos {
    const ColorArgs& A;
    __device__ __forceinline__ bool luma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        color_map<CAMERA>(A.luma, f, A.height, A.out_width, A.iterations, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)A.width, (int)A.height);
    }
    __device__ __forceinline__ bool chroma(uint32_t f, uint32_t u, uint32_t v, float* x, float* y) const {
        color_map<CAMERA>(A.chroma, f, A.height >> 1, A.out_width >> 1, A.iterations, u, v, x, y);
        return rs::rect_inside(*x, *y, (int)(A.width >> 1), (int)(A.height >> 1));
    }
};

// the four counters of a 4:2:0 kernel: bit 0 .. 3 of miss_y / lent_y are the thread's 2 x 2 luma pixels
__device__ __forceinline__ void color_count4(const ColorArgs& A, unsigned long long* borrowed, unsigned long long* borrowed_c, uint32_t f,
                                             bool miss_c, bool lent_c, uint32_t miss_y, uint32_t lent_y) {
    const unsigned long long mc = __ballot(miss_c), bc = __ballot(lent_c);
    uint32_t ny = 0, by = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ny += (uint32_t)__popcll(__ballot((miss_y >> k) & 1u));
        by += (uint32_t)__popcll(__ballot((lent_y >> k) & 1u));
    }
    if ((threadIdx.x & 63) == 0) {
        if (ny) atomicAdd(A.outside + f, (unsigned long long)ny);
        if (mc) atomicAdd(A.outside_c + f, (unsigned long long)__popcll(mc));
        if (by) atomicAdd(borrowed + f, (unsigned long long)by);
        if (bc) atomicAdd(borrowed_c + f, (unsigned long long)__popcll(bc));
    }
}

// the two counters of a kernel of one sample per thread
__device__ __forceinline__ void color_count1(const ColorArgs& A, unsigned long long* borrowed, uint32_t f, bool filled, bool lent) {
    const unsigned long long m = __ballot(filled), b = __ballot(lent);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(A.outside + f, (unsigned long long)__popcll(m));
        if (b) atomicAdd(borrowed + f, (unsigned long long)__popcll(b));
    }
}

template <bool NV12, int FILTER, class POS>
__device__ __forceinline__ void yuv8(const ColorArgs& A, const POS& pos) {
    const uint32_t cu = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t cv = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    const uint32_t cw = A.width >> 1, ch = A.height >> 1, ocw = A.out_width >> 1, och = A.out_height >> 1;
    bool miss_c = false;
    uint32_t miss_y = 0;
    if (cu < ocw && cv < och) {
        // the chroma sample: one position for U and V
        float x, y;
        bool in = pos.chroma(f, cu, cv, &x, &y);
        uint32_t cb = (A.fill >> 8) & 255u, cr = (A.fill >> 16) & 255u;
        if (in)
            sample_uv8<NV12, FILTER>(color_plane(A, 1, f), A.src_pitch[1], NV12 ? nullptr : color_plane(A, 2, f), A.src_pitch[2], (int)cw,
                                     (int)ch, x, y, &cb, &cr);
        miss_c = !in;
        if (NV12) {
            color_store16(A.dst[1] + (size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + 2 * (size_t)cu, cb | (cr << 8));
        } else {
            A.dst[1][(size_t)f * A.dst_stride[1] + (size_t)cv * A.dst_pitch[1] + cu] = (uint8_t)cb;
            A.dst[2][(size_t)f * A.dst_stride[2] + (size_t)cv * A.dst_pitch[2] + cu] = (uint8_t)cr;
        }
        // the 2 x 2 luma pixels under it
        uint8_t* dst = A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)(2 * cv) * A.dst_pitch[0] + 2 * (size_t)cu;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            uint32_t pair = 0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                in = pos.luma(f, 2 * cu + dx, 2 * cv + dy, &x, &y);
                uint32_t val = A.fill & 255u;
                if (in) val = sample_luma8<FILTER>(color_plane(A, 0, f), A.src_pitch[0], (int)A.width, (int)A.height, x, y);
                miss_y |= (uint32_t)!in << (2 * dy + dx);
                pair |= val << (8 * dx);
            }
            color_store16(dst + (size_t)dy * A.dst_pitch[0], pair);
        }
    }
    color_count4(A, nullptr, nullptr, f, miss_c, false, miss_y, 0);
}

template <int FILTER, class POS>
__device__ __forceinline__ void rgba8(const ColorArgs& A, const POS& pos) {
    const uint32_t u = blockIdx.x * kRectTW + (threadIdx.x & (kRectTW - 1));
    const uint32_t v = blockIdx.y * kRectTH + threadIdx.x / kRectTW;
    const uint32_t f = blockIdx.z;
    bool filled = false;
    if (u < A.out_width && v < A.out_height) {
        float x, y;
        uint32_t px = A.fill;
        if (pos.luma(f, u, v, &x, &y))
            px = sample_rgba8<FILTER>(color_plane(A, 0, f), A.src_pitch[0], (int)A.width, (int)A.height, x, y);
        else
            filled = true;
        color_store32(A.dst[0] + (size_t)f * A.dst_stride[0] + (size_t)v * A.dst_pitch[0] + 4 * (size_t)u, px);
    }
    color_count1(A, nullptr, f, filled, false);
}

template <int CAMERA, bool NV12>
__global__ __launch_bounds__(256) void color_yuv_kernel(ColorArgs A) {
    yuv8<NV12, 0>(A, ColorPos<CAMERA>{A});
}

template <int CAMERA>
__global__ __launch_bounds__(256) void color_rgba_kernel(ColorArgs A) {
    rgba8<0>(A, ColorPos<CAMERA>{A});
}

} // namespace
