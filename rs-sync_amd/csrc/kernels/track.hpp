// track.hpp -- sparse pyramidal Lucas-Kanade on grayscale frames: the reference driver's optical-flow step
// (core_testcode.cpp:97-133) at its grid points, ahead of rship_pack (set_track_pixels).
// Part of the single HIP translation unit rssync_kernels.hip (included there, in order).
//
//   pyr_down_kernel  one launch per pyramid level for all frames of a chunk: separable binomial [1 4 6 4 1] / 16,
//                    even pixels kept, reflect-101 border.  A workgroup loads its (2 TW + 4) x (2 TH + 4) input block
//                    into LDS once, runs the horizontal pass into a second LDS tile, then the vertical pass.  The taps
//                    are summed in ONE fixed order with contraction off, so that a float32 restatement (numpy:
//                    tests/track_reference.py) is bit-exact; level 1 is exact in any order (integer sums of bytes).
//   lk_kernel        one wave64 per (frame pair, grid point), every pair and point of a chunk in one launch, the level
//                    loop inside the kernel.  Inverse-compositional translational LK: the template (window of frame k
//                    around the point) and its central-difference gradients stay in registers -- 441 samples of a
//                    21 x 21 window are 7 per lane -- and so does the 2 x 2 structure tensor; one iteration samples
//                    frame k+1 bilinearly at the current position and reduces the two right-hand-side sums across the
//                    wave with a shuffle butterfly, which leaves the identical sum in every lane: every lane solves the
//                    2 x 2 system itself and the wave takes the same branch without a trip through LDS.  The body is
//                    lk_point, which kernels/features.hpp's lkfb_kernel calls too.
//
// Pixel arithmetic is relative to the integer base of the point (floor of the point at that level): positions are
// int base + fp32 offset, so fp32 keeps sub-pixel resolution at x ~ 4000.  The kernel returns the FLOW; the host adds it
// to the (integer) grid point in fp64.
#pragma once

namespace {

constexpr int kTrackMaxLevels = 8;
constexpr int kTrackMaxWin = 21;             // window side; 21 x 21 = 441 samples <= 7 per lane
constexpr int kTrackPerLane = (kTrackMaxWin * kTrackMaxWin + 63) / 64;
constexpr int kPyrTW = 32, kPyrTH = 8;       // output tile of pyr_down_kernel (256 threads)

struct TrackLevels {
    uint32_t w[kTrackMaxLevels], h[kTrackMaxLevels];
    uint64_t off[kTrackMaxLevels]; // level l >= 1: first float of the level in a frame's pyramid block (off[1] = 0)
};

struct TrackArgs {
    const uint8_t* u8;      // level 0 of the chunk's frames, packed (pitch = width)
    const float* pyr;       // levels 1 .. levels-1 of the chunk's frames
    uint64_t u8_stride, pyr_stride; // bytes / floats per frame
    uint32_t levels, n_pairs, n_points, ny, step, win, max_iters;
    float eps2, min_eig;    // squared convergence step (px^2); smallest eigenvalue / window area (intensity^2 / px^2)
    float2* flow;           // [n_pairs * n_points] flow at level 0
    uint8_t* status;
    float* resid;           // mean |I_b - T| over the window at the final position, level 0
    TrackLevels L;
};

__device__ __forceinline__ int reflect101(int x, int n) {
    if (x < 0) x = -x;
    if (x >= n) x = 2 * (n - 1) - x;
    return min(max(x, 0), n - 1); // (only reached by the lanes of a partial tile, whose outputs are not stored)
}

// the binomial taps a, b, c, d, e = x-2 .. x+2, in the one order the numpy restatement uses
__device__ __forceinline__ float tap5(float a, float b, float c, float d, float e) {
#pragma clang fp contract(off)
    return ((a + e) + (b + d) * 4.0f) + c * 6.0f;
}

// level `l` = downsample(level l-1): src is level l-1 (bytes when U8, else floats) of frame blockIdx.z
template <bool U8>
__global__ __launch_bounds__(256) void pyr_down_kernel(const void* __restrict__ src, uint64_t s_stride, int sw, int sh,
                                                       float* __restrict__ dst, uint64_t d_stride, int dw, int dh) {
#pragma clang fp contract(off)
    constexpr int TWI = 2 * kPyrTW + 4, THI = 2 * kPyrTH + 4;
    __shared__ float tile[THI][TWI + 1];
    __shared__ float hs[THI][kPyrTW + 1];
    const uint64_t f = blockIdx.z;
    const int ox0 = blockIdx.x * kPyrTW, oy0 = blockIdx.y * kPyrTH;
    const int ix0 = 2 * ox0 - 2, iy0 = 2 * oy0 - 2;
    for (int i = threadIdx.x; i < TWI * THI; i += 256) {
        const int ty = i / TWI, tx = i - ty * TWI;
        const size_t at = (size_t)reflect101(iy0 + ty, sh) * sw + reflect101(ix0 + tx, sw);
        tile[ty][tx] = U8 ? (float)((const uint8_t*)src)[f * s_stride + at] : ((const float*)src)[f * s_stride + at];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < THI * kPyrTW; i += 256) {
        const int ty = i / kPyrTW, tx = i - ty * kPyrTW;
        const float* p = &tile[ty][2 * tx];
        hs[ty][tx] = tap5(p[0], p[1], p[2], p[3], p[4]);
    }
    __syncthreads();
    const int tx = threadIdx.x % kPyrTW, ty = threadIdx.x / kPyrTW;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox < dw && oy < dh) {
        const float v = tap5(hs[2 * ty][tx], hs[2 * ty + 1][tx], hs[2 * ty + 2][tx], hs[2 * ty + 3][tx], hs[2 * ty + 4][tx]);
        dst[f * d_stride + (size_t)oy * dw + ox] = v * (1.0f / 256.0f); // (exact: a power of two)
    }
}

__device__ __forceinline__ float wave_allsum(float v) {
    // xor butterfly: lane i and lane i^m add the same two numbers, so every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// bilinear sample of frame `f` (of the chunk) at level l, position (ix + fx, iy + fy), fx, fy in [0, 1); coordinates
// clamped to the border
__device__ __forceinline__ float track_sample(const TrackArgs& A, uint32_t f, int l, int ix, int iy, float fx, float fy) {
    const int w = (int)A.L.w[l], h = (int)A.L.h[l];
    const int x0 = min(max(ix, 0), w - 1), x1 = min(max(ix + 1, 0), w - 1);
    const int y0 = min(max(iy, 0), h - 1), y1 = min(max(iy + 1, 0), h - 1);
    float p00, p01, p10, p11;
    if (l == 0) {
        const uint8_t* b = A.u8 + f * A.u8_stride;
        p00 = b[(size_t)y0 * w + x0]; p01 = b[(size_t)y0 * w + x1];
        p10 = b[(size_t)y1 * w + x0]; p11 = b[(size_t)y1 * w + x1];
    } else {
        const float* b = A.pyr + f * A.pyr_stride + A.L.off[l];
        p00 = b[(size_t)y0 * w + x0]; p01 = b[(size_t)y0 * w + x1];
        p10 = b[(size_t)y1 * w + x0]; p11 = b[(size_t)y1 * w + x1];
    }
    const float top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
    return top + fy * (bot - top);
}

// status codes (include/rssync_track.h)
constexpr uint8_t kTrackOk = 0, kTrackIllConditioned = 1, kTrackLeftImage = 2, kTrackIterCap = 3;

// LK of one point from frame fa (the template) to frame fb of the chunk, started at the level-0 position (ax + fx0,
// ay + fy0): an integer base plus a fraction in [0, 1).  FRAC = false is the integer start (fx0 = fy0 = 0 and never
// read), the grid point of lk_kernel; FRAC = true carries the fraction into every level, the template included, so a
// fraction of 0 gives the integer path's numbers.  RESID: also the mean |I_b - T| at the final position.  Returns the
// flow (relative to the start) at level 0.
struct LkOut {
    float flx, fly, res;
    uint8_t st;
};

template <bool FRAC, bool RESID>
__device__ __forceinline__ LkOut lk_point(const TrackArgs& A, uint32_t fa, uint32_t fb, int ax, int ay, float fx0, float fy0) {
    const int lane = threadIdx.x & 63;
    const int win = (int)A.win, r = win / 2, area = win * win;
    int dx[kTrackPerLane], dy[kTrackPerLane];
#pragma unroll
    for (int j = 0; j < kTrackPerLane; ++j) {
        const int s = lane + 64 * j;
        dy[j] = s < area ? s / win - r : 0;
        dx[j] = s < area ? s % win - r : 0;
    }
    auto valid = [&](int j) { return lane + 64 * j < area; };
    float T[kTrackPerLane], GX[kTrackPerLane], GY[kTrackPerLane];
    float flx = 0.f, fly = 0.f;
    uint8_t st = kTrackOk;
    for (int l = (int)A.levels - 1; l >= 0; --l) {
        if (l != (int)A.levels - 1) { flx *= 2.f; fly *= 2.f; }
        const int bx = ax >> l, by = ay >> l;                 // integer base of the point at this level
        const float sc = 1.0f / (float)(1 << l);
        // its fraction (exact for an integer start)
        const float fax = FRAC ? ((float)(ax - (bx << l)) + fx0) * sc : (float)(ax - (bx << l)) * sc;
        const float fay = FRAC ? ((float)(ay - (by << l)) + fy0) * sc : (float)(ay - (by << l)) * sc;
        const int w = (int)A.L.w[l], h = (int)A.L.h[l];
        float hxx = 0.f, hxy = 0.f, hyy = 0.f;
#pragma unroll
        for (int j = 0; j < kTrackPerLane; ++j) {
            T[j] = GX[j] = GY[j] = 0.f;
            if (!valid(j)) continue;
            const int x = bx + dx[j], y = by + dy[j];
            T[j] = track_sample(A, fa, l, x, y, fax, fay);
            GX[j] = 0.5f * (track_sample(A, fa, l, x + 1, y, fax, fay) - track_sample(A, fa, l, x - 1, y, fax, fay));
            GY[j] = 0.5f * (track_sample(A, fa, l, x, y + 1, fax, fay) - track_sample(A, fa, l, x, y - 1, fax, fay));
            hxx += GX[j] * GX[j];
            hxy += GX[j] * GY[j];
            hyy += GY[j] * GY[j];
        }
        hxx = wave_allsum(hxx);
        hxy = wave_allsum(hxy);
        hyy = wave_allsum(hyy);
        const float det = hxx * hyy - hxy * hxy;
        const float dd = hxx - hyy;
        const float min_eig = 0.5f * (hxx + hyy - sqrtf(dd * dd + 4.f * hxy * hxy)) / (float)area;
        if (!(min_eig >= A.min_eig) || !(det > 0.f)) { // a coarser level is skipped (the flow carries over), level 0 is a status
            if (l == 0) st = kTrackIllConditioned;
            continue;
        }
        const float idet = 1.0f / det;
        bool conv = false;
        for (uint32_t it = 0; it < A.max_iters; ++it) {
            const float px = fax + flx, py = fay + fly;       // position relative to the base
            if (px < (float)-bx || px > (float)(w - 1 - bx) || py < (float)-by || py > (float)(h - 1 - by)) {
                st = kTrackLeftImage;
                break;
            }
            const float ipx = floorf(px), ipy = floorf(py);
            const int ix = bx + (int)ipx, iy = by + (int)ipy;
            const float fx = px - ipx, fy = py - ipy;
            float ex = 0.f, ey = 0.f;
#pragma unroll
            for (int j = 0; j < kTrackPerLane; ++j) {
                if (!valid(j)) continue;
                const float e = track_sample(A, fb, l, ix + dx[j], iy + dy[j], fx, fy) - T[j];
                ex += GX[j] * e;
                ey += GY[j] * e;
            }
            ex = wave_allsum(ex);
            ey = wave_allsum(ey);
            const float ux = (hyy * ex - hxy * ey) * idet, uy = (hxx * ey - hxy * ex) * idet;
            flx -= ux; // inverse compositional: the increment is applied inverted
            fly -= uy;
            if (ux * ux + uy * uy < A.eps2) { conv = true; break; }
        }
        if (st == kTrackLeftImage) { flx *= (float)(1 << l); fly *= (float)(1 << l); break; } // (flow at level 0's scale)
        if (!conv && l == 0) st = kTrackIterCap;
    }
    const int W = (int)A.L.w[0], H = (int)A.L.h[0];
    const float ox = FRAC ? fx0 + flx : flx, oy = FRAC ? fy0 + fly : fly; // final position relative to (ax, ay)
    if (st != kTrackLeftImage && (ox < (float)-ax || ox > (float)(W - 1 - ax) || oy < (float)-ay || oy > (float)(H - 1 - ay)))
        st = kTrackLeftImage;
    float res = 0.f;
    if (RESID) {
        // mean absolute residual at the final position, level 0 (template = frame fa's pixels around the start point)
        const float cx = fminf(fmaxf(ox, (float)(-ax - 1)), (float)(W - ax)), cy = fminf(fmaxf(oy, (float)(-ay - 1)), (float)(H - ay));
        const float ipx = floorf(cx), ipy = floorf(cy);
        const int ix = ax + (int)ipx, iy = ay + (int)ipy;
        const float fx = cx - ipx, fy = cy - ipy;
#pragma unroll
        for (int j = 0; j < kTrackPerLane; ++j) {
            if (!valid(j)) continue;
            res += fabsf(track_sample(A, fb, 0, ix + dx[j], iy + dy[j], fx, fy) -
                         track_sample(A, fa, 0, ax + dx[j], ay + dy[j], FRAC ? fx0 : 0.f, FRAC ? fy0 : 0.f));
        }
        res = wave_allsum(res) / (float)area;
    }
    return LkOut{flx, fly, res, st};
}

__global__ __launch_bounds__(256) void lk_kernel(TrackArgs A) {
    const uint32_t g = blockIdx.x * 4 + threadIdx.x / 64; // one wave per (pair, point)
    const int lane = threadIdx.x & 63;
    if (g >= A.n_pairs * A.n_points) return;
    const uint32_t pair = g / A.n_points, pt = g - pair * A.n_points;
    // the driver's grid (core_testcode.cpp:124-132): x-major, i = step, 2 step, ... < width
    const int ax = (int)((pt / A.ny + 1) * A.step), ay = (int)((pt % A.ny + 1) * A.step);
    const LkOut o = lk_point<false, true>(A, pair, pair + 1, ax, ay, 0.f, 0.f);
    if (lane == 0) {
        A.flow[g] = make_float2(o.flx, o.fly);
        A.status[g] = o.st;
        A.resid[g] = o.res;
    }
}

} // namespace
