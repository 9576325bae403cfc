// features.hpp -- corner detection and forward-backward tracking of the detected corners (include/rssync_features.h),
// on top of the tracker's pyramid and LK (kernels/track.hpp).  Part of the single HIP translation unit
// rssync_kernels.hip (included there after track.hpp).
//
//   corner_cell_kernel    one workgroup per (frame, cell).  The cell's bytes plus a halo of b + 1 px (b = block / 2 + 1)
//                         are staged in LDS once.  Harris responses R are exact integers (int64), computed over the
//                         cell plus a 1-px halo in row bands: each thread owns one column of its band, keeps the
//                         block x block structure-tensor sums as a vertical sliding window (the sums of the entering
//                         row added, of the leaving row subtracted -- exact in any order), and writes one R per row into
//                         a 4-row ring in LDS, from which the non-maximum suppression of the row before reads its
//                         neighbours.  Out: the cell's largest R and its best local maximum (R, raster index).
//   corner_select_kernel  one workgroup per frame: R_max = the largest cell maximum, T = max(1, ceil(quality R_max)) in
//                         fp64, and the cell winners with R >= T compacted into the frame's list in cell order by a
//                         block prefix sum (no atomics: the list is deterministic).
//   lkfb_kernel<FB>       one wave64 per (pair, slot of the pair's list); waves past the pair's count return at once.
//                         FB: LK forward from frame k to k+1 at the listed point, then backward from k+1 to k started at
//                         b = a + flow (an integer base plus an fp32 fraction), fb_error = |flow_fwd + flow_bwd|.
//                         !FB: forward only, with the residual -- lk_kernel at caller-given points (a test path).
//
// The detector is defined so that a numpy restatement (tests/feature_reference.py) agrees bit for bit: integer
// gradients (twice the central difference), int32 tensor sums, R = 64 (A C - B^2) - 3 (A + C)^2 in int64.
#pragma once

namespace {

constexpr int kCornerMaxCell = 128, kCornerMaxBlock = 9;
constexpr int kCornerThreads = 256;
constexpr int64_t kNoResponse = INT64_MIN; // an invalid pixel: every valid R beats it

struct CornerArgs {
    const uint8_t* u8;     // level 0 of the chunk's frames, packed (pitch = width)
    uint64_t u8_stride;
    int W, H, cell, r;     // r = block / 2
    int ncy, ncells;       // cells per column, cells per frame (numbered x-major: cell = cx * ncy + cy)
    int64_t* cell_max;     // [frame][cell] largest R over the cell's valid pixels (kNoResponse: none)
    int64_t* best_r;       // [frame][cell] the cell's best local maximum
    int64_t* best_idx;     // its raster index y W + x, -1 = none
};

// p (R, index) beats q: a larger R, or an equal R and a smaller raster index
__device__ __forceinline__ bool corner_beats(int64_t rp, int64_t ip, int64_t rq, int64_t iq) {
    return rp > rq || (rp == rq && ip < iq);
}

// the tensor sums of one row of the block window: gradients of the pixels (yy, xx - r .. xx + r) of the tile
__device__ __forceinline__ void corner_row(const uint8_t* t, int tp, int yy, int xx, int r, int& a, int& b, int& c) {
    a = b = c = 0;
    for (int d = -r; d <= r; ++d) {
        const uint8_t* q = t + yy * tp + xx + d;
        const int gx = (int)q[1] - (int)q[-1], gy = (int)q[tp] - (int)q[-tp];
        a += gx * gx;
        b += gx * gy;
        c += gy * gy;
    }
}

__global__ __launch_bounds__(kCornerThreads) void corner_cell_kernel(CornerArgs A) {
    extern __shared__ uint8_t corner_tile[];                // (cell + 2 (r + 2))^2 bytes
    __shared__ int64_t ring[4][kCornerThreads];             // R of the last four rows, per thread column
    __shared__ int64_t red_max[4], red_r[4], red_i[4];
    const int f = blockIdx.x / A.ncells, cell = blockIdx.x - f * A.ncells; // one workgroup per (frame, cell)
    const int cx = cell / A.ncy, cy = cell - cx * A.ncy;
    const int x0 = cx * A.cell, y0 = cy * A.cell;
    const int cw = min(A.cell, A.W - x0), ch = min(A.cell, A.H - y0);
    const int r = A.r, h = r + 2;                           // tile halo = b + 1
    const int tp = A.cell + 2 * h;                          // tile side (partial cells use the same layout)
    const int tx0 = x0 - h, ty0 = y0 - h;
    const uint8_t* img = A.u8 + (uint64_t)f * A.u8_stride;
    for (int i = threadIdx.x; i < tp * tp; i += kCornerThreads) {
        const int ty = i / tp, tx = i - ty * tp;
        const int gx = tx0 + tx, gy = ty0 + ty;
        corner_tile[i] = (gx >= 0 && gx < A.W && gy >= 0 && gy < A.H) ? img[(size_t)gy * A.W + gx] : (uint8_t)0;
    }
    // bands: nc = cw + 2 columns of R (x0 - 1 .. x0 + cw); each band covers rpb rows of the cell
    const int nc = cw + 2, nb = kCornerThreads / nc, rpb = (ch + nb - 1) / nb;
    const int t = threadIdx.x, band = t / nc, col = t - band * nc;
    const bool active = band < nb;
    const int x = x0 - 1 + col;                              // this thread's column
    const int ys = y0 + band * rpb, ye = min(ys + rpb, y0 + ch); // NMS rows [ys, ye): R rows ys - 1 .. ye
    const int b = r + 1;
    const bool xok = x >= b && x <= A.W - 1 - b;
    const int lx = x - tx0;                                  // tile column
    int sa = 0, sb = 0, sc = 0;
    int64_t cmax = kNoResponse, best = kNoResponse, besti = -1;
    __syncthreads();
    for (int s = 0; s < rpb + 2; ++s) {
        const int y = ys - 1 + s;                             // the R row of this step
        if (active && y <= ye) {
            const int ly = y - ty0;
            if (s == 0) {
                for (int d = -r; d <= r; ++d) {
                    int a1, b1, c1;
                    corner_row(corner_tile, tp, ly + d, lx, r, a1, b1, c1);
                    sa += a1; sb += b1; sc += c1;
                }
            } else {
                int a1, b1, c1, a0, b0, c0;
                corner_row(corner_tile, tp, ly + r, lx, r, a1, b1, c1);
                corner_row(corner_tile, tp, ly - r - 1, lx, r, a0, b0, c0);
                sa += a1 - a0; sb += b1 - b0; sc += c1 - c0;
            }
            int64_t R = kNoResponse;
            if (xok && y >= b && y <= A.H - 1 - b) {
                const int64_t A64 = sa, B64 = sb, C64 = sc;
                R = 64 * (A64 * C64 - B64 * B64) - 3 * (A64 + C64) * (A64 + C64);
            }
            ring[s & 3][t] = R;
        }
        __syncthreads();
        // NMS of row y - 1 (rows ys .. ye - 1), the cell's own columns only
        const int yn = y - 1;
        if (active && s >= 2 && yn < ye && col >= 1 && col <= cw) {
            const int64_t R = ring[(s - 1) & 3][t];
            if (R != kNoResponse) {
                cmax = max(cmax, R);
                const int64_t* up = ring[(s - 2) & 3];
                const int64_t* mid = ring[(s - 1) & 3];
                const int64_t* dn = ring[s & 3];
                // neighbours before p in raster order must be beaten strictly, those after it may tie
                const bool lm = R > up[t - 1] && R > up[t] && R > up[t + 1] && R > mid[t - 1] && R >= mid[t + 1] &&
                                R >= dn[t - 1] && R >= dn[t] && R >= dn[t + 1];
                const int64_t idx = (int64_t)yn * A.W + x;
                if (lm && corner_beats(R, idx, best, besti)) { best = R; besti = idx; }
            }
        }
    }
    // reductions: largest R, best (R, index) -- the wave by shuffles, the workgroup through LDS
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t om = __shfl_xor(cmax, m, 64), orr = __shfl_xor(best, m, 64), oi = __shfl_xor(besti, m, 64);
        cmax = max(cmax, om);
        if (oi >= 0 && (besti < 0 || corner_beats(orr, oi, best, besti))) { best = orr; besti = oi; }
    }
    const int wv = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) { red_max[wv] = cmax; red_r[wv] = best; red_i[wv] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kCornerThreads / 64; ++w) {
            cmax = max(cmax, red_max[w]);
            if (red_i[w] >= 0 && (besti < 0 || corner_beats(red_r[w], red_i[w], best, besti))) { best = red_r[w]; besti = red_i[w]; }
        }
        const size_t o = (size_t)f * A.ncells + cell;
        A.cell_max[o] = cmax;
        A.best_r[o] = best;
        A.best_idx[o] = besti;
    }
}

struct SelectArgs {
    const int64_t* cell_max;
    const int64_t* best_r;
    const int64_t* best_idx;
    int W, ncells;
    double quality;
    int2* pts;             // [pair][ncells] the frame's features (x, y) in cell order
    uint32_t* counts;      // [pair]
};

__global__ __launch_bounds__(kCornerThreads) void corner_select_kernel(SelectArgs A) {
    __shared__ int64_t red[4];
    __shared__ uint32_t wsum[4];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x / 64;
    const size_t o = (size_t)f * A.ncells;
    int64_t m = kNoResponse;
    for (int i = threadIdx.x; i < A.ncells; i += kCornerThreads) m = max(m, A.cell_max[o + i]);
    for (int k = 32; k >= 1; k >>= 1) m = max(m, (int64_t)__shfl_xor(m, k, 64));
    if (lane == 0) red[wv] = m;
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    // T = max(1, ceil(quality R_max)) in fp64: R_max < 2^53 converts exactly, the product is one rounding
    int64_t T = 1;
    if (m != kNoResponse) {
        const double q = __dmul_rn(A.quality, (double)m);
        T = max((int64_t)1, (int64_t)ceil(q));
    }
    uint32_t base = 0;
    for (int i0 = 0; i0 < A.ncells; i0 += kCornerThreads) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < A.ncells && A.best_idx[o + i] >= 0 && A.best_r[o + i] >= T;
        const uint64_t bal = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        __syncthreads(); // (wsum of the previous round has been read)
        if (lane == 0) wsum[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        if (keep) {
            const int64_t idx = A.best_idx[o + i];
            const int y = (int)(idx / A.W), x = (int)(idx - (int64_t)y * A.W);
            A.pts[o + off + before] = make_int2(x, y);
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
    if (threadIdx.x == 0) A.counts[f] = base;
}

struct LkfbArgs {
    TrackArgs T;           // pyramid, LK settings; T.flow / T.status / T.resid: the forward outputs [pair][slots]
    const int2* pts;       // [pair][slots] the start points a
    const uint32_t* counts;// [pair]
    uint32_t slots;
    float2* flow_b;        // FB: [pair][slots] backward flow
    float* fb;             // FB: [pair][slots] |flow_fwd + flow_bwd| (NaN when the forward status is not 0)
    float max_fb;
};

constexpr uint8_t kFeatureFbMismatch = 4; // include/rssync_features.h

template <bool FB>
__global__ __launch_bounds__(256) void lkfb_kernel(LkfbArgs A) {
    const uint32_t g = blockIdx.x * 4 + threadIdx.x / 64; // one wave per (pair, slot)
    const int lane = threadIdx.x & 63;
    if (g >= A.T.n_pairs * A.slots) return;
    const uint32_t pair = g / A.slots, slot = g - pair * A.slots;
    if (slot >= A.counts[pair]) return;
    const int2 a = A.pts[g];
    const LkOut o = lk_point<false, !FB>(A.T, pair, pair + 1, a.x, a.y, 0.f, 0.f);
    if (!FB) {
        if (lane == 0) {
            A.T.flow[g] = make_float2(o.flx, o.fly);
            A.T.status[g] = o.st;
            A.T.resid[g] = o.res;
        }
        return;
    }
    uint8_t st = o.st;
    float2 back = make_float2(0.f, 0.f);
    float fb = __builtin_nanf("");
    if (st == kTrackOk) {
        // b = a + flow as an integer base plus a fraction in [0, 1)
        const float ix = floorf(o.flx), iy = floorf(o.fly);
        int bx = a.x + (int)ix, by = a.y + (int)iy;
        float fx = o.flx - ix, fy = o.fly - iy;
        if (fx >= 1.f) { bx += 1; fx = 0.f; } // (a tiny negative flow: the difference rounded up to 1)
        if (fy >= 1.f) { by += 1; fy = 0.f; }
        const LkOut q = lk_point<true, false>(A.T, pair + 1, pair, bx, by, fx, fy);
        back = make_float2(q.flx, q.fly);
        const float ex = o.flx + q.flx, ey = o.fly + q.fly;
        fb = sqrtf(ex * ex + ey * ey);
        if (q.st != kTrackOk || !(fb <= A.max_fb)) st = kFeatureFbMismatch;
    }
    if (lane == 0) {
        A.T.flow[g] = make_float2(o.flx, o.fly);
        A.T.status[g] = st;
        A.flow_b[g] = back;
        A.fb[g] = fb;
    }
}

} // namespace
