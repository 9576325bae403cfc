"""Inputs of tests/test_gpu_feature_ties.py and of the tie tests in tests/test_features_cpu.py: frames on which the corner
detector's tie rule decides ("p beats q iff R(p) > R(q), or they are equal and p's raster index is smaller",
include/rssync_features.h), the case lists both files iterate over, and statistics that say from the numpy restatement
(tests/feature_reference.py) alone how many ties an input has and where in corner_cell_kernel's thread layout they fall.
numpy + feature_reference only."""
import numpy as np

import feature_reference as fr

THREADS = 256                    # kCornerThreads (csrc/kernels/features.hpp)

# --- a. ties in the suppression and in the cell winner: (h, w, P, seed).  The seed is h, but for 120 x 64: there the
# largest response of blocks 5 and 9 lies next to no mirror axis at seed 120, so quality 1.0 would leave no plateau
TIE_FRAMES = ((197, 331, 13, 197), (120, 64, 12, 121), (29, 37, 7, 29), (129, 257, 20, 129))
TIE_CONFIGS = ((16, 3, 1e-3), (64, 9, 0.01), (128, 5, 0.5), (16, 9, 1.0), (128, 5, 1.0), (64, 7, 0.01))   # cell, block, quality
PITCHED = TIE_FRAMES[0]          # the frame of the pitched view (pitch > width)
# --- c. full range: a 0/255 pattern
RANGE_FRAME = (130, 258, 9, 4)   # h, w, P, seed
RANGE_BLOCKS = (3, 5, 7, 9)
RANGE_QUALITIES = (1.0, 0.37, 1e-3, 1e-18)
RANGE_CELLS = (16, 64)
# --- d. sliver cells
SLIVER_BLOCKS, SLIVER_CELLS, SLIVER_QUALITY = (3, 9), (16, 128), 1e-3
# --- e. cells without a positive response inside a textured frame
PATCH_FRAME = (160, 224, 13, 3)
PATCH_FLAT = (32, 96, 64, 160)   # rows [y0, y1), columns [x0, x1) of the constant rectangle
PATCH_RAMP = (100, 150, 10, 60)  # of the horizontal ramp
PATCH_CELL, PATCH_BLOCK, PATCH_QUALITIES = 16, 5, (1e-18, 1e-3)
# --- f. compaction rounds of corner_select_kernel: 255, 256 and 272 cells of 16 px, every one kept
ROUND_FRAMES = ((240, 272), (256, 256), (256, 272))
ROUND_CELL, ROUND_BLOCK, ROUND_QUALITY, ROUND_P = 16, 3, 1e-18, 13
# --- g. a pair without features between pairs with many
MIXED_FRAME = (197, 331, 13, 197)
MIXED_CONFIG = (16, 3, 1e-3)


def kaleidoscope(h, w, P, seed, lo=0, hi=256):
    """A P x P block q of random bytes in [lo, hi), mirrored to 2P x 2P ([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]]),
    tiled and cropped to h x w.  A reflection about a vertical axis flips the sign of gx only, so the tensor sums A and C
    are unchanged and B changes sign: R is mirror-symmetric.  Pixels adjacent across an axis (horizontally, vertically,
    diagonally) have equal R, and the pattern repeats with period 2P, so equal maxima recur inside a cell, across its
    bands and across its waves whenever 2P < cell."""
    q = np.random.default_rng(seed).integers(lo, hi, size=(P, P), dtype=np.uint8)
    m = np.block([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]])
    reps = (-(-h // (2 * P)), -(-w // (2 * P)))
    return np.ascontiguousarray(np.tile(m, reps)[:h, :w])


def range_frame():
    """0 / 255 only: the largest gradients a byte image has"""
    h, w, P, seed = RANGE_FRAME
    return kaleidoscope(h, w, P, seed, 0, 2) * np.uint8(255)


def sliver_sizes(cell, block):
    """-> [(h, w, what)]: a last column and row of cells of e px, e = 1 and b (no valid pixel in them) and b + 1 (exactly
    one valid column, or row); then 1 px in width only and in height only (cw = 1 beside full-height cells: 85 bands)"""
    b = block // 2 + 1
    out = [(cell + e, 2 * cell + e, "e=%d" % e) for e in (1, b, b + 1)]
    return out + [(cell, 2 * cell + 1, "width+1"), (cell + 1, 2 * cell, "height+1")]


def sliver_frame(h, w):
    """(P and seed: with them the reference lists a feature on the one valid column and on the one valid row of every
    e = b + 1 size)"""
    return kaleidoscope(h, w, 13, 9)


def patch_frame():
    """a textured frame with a constant rectangle and a horizontal ramp inside"""
    h, w, P, seed = PATCH_FRAME
    img = kaleidoscope(h, w, P, seed)
    y0, y1, x0, x1 = PATCH_FLAT
    img[y0:y1, x0:x1] = 90
    y0, y1, x0, x1 = PATCH_RAMP
    img[y0:y1, x0:x1] = (40 + 4 * np.arange(x1 - x0)).astype(np.uint8)
    return img


def round_frame(h, w):
    return kaleidoscope(h, w, ROUND_P, h + w)


def mixed_frames():
    """[K, flat, K, K']: K' is K rolled by two pixels"""
    h, w, P, seed = MIXED_FRAME
    K = kaleidoscope(h, w, P, seed)
    return np.stack([K, np.full_like(K, 77), K, np.roll(K, 2, axis=1)])


_REF = {}


def detect(img, cell, block, quality):
    """fr.detect, computed once per (frame, configuration) and shared: do not write to the result"""
    key = (img.shape, img.tobytes(), cell, block, quality)
    if key not in _REF:
        _REF[key] = fr.detect(img, cell, block, quality)
        _REF[key].setflags(write=False)
    return _REF[key]


def cell_counts(pts, h, w, cell):
    """(ncx, ncy) int: the features per cell"""
    n = np.zeros((-(-w // cell), -(-h // cell)), np.int64)
    np.add.at(n, (pts[:, 0] // cell, pts[:, 1] // cell), 1)
    return n


def _tied_cells(img, cell, block, quality):
    """-> R, T, local maxima, and per cell whose best local maximum has R >= T and is attained more than once: the (y, x)
    of all local maxima that attain it"""
    R = fr.response(img, block)
    T = fr.threshold(R, quality)
    lm = fr.local_maxima(R)
    H, W = R.shape
    ys, xs = np.nonzero(lm & (R >= T))
    rv = R[ys, xs]
    cid = (xs // cell) * (-(-H // cell)) + ys // cell
    tied = []
    for c in np.unique(cid):
        m = cid == c
        top = rv[m] == rv[m].max()
        if top.sum() >= 2:
            tied.append(np.stack([ys[m][top], xs[m][top]], axis=-1))
    return R, T, lm, tied


def tie_stats(img, cell, block, quality):
    """counts from feature_reference only:
      plateau               valid pixels with R >= T that are >= all valid neighbours and equal to at least one
      dropped_by_tie        those of them that local_maxima rejects
      cells_with_tied_best  cells whose best local maximum's R is attained by two or more local maxima with R >= T
      kept                  len(detect(...))
      r_max, T"""
    R, T, lm, tied = _tied_cells(img, cell, block, quality)
    H, W = R.shape
    pad = np.full((H + 2, W + 2), fr.NO_RESPONSE, np.int64)
    pad[1:-1, 1:-1] = R
    ge = (R != fr.NO_RESPONSE) & (R >= T)
    eq = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                q = pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
                ge &= R >= q
                eq |= R == q
    plateau = ge & eq
    return dict(plateau=int(plateau.sum()), dropped_by_tie=int((plateau & ~lm).sum()), cells_with_tied_best=len(tied),
                kept=len(detect(img, cell, block, quality)), r_max=int(R[R != fr.NO_RESPONSE].max()), T=int(T))


def tie_paths(img, cell, block, quality):
    """Where the tied bests of tie_stats' cells_with_tied_best sit in corner_cell_kernel's layout (nc = cw + 2 columns per
    band, nb = 256 // nc bands of rpb = ceil(ch / nb) rows, thread = band nc + column, wave = thread // 64).  -> the
    number of cells in which two of the tied local maxima meet
      thread     in one thread (one column of one band): corner_beats in the thread's own loop decides
      wave       in two threads of one wave: the shuffle butterfly decides
      workgroup  in two waves: the reduction through LDS decides"""
    R, T, lm, tied = _tied_cells(img, cell, block, quality)
    H, W = R.shape
    out = dict(thread=0, wave=0, workgroup=0)
    for yx in tied:
        y0, x0 = yx[0, 0] // cell * cell, yx[0, 1] // cell * cell
        cw, ch = min(cell, W - x0), min(cell, H - y0)
        nc = cw + 2
        nb = THREADS // nc
        rpb = -(-ch // nb)
        t = (yx[:, 0] - y0) // rpb * nc + yx[:, 1] - x0 + 1
        assert t.max() < nb * nc
        wv = t // 64
        out["thread"] += len(np.unique(t)) < len(t)
        out["wave"] += any(len(np.unique(t[wv == v])) >= 2 for v in np.unique(wv))
        out["workgroup"] += len(np.unique(wv)) >= 2
    return out
