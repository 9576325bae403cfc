"""numpy restatement of the feature tracker (include/rssync_features.h, rs-sync_amd/csrc/kernels/features.hpp), for the
tests.

  response   integer gradients, int32 structure-tensor sums, int64 Harris response: bit-exact with corner_cell_kernel
  detect     non-maximum suppression, threshold and cell winners: bit-exact with corner_select_kernel's lists
  track_fb   the forward and backward LK passes with tests/track_reference.py's tracker (float64), the fb check
"""
import math

import numpy as np

import track_reference as tr

STATUS_FB_MISMATCH = 4
NO_RESPONSE = np.iinfo(np.int64).min


def response(frame, block=5):
    """-> R (H, W) int64, with NO_RESPONSE at the pixels that have none (closer than b = block // 2 + 1 to the border)"""
    I = np.asarray(frame).astype(np.int64)
    H, W = I.shape
    r, b = block // 2, block // 2 + 1
    gx = np.zeros((H, W), np.int64)
    gy = np.zeros((H, W), np.int64)
    gx[:, 1:-1] = I[:, 2:] - I[:, :-2]
    gy[1:-1, :] = I[2:, :] - I[:-2, :]

    def box(v):
        """sum over the block x block window centred on each pixel whose window lies inside the frame"""
        c = np.zeros((H + 1, W + 1), np.int64)
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        n = 2 * r + 1
        out = np.zeros((H, W), np.int64)
        out[r:H - r, r:W - r] = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
        return out

    A, B, C = box(gx * gx), box(gx * gy), box(gy * gy)
    assert max(A.max(), C.max(), np.abs(B).max()) < 2 ** 31        # int32 on the device
    R = 64 * (A * C - B * B) - 3 * (A + C) ** 2
    valid = np.zeros((H, W), bool)
    valid[b:H - b, b:W - b] = True
    return np.where(valid, R, NO_RESPONSE)


def local_maxima(R):
    """p beats each of its valid 8-neighbours: a larger R, or an equal R and a smaller raster index"""
    H, W = R.shape
    pad = np.full((H + 2, W + 2), NO_RESPONSE, np.int64)
    pad[1:-1, 1:-1] = R
    lm = R != NO_RESPONSE
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            q = pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
            earlier = dy < 0 or (dy == 0 and dx < 0)        # q's raster index is smaller than p's
            lm &= (R > q) if earlier else (R >= q)
    return lm


def threshold(R, quality=0.01):
    """T = max(1, ceil(quality * (double) R_max)) over the valid pixels"""
    rmax = int(R[R != NO_RESPONSE].max())
    return max(1, math.ceil(quality * float(rmax)))


def detect(frame, cell=64, block=5, quality=0.01):
    """-> (K, 2) int64 features (x, y) in cell order (cells x-major: cx outer, cy inner)"""
    R = response(frame, block)
    H, W = R.shape
    lm = local_maxima(R)
    T = threshold(R, quality)
    ys, xs = np.nonzero(lm)
    rv = R[ys, xs]
    ncy = -(-H // cell)
    cid = (xs // cell) * ncy + ys // cell
    order = np.lexsort((ys * W + xs, -rv, cid))             # by cell, then the best first
    cid, xs, ys, rv = cid[order], xs[order], ys[order], rv[order]
    first = np.ones(len(cid), bool)
    first[1:] = cid[1:] != cid[:-1]
    keep = first & (rv >= T)
    return np.stack([xs[keep], ys[keep]], axis=-1).astype(np.int64).reshape(-1, 2)


def track_fb(pyr_a, pyr_b, pts, max_fb_error=0.5, diag=False, **lk):
    """-> flow_fwd (P, 2), flow_bwd (P, 2), status (P,), fb_error (P,) for the features pts of frame a.  The backward pass
    runs from b = a + flow_fwd for the tracks of forward status 0; the others have a NaN fb_error.  diag=True adds the
    decision margins of tests/track_reference.py's track_pair, the smaller of the forward and the backward pass's."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    if diag:
        flow, st, _, m = tr.track_pair(pyr_a, pyr_b, pts, diag=True, **lk)
    else:
        flow, st, _ = tr.track_pair(pyr_a, pyr_b, pts, **lk)
    back = np.zeros_like(flow)
    fb = np.full(len(pts), np.nan)
    ok = st == tr.STATUS_OK
    if ok.any():
        if diag:
            fb_flow, fb_st, _, mb = tr.track_pair(pyr_b, pyr_a, pts[ok] + flow[ok], diag=True, **lk)
            for k in ("eig", "det", "conv", "border"):
                m[k][ok] = np.minimum(m[k][ok], mb[k])
        else:
            fb_flow, fb_st, _ = tr.track_pair(pyr_b, pyr_a, pts[ok] + flow[ok], **lk)
        back[ok] = fb_flow
        fb[ok] = np.linalg.norm(flow[ok] + fb_flow, axis=-1)
        bad = (fb_st != tr.STATUS_OK) | (fb[ok] > max_fb_error)
        st = st.copy()
        st[np.nonzero(ok)[0][bad]] = STATUS_FB_MISMATCH
    if diag:
        return flow, back, st, fb, m
    return flow, back, st, fb


def fb_edge(fb_ref, max_fb=0.5, tol=1e-3):
    """(P,) bool: the tracks whose reference fb error is within tol px of the bound, where fp32 and fp64 may split"""
    return np.abs(np.nan_to_num(fb_ref, nan=1e9) - max_fb) < tol


def fb_ok(st_dev, st_ref, fb_ref, max_fb=0.5, tol=1e-3):
    """statuses equal, apart from tracks whose fb error is within tol px of the bound (fp32 against fp64)"""
    return (st_dev == st_ref) | fb_edge(fb_ref, max_fb, tol)


def track(frames, cell=64, block=5, quality=0.01, max_fb_error=0.5, levels=4, **lk):
    """frames (n, H, W) uint8 -> a list over the n-1 pairs of (points_a (K, 2), points_b (K, 2), status (K,), fb_error (K,))"""
    pyrs = [tr.pyramid(f, levels) for f in frames]
    out = []
    for k in range(len(frames) - 1):
        a = detect(frames[k], cell, block, quality).astype(np.float64)
        flow, _, st, fb = track_fb(pyrs[k], pyrs[k + 1], a, max_fb_error, **lk)
        out.append((a, a + flow, st, fb))
    return out
