"""numpy restatement of the tracker (include/rssync_track.h, rs-sync_amd/csrc/kernels/track.hpp), for the tests.

  grid       the driver's loop (core_testcode.cpp:124-132), written as that loop
  pyramid    float32, the kernel's tap order: bit-exact with pyr_down_kernel
  track      inverse-compositional translational LK, vectorised over points; bilinear samples and sums in float64
             (the kernel: fp32 samples, fp32 wave sums), the same level loop, statuses and stopping rules
  margins    track_pair(..., diag=True): how close each point came to every decision it took, so that a comparison with
             the fp32 kernel can tell a legitimate fp32/fp64 split at a threshold from a wrong kernel (near_decision)
"""
import numpy as np

STATUS_OK, STATUS_ILL, STATUS_LEFT, STATUS_CAP = 0, 1, 2, 3


def grid(width, height, step=200):
    """core_testcode.cpp:124-132: for (i = step; i < width; i += step) for (j = step; j < height; j += step)"""
    pts = []
    i = step
    while i < width:
        j = step
        while j < height:
            pts.append((i, j))
            j += step
        i += step
    return np.array(pts, np.float64).reshape(-1, 2)


def _reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _tap5(a, b, c, d, e):
    four, six = np.float32(4.0), np.float32(6.0)
    return ((a + e) + (b + d) * four) + c * six


def pyr_down(img):
    """one level: binomial [1 4 6 4 1] / 16 both ways, even pixels, reflect-101; float32 in the kernel's tap order"""
    img = np.asarray(img).astype(np.float32)
    h, w = img.shape
    ow, oh = (w + 1) // 2, (h + 1) // 2
    cols = _reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)
    hs = _tap5(*(img[:, cols[:, k]] for k in range(5)))
    rows = _reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)
    return _tap5(*(hs[rows[:, k], :] for k in range(5))) * np.float32(1.0 / 256.0)


def pyramid(frame, levels=4):
    """[level 0 (as float32), level 1, ...]"""
    out = [np.asarray(frame).astype(np.float32)]
    for _ in range(1, levels):
        out.append(pyr_down(out[-1]))
    return out


def _sample(img, X, Y):
    """bilinear, coordinates clamped to the border (float64)"""
    h, w = img.shape
    x0, y0 = np.floor(X), np.floor(Y)
    fx, fy = X - x0, Y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    im = img.astype(np.float64, copy=False)
    top = im[ya, xa] + fx * (im[ya, xb] - im[ya, xa])
    bot = im[yb, xa] + fx * (im[yb, xb] - im[yb, xa])
    return top + fy * (bot - top)


def _template(A, al, dx, dy):
    """template, its central-difference gradients and the structure tensor at the positions al (P, 2) of image A"""
    TX, TY = al[:, :1] + dx, al[:, 1:] + dy
    T = _sample(A, TX, TY)
    GX = 0.5 * (_sample(A, TX + 1, TY) - _sample(A, TX - 1, TY))
    GY = 0.5 * (_sample(A, TX, TY + 1) - _sample(A, TX, TY - 1))
    return T, GX, GY, (GX * GX).sum(1), (GX * GY).sum(1), (GY * GY).sum(1)


def _min_eig(hxx, hxy, hyy, area):
    return 0.5 * (hxx + hyy - np.sqrt((hxx - hyy) ** 2 + 4 * hxy * hxy)) / area


def min_eigenvalue(img, pts, window=21):
    """(P,) the smallest eigenvalue of the structure tensor / window area at the points of img (level 0): the number the
    min_eig test compares"""
    r = window // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    dx, dy = dx.ravel()[None, :].astype(np.float64), dy.ravel()[None, :].astype(np.float64)
    _, _, _, hxx, hxy, hyy = _template(np.asarray(img), np.asarray(pts, np.float64).reshape(-1, 2), dx, dy)
    return _min_eig(hxx, hxy, hyy, window * window)


def track_pair(pyr_a, pyr_b, pts, window=21, max_iters=30, epsilon=0.01, min_eig=1e-4, diag=False):
    """-> flow (P, 2), status (P,) uint8, residual (P,) for the points pts (P, 2) from frame a to frame b.

    diag=True adds a fourth value, a dict of (P,) float64 margins: for each point the smallest distance to the threshold
    of every decision of that kind it took (inf when it took none):
      eig     min-eig test, every level: |min_eig(H) - min_eig| / max(min_eig, (hxx + hyy) / (2 area)) -- relative to the
              larger of the bound and the tensor's scale, which is what fp32's rounding of the eigenvalue is relative to
      det     det > 0, at the levels whose min-eig test passed: det / (hxx hyy + hxy^2)
      conv    every convergence test: |ux^2 + uy^2 - eps^2| / eps^2
      border  every border test (each iteration's, and the final one at level 0): distance of the position to the
              nearest border line, in pixels of that level -- at a flow other than exactly 0: with none, the position is
              the point's own, exact in fp32 (integer base + dyadic fraction) as in fp64, and the test cannot split
    and left_level (P,) int: the level whose iteration found the point outside (status 2 by the level loop's break), -1
    for none (the final level-0 test is not a level's break).
    """
    levels = len(pyr_a)
    r = window // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    dx, dy = dx.ravel()[None, :].astype(np.float64), dy.ravel()[None, :].astype(np.float64)
    area = window * window
    P = pts.shape[0]
    flow = np.zeros((P, 2))
    status = np.zeros(P, np.uint8)
    active = np.ones(P, bool)           # not yet out of the image
    m = {k: np.full(P, np.inf) for k in ("eig", "det", "conv", "border")}
    m["left_level"] = np.full(P, -1)

    def note(kind, idx, v):
        np.minimum.at(m[kind], idx, v)

    def border_margin(pos, w, h):
        return np.minimum(np.minimum(np.abs(pos[:, 0]), np.abs(w - 1 - pos[:, 0])),
                          np.minimum(np.abs(pos[:, 1]), np.abs(h - 1 - pos[:, 1])))

    for l in range(levels - 1, -1, -1):
        if l != levels - 1:
            flow *= 2.0
        A, B = pyr_a[l], pyr_b[l]
        h, w = A.shape
        al = pts / 2.0 ** l
        T, GX, GY, hxx, hxy, hyy = _template(A, al, dx, dy)
        det = hxx * hyy - hxy * hxy
        me = _min_eig(hxx, hxy, hyy, area)
        ok = (me >= min_eig) & (det > 0)
        if diag:
            i = np.nonzero(active)[0]
            note("eig", i, np.abs(me[i] - min_eig) / np.maximum(min_eig, (hxx[i] + hyy[i]) / (2 * area)))
            i = np.nonzero(active & (me >= min_eig))[0]
            note("det", i, np.abs(det[i]) / (hxx[i] * hyy[i] + hxy[i] * hxy[i]))
        if l == 0:
            status[active & ~ok] = STATUS_ILL
        run = active & ok
        conv = np.zeros(P, bool)
        for _ in range(max_iters):
            todo = run & ~conv
            if not todo.any():
                break
            pos = al + flow
            if diag:
                i = np.nonzero(todo & (flow != 0).any(1))[0]
                note("border", i, border_margin(pos[i], w, h))
            out = (pos[:, 0] < 0) | (pos[:, 0] > w - 1) | (pos[:, 1] < 0) | (pos[:, 1] > h - 1)
            left = todo & out
            if left.any():
                status[left] = STATUS_LEFT
                if diag:
                    m["left_level"][left] = l
                active[left] = False
                run[left] = False
                todo &= ~out
            i = np.nonzero(todo)[0]
            if i.size == 0:
                break
            e = _sample(B, pos[i, :1] + dx, pos[i, 1:] + dy) - T[i]
            ex, ey = (GX[i] * e).sum(1), (GY[i] * e).sum(1)
            ux = (hyy[i] * ex - hxy[i] * ey) / det[i]
            uy = (hxx[i] * ey - hxy[i] * ex) / det[i]
            flow[i, 0] -= ux
            flow[i, 1] -= uy
            conv[i] |= ux * ux + uy * uy < epsilon * epsilon
            if diag:
                note("conv", i, np.abs(ux * ux + uy * uy - epsilon * epsilon) / (epsilon * epsilon))
        if l == 0:
            status[run & ~conv] = STATUS_CAP
    H0, W0 = pyr_a[0].shape
    pos = pts + flow
    if diag:
        i = np.nonzero(active & (flow != 0).any(1))[0]
        note("border", i, border_margin(pos[i], W0, H0))
    out = (pos[:, 0] < 0) | (pos[:, 0] > W0 - 1) | (pos[:, 1] < 0) | (pos[:, 1] > H0 - 1)
    status[out] = STATUS_LEFT
    px = np.clip(pos[:, :1], -1, W0) + dx
    py = np.clip(pos[:, 1:], -1, H0) + dy
    res = np.abs(_sample(pyr_b[0], px, py) - _sample(pyr_a[0], pts[:, :1] + dx, pts[:, 1:] + dy)).mean(1)
    if diag:
        return flow, status, res, m
    return flow, status, res


# Tolerances of near_decision.  The kernel samples in fp32 (relative error ~6e-8 of a pixel value) and sums a window's
# products in fp32 (relative ~1e-6 of the sum over 441 terms); the eigenvalue, det and update inherit that, so 1e-4 of
# their scale is ~100 times the largest split fp32 and fp64 can show.  A position is fp32 relative to an integer base:
# its rounding is ~1e-6 px, and the flow behind it differs from fp64's by at most ~1e-4 px (3 x 3 windows; ~1e-6 px from
# 7 x 7 up), so 1e-3 px of a border is an order beyond either.  An update's length is decided against eps in fp32 with an
# error below 1e-6 px (measured against the kernel down to epsilon = 1e-4): CONV_PX states it in pixels, so that the
# relative tolerance follows epsilon (4e-4 at the default 0.01, 0.02 at 1e-4).
NEAR_REL = 1e-4
NEAR_PX = 1e-3
CONV_PX = 1e-6


def near_decision(margins, epsilon, rel=NEAR_REL, px=NEAR_PX, conv_px=CONV_PX):
    """(P,) bool: the points that came within a tolerance of a decision's threshold (track_pair(..., diag=True)).  The
    convergence margin is relative to eps^2; an fp32 error d in the update length moves it by ~2 d / eps, so the
    tolerance there is max(rel, 2 conv_px / eps)."""
    conv_rel = max(rel, 2.0 * conv_px / epsilon)
    return (margins["eig"] < rel) | (margins["det"] < rel) | (margins["conv"] < conv_rel) | (margins["border"] < px)


def track(frames, step=200, window=21, levels=4, max_iters=30, epsilon=0.01, min_eig=1e-4):
    """frames (n, H, W) uint8 -> points_a (P, 2), points_b (n-1, P, 2), status (n-1, P), residual (n-1, P)"""
    n, H, W = frames.shape
    pts = grid(W, H, step)
    pyrs = [pyramid(f, levels) for f in frames]
    pb = np.zeros((n - 1, pts.shape[0], 2))
    st = np.zeros((n - 1, pts.shape[0]), np.uint8)
    rs = np.zeros((n - 1, pts.shape[0]))
    for k in range(n - 1):
        flow, st[k], rs[k] = track_pair(pyrs[k], pyrs[k + 1], pts, window, max_iters, epsilon, min_eig)
        pb[k] = pts + flow
    return pts, pb, st, rs
