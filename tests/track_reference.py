"""numpy restatement of the tracker (include/rssync_track.h, rs-sync_amd/csrc/kernels/track.hpp), for the tests.

  grid       the driver's loop (core_testcode.cpp:124-132), written as that loop
  pyramid    float32, the kernel's tap order: bit-exact with pyr_down_kernel
  track      inverse-compositional translational LK, vectorised over points; bilinear samples and sums in float64
             (the kernel: fp32 samples, fp32 wave sums), the same level loop, statuses and stopping rules
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


def track_pair(pyr_a, pyr_b, pts, window=21, max_iters=30, epsilon=0.01, min_eig=1e-4):
    """-> flow (P, 2), status (P,) uint8, residual (P,) for the points pts (P, 2) from frame a to frame b"""
    levels = len(pyr_a)
    r = window // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    dx, dy = dx.ravel()[None, :].astype(np.float64), dy.ravel()[None, :].astype(np.float64)
    area = window * window
    P = pts.shape[0]
    flow = np.zeros((P, 2))
    status = np.zeros(P, np.uint8)
    active = np.ones(P, bool)           # not yet out of the image
    for l in range(levels - 1, -1, -1):
        if l != levels - 1:
            flow *= 2.0
        A, B = pyr_a[l], pyr_b[l]
        h, w = A.shape
        al = pts / 2.0 ** l
        TX, TY = al[:, :1] + dx, al[:, 1:] + dy
        T = _sample(A, TX, TY)
        GX = 0.5 * (_sample(A, TX + 1, TY) - _sample(A, TX - 1, TY))
        GY = 0.5 * (_sample(A, TX, TY + 1) - _sample(A, TX, TY - 1))
        hxx, hxy, hyy = (GX * GX).sum(1), (GX * GY).sum(1), (GY * GY).sum(1)
        det = hxx * hyy - hxy * hxy
        me = 0.5 * (hxx + hyy - np.sqrt((hxx - hyy) ** 2 + 4 * hxy * hxy)) / area
        ok = (me >= min_eig) & (det > 0)
        if l == 0:
            status[active & ~ok] = STATUS_ILL
        run = active & ok
        conv = np.zeros(P, bool)
        for _ in range(max_iters):
            todo = run & ~conv
            if not todo.any():
                break
            pos = al + flow
            out = (pos[:, 0] < 0) | (pos[:, 0] > w - 1) | (pos[:, 1] < 0) | (pos[:, 1] > h - 1)
            left = todo & out
            if left.any():
                status[left] = STATUS_LEFT
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
        if l == 0:
            status[run & ~conv] = STATUS_CAP
    H0, W0 = pyr_a[0].shape
    pos = pts + flow
    out = (pos[:, 0] < 0) | (pos[:, 0] > W0 - 1) | (pos[:, 1] < 0) | (pos[:, 1] > H0 - 1)
    status[out] = STATUS_LEFT
    px = np.clip(pos[:, :1], -1, W0) + dx
    py = np.clip(pos[:, 1:], -1, H0) + dy
    res = np.abs(_sample(pyr_b[0], px, py) - _sample(pyr_a[0], pts[:, :1] + dx, pts[:, 1:] + dy)).mean(1)
    return flow, status, res


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
