"""The LMedS selection (core_private.cpp:34-59) restated in numpy, for the tests that check which hypothesis a search picks:
the lower quartile of one hypothesis in fp64, the first-wins arg-min over a list of hypotheses, the same arg-min on the
DEVICE'S OWN residuals (the tolerance-free anchor of tests/test_gpu_fuzz.py and tests/test_gpu_guess_motion.py), and the interval
an fp32 search's quartile can lie in (what makes a device-vs-fp64 flip legitimate)."""
import numpy as np


def lower_quartile_fp64(P, i0, i1):
    """core_private.cpp:35-52 in numpy fp64: the N/4-th smallest squared residual of the hypothesis drawn as rows (i0, i1)"""
    nrm = np.linalg.norm(P, axis=1)
    nP = P / np.where(nrm < 1e-12, 1.0, nrm)[:, None]
    v = np.cross(P[i0], P[i1])
    nv = np.linalg.norm(v)
    if nv >= 1e-12:
        v = v / nv
    return float(np.sort((nP @ v) ** 2)[len(P) // 4])


def guess_winner64(P, pairs):
    """core_private.cpp:48-56 over a list of row pairs: the index of the hypothesis whose lower quartile (lower_quartile_fp64)
    is smallest, the FIRST of equals (med < least_med, strict); -1 if no quartile is finite"""
    best, least = -1, np.inf
    for h, (i0, i1) in enumerate(pairs):
        med = lower_quartile_fp64(P, i0, i1)
        if med < least:
            best, least = h, med
    return best


def flip_interval(P, i0, i1):
    """-> (lo, hi, rq): where the fp32 search's lower-quartile |residual| of hypothesis (i0, i1) can lie, given rows known
    to 5e-7 absolute (profiles/r4_config2_parity.json).  The direction v = P[i0] x P[i1] is off by up to
    err_v = 5e-7 (1/|P[i0]| + 1/|P[i1]|) / sin(angle) radians -- 0.2 of that is taken, the largest fraction a soak of 6000
    cases showed was 0.066 --; a residual n_i.v by that plus its own row's 5e-7 / |P_i|; the rows whose residual lies within
    their error of the quartile value may change sides, and the quartile moves by as many order statistics."""
    nr = np.linalg.norm(P, axis=1)
    nP = P / np.where(nr < 1e-12, 1.0, nr)[:, None]
    v = np.cross(P[i0], P[i1])
    nv = np.linalg.norm(v)
    if nv >= 1e-12:
        v = v / nv
    r = np.abs(nP @ v)
    sin_a = nv / max(nr[i0] * nr[i1], 1e-300) if nv >= 1e-12 else 1.0
    err_v = 5e-7 * (1.0 / max(nr[i0], 1e-300) + 1.0 / max(nr[i1], 1e-300)) / max(sin_a, 1e-300)
    e = 0.2 * err_v * np.linalg.norm(v) + 5e-7 / np.maximum(nr, 1e-300)
    order = np.argsort(r)
    kq = len(P) // 4
    rq = r[order[kq]]
    m = int(np.sum(np.abs(r - rq) <= e)) - 1            # rows (other than the quartile's own) that may change sides
    m = max(m, 0)
    lo_k, hi_k = max(kq - m, 0), min(kq + m, len(P) - 1)
    return float(r[order[lo_k]] - e[order[lo_k]]), float(r[order[hi_k]] + e[order[hi_k]]), float(rq)


def exact_winners(res, counts):
    """core_private.cpp:48-56 on the device's OWN residuals: res [candidates][frames][hypotheses][rows] of |r| (float32);
    per (candidate, frame) the hypothesis whose sorted residuals' element at index N / 4 is smallest, the first of equals
    (strict <).  |r| orders like the r^2 the reference sorts.  -> int32 [candidates][frames]"""
    C_, F_, H_, _ = res.shape
    out = np.full((C_, F_), -1, dtype=np.int32)
    for j, n in enumerate(counts):
        r = res[:, j, :, :n]                                        # [C][H][n]
        q = np.partition(r, n // 4, axis=2)[:, :, n // 4]           # the element std::sort would leave at index n / 4
        q = np.where(np.isnan(q), np.inf, q)
        win = np.argmin(q, axis=1)                                  # first minimum
        out[:, j] = np.where(np.isfinite(q[np.arange(C_), win]), win, -1)
    return out
