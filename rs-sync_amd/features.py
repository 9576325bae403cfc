"""Grayscale frames -> corner features tracked forward and backward on the GPU (include/rssync_features.h).

Each frame's corners are found per cell (an exact integer Harris response, non-maximum suppression, a threshold
relative to the frame's largest response; csrc/kernels/features.hpp), tracked to the next frame with the tracker's
pyramidal LK and back again; tracks that do not come back within ``max_fb_error`` get status 4.  ``features_frames``
hands the status-0 tracks of each pair to ``set_track_pixels``.

Frames are taken as in ``track`` (numpy arrays, pitched views, uint8 device tensors); so are the LK settings
(``window``, ``levels``, ``max_iters``, ``epsilon``, ``min_eig``).
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import track
from .problem import RsSyncError, product_library

_PD = C.POINTER(C.c_double)
_SZ = C.c_size_t


class FeatureParams(C.Structure):
    """rssync_feature_params: 0 = the default"""
    _fields_ = [("cell", C.c_int32), ("block", C.c_int32), ("quality", C.c_double), ("max_fb_error", C.c_double),
                ("min_tracks", C.c_int32), ("lk", track.TrackParams)]


class _Cfg(C.Structure):
    """rship_feature_cfg (csrc/track_hip.h), for the tests' direct path"""
    _fields_ = [("lk", track._Cfg), ("cell", C.c_uint32), ("block", C.c_uint32), ("quality", C.c_double),
                ("max_fb_error", C.c_float)]


_PI32, _PU32, _PF = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
# name -> (restype, argtypes): every function include/rssync_features.h declares, and the internal launchers the tests use
SIGNATURES = {
    "rssync_features_track": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, C.POINTER(FeatureParams), _PD, _PD,
                                        C.c_void_p, _PF, _PU32, _SZ, C.POINTER(_SZ)]),
    "rssync_features_frames": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, _PD, C.c_int64, C.c_void_p,
                                         C.POINTER(FeatureParams), C.POINTER(_SZ)]),
    "rship_features_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, C.POINTER(_Cfg), _PI32, _PU32, _PF, _PF,
                                       C.c_void_p, _PF]),
    "rship_track_list": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, C.POINTER(track._Cfg), _PI32, _PU32,
                                   C.c_uint32, _PF, C.c_void_p, _PF]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}

DEFAULTS = dict(cell=64, block=5, quality=0.01, max_fb_error=0.5, min_tracks=8)
STATUS = {**track.STATUS, 4: "forward-backward mismatch"}

# per pair k, the first counts[k] entries of each array are set
Features = namedtuple("Features", "counts points_a points_b status fb_error")


def library():
    """the product library with the feature tracker's signatures attached"""
    track.library()
    return product_library(SIGNATURES)


def _lib_of(problem):
    track._lib_of(problem)
    return library()


def params(cell=64, block=5, quality=0.01, max_fb_error=0.5, min_tracks=8, **lk):
    """-> FeatureParams; lk: the tracker's LK settings (track.DEFAULTS but grid_step, which must stay 0)"""
    return FeatureParams(int(cell), int(block), float(quality), float(max_fb_error), int(min_tracks), track.params(0, **lk))


def n_cells(width, height, cell=64):
    return -(-width // cell) * -(-height // cell)


def track_features(problem, frames, **kw):
    """-> Features(counts (n-1,), points_a (n-1, S, 2), points_b (n-1, S, 2), status (n-1, S) uint8,
    fb_error (n-1, S) float32), S = the frame's cells; pair k's tracks are the first counts[k] entries"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = track._frames(frames)
    prm = params(**kw)
    cell = kw.get("cell", DEFAULTS["cell"]) or DEFAULTS["cell"]
    S = n_cells(w, h, cell) if 0 < cell and w and h else 0
    m = max(n - 1, 1)
    pa, pb = np.zeros((m, max(S, 1), 2)), np.zeros((m, max(S, 1), 2))
    st = np.zeros((m, max(S, 1)), np.uint8)
    fb = np.zeros((m, max(S, 1)), np.float32)
    cnt = np.zeros(m, np.uint32)
    got = C.c_size_t()
    track._check(problem, lib.rssync_features_track(problem._h, ptr, n, w, h, pitch, fstride, C.byref(prm),
                                                    pa.ctypes.data_as(_PD), pb.ctypes.data_as(_PD), st.ctypes.data,
                                                    fb.ctypes.data_as(_PF), cnt.ctypes.data_as(_PU32), S, C.byref(got)))
    del keep
    return Features(cnt[:n - 1], pa[:n - 1, :S], pb[:n - 1, :S], st[:n - 1, :S], fb[:n - 1, :S])


def features_frames(problem, frames, frame_times, lens, first_frame=0, **kw):
    """detect and track, then set_track_pixels(first_frame + k, t[k], t[k+1], kept a_k, kept b_k, lens, H) for every pair
    that keeps at least min_tracks tracks of status 0 -> the number of pairs handed on"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = track._frames(frames)
    t = np.ascontiguousarray(frame_times, np.float64)
    if t.shape != (n,):
        raise ValueError("frame_times must hold one time per frame")
    L = np.ascontiguousarray(lens, np.float64)
    if L.shape != (9,):
        raise ValueError("lens = (ro, fx, fy, cx, cy, k1, k2, k3, k4)")
    prm = params(**kw)
    n_set = C.c_size_t()
    track._check(problem, lib.rssync_features_frames(problem._h, ptr, n, w, h, pitch, fstride, t.ctypes.data_as(_PD),
                                                     int(first_frame), L.ctypes.data, C.byref(prm), C.byref(n_set)))
    del keep
    return n_set.value


def _ctx_call(problem, lib, fn, *args):
    ctx = C.c_void_p(problem.device_context())
    if fn(ctx, *args):
        raise RsSyncError(lib.rship_last_error(ctx).decode())


def _track_cfg(w, h, window=21, levels=4, max_iters=30, epsilon=0.01, min_eig=1e-4):
    return track._Cfg(w, h, 0, window, levels, max_iters, epsilon, min_eig)


def raw_features(problem, frames, cell=64, block=5, quality=0.01, max_fb_error=0.5, **lk):
    """the device launcher itself (tests): -> counts (n-1,), points (n-1, S, 2) int32, flow_fwd, flow_bwd (n-1, S, 2)
    float32, status (n-1, S), fb_error (n-1, S); every parameter given explicitly (no 0 = default here)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = track._frames(frames)
    cfg = _Cfg(_track_cfg(w, h, **lk), cell, block, quality, max_fb_error)
    S = n_cells(w, h, cell)
    pts = np.zeros((n - 1, S, 2), np.int32)
    cnt = np.zeros(n - 1, np.uint32)
    ff, fbk = np.zeros((n - 1, S, 2), np.float32), np.zeros((n - 1, S, 2), np.float32)
    st = np.zeros((n - 1, S), np.uint8)
    fb = np.zeros((n - 1, S), np.float32)
    _ctx_call(problem, lib, lib.rship_features_track, ptr, n, pitch, fstride, C.byref(cfg), pts.ctypes.data_as(_PI32),
              cnt.ctypes.data_as(_PU32), ff.ctypes.data_as(_PF), fbk.ctypes.data_as(_PF), st.ctypes.data, fb.ctypes.data_as(_PF))
    del keep
    return cnt, pts, ff, fbk, st, fb


def track_list(problem, frames, points, counts, **lk):
    """LK at integer points (n-1, cap, 2) per pair, the first counts[k] of pair k (tests) -> flow (n-1, cap, 2),
    status (n-1, cap), residual (n-1, cap)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = track._frames(frames)
    pts = np.ascontiguousarray(points, np.int32)
    cnt = np.ascontiguousarray(counts, np.uint32)
    if pts.ndim != 3 or pts.shape[0] != n - 1 or pts.shape[2] != 2 or cnt.shape != (n - 1,):
        raise ValueError("points (n-1, cap, 2) and counts (n-1,)")
    cap = pts.shape[1]
    cfg = _track_cfg(w, h, **lk)
    flow = np.zeros((n - 1, cap, 2), np.float32)
    st = np.zeros((n - 1, cap), np.uint8)
    res = np.zeros((n - 1, cap), np.float32)
    _ctx_call(problem, lib, lib.rship_track_list, ptr, n, pitch, fstride, C.byref(cfg), pts.ctypes.data_as(_PI32),
              cnt.ctypes.data_as(_PU32), cap, flow.ctypes.data_as(_PF), st.ctypes.data, res.ctypes.data_as(_PF))
    del keep
    return flow, st, res
