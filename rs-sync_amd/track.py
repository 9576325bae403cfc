"""Grayscale frames -> tracked grid points on the GPU (include/rssync_track.h).

The reference driver gets the pixel pairs it hands to the solver from OpenCV's optical flow at a grid of
points (core_testcode.cpp:97-133).  Here a sparse pyramidal Lucas-Kanade on gfx950 does it
(csrc/kernels/track.hpp), and ``track_frames`` feeds the result straight into ``set_track_pixels``.

``frames`` is an ``(n, H, W)`` uint8 array: numpy (pitched views included) or a uint8 torch tensor on the
problem's device.  Calls keep no state; a long video goes in overlapping batches (frames ``[k, k+B]``,
then ``[k+B, k+2B]``, ...), see INTEGRATION.md.

Its own ctypes table, bound to the product library only: the tracker has no CPU test double.
"""
import ctypes as C

import numpy as np

from .problem import RsSyncError, product_library, product_only

_PD = C.POINTER(C.c_double)


class TrackParams(C.Structure):
    """rssync_track_params: 0 = the default"""
    _fields_ = [("grid_step", C.c_int32), ("window", C.c_int32), ("levels", C.c_int32), ("max_iters", C.c_int32),
                ("epsilon", C.c_double), ("min_eig", C.c_double)]


class _Cfg(C.Structure):
    """rship_track_cfg (csrc/track_hip.h), for the pyramid read-back used by the tests"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("step", C.c_uint32), ("window", C.c_uint32),
                ("levels", C.c_uint32), ("max_iters", C.c_uint32), ("epsilon", C.c_float), ("min_eig", C.c_float)]


_SZ = C.c_size_t
# name -> (restype, argtypes): every function include/rssync_track.h declares, and the internal pyramid read-back
SIGNATURES = {
    "rssync_track_points": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, C.POINTER(TrackParams), _PD, _PD,
                                      C.c_void_p, C.POINTER(C.c_float), _SZ, C.POINTER(_SZ)]),
    "rssync_track_frames": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, _PD, C.c_int64, C.c_void_p,
                                      C.POINTER(TrackParams)]),
    "rship_track_pyramid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, C.POINTER(_Cfg), C.POINTER(C.c_float)]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}

DEFAULTS = dict(grid_step=200, window=21, levels=4, max_iters=30, epsilon=0.01, min_eig=1e-4)
STATUS = {0: "ok", 1: "ill-conditioned", 2: "left the image", 3: "iteration cap"}


def library():
    """the product library with the tracker's signatures attached"""
    return product_library(SIGNATURES)


def grid(width, height, step=200):
    """the driver's grid (core_testcode.cpp:124-132): (P, 2) float64, x-major"""
    xs = np.arange(step, width, step)
    ys = np.arange(step, height, step)
    return np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)


def params(grid_step=200, **kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown tracker parameters: %s" % ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, grid_step=grid_step, **kw)
    return TrackParams(int(p["grid_step"]), int(p["window"]), int(p["levels"]), int(p["max_iters"]), float(p["epsilon"]),
                       float(p["min_eig"]))


def _frames(frames):
    """-> (pointer, n, height, width, pitch, frame_stride, keep-alive)"""
    if type(frames).__module__.split(".")[0] == "torch":
        import torch
        t = frames
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError("frames must be an (n, H, W) uint8 tensor")
        if not t.is_cuda:
            return _frames(t.numpy())
        n, h, w = t.shape
        if t.stride(2) != 1 or t.stride(1) < w or (n > 1 and t.stride(0) < t.stride(1) * h):
            t = t.contiguous()
        torch.cuda.current_stream(t.device).synchronize()   # the tracker reads on its own streams
        return t.data_ptr(), n, h, w, t.stride(1), t.stride(0), t
    a = np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("frames must be an (n, H, W) uint8 array")
    n, h, w = a.shape
    s0, s1, s2 = a.strides
    if s2 != 1 or s1 < w or (n > 1 and s0 < s1 * h):
        a = np.ascontiguousarray(a)
        s0, s1 = a.strides[:2]
    return a.ctypes.data, n, h, w, s1, s0, a


def _check(problem, rc):
    if rc:
        raise RsSyncError(problem._lib.rssync_last_error().decode())


def _lib_of(problem):
    return product_only(problem, library(), "the tracker")


def track_points(problem, frames, grid_step=200, **kw):
    """-> points_a (P, 2), points_b (n-1, P, 2), status (n-1, P) uint8, residual (n-1, P) float32"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    prm = params(grid_step, **kw)
    step = grid_step or DEFAULTS["grid_step"]   # (0 = the default, as in the C struct; < 0 is the library's error)
    P = len(range(step, w, step)) * len(range(step, h, step)) if step > 0 else 0
    pa = np.zeros((max(P, 1), 2))
    pb = np.zeros((max(n - 1, 1), max(P, 1), 2))
    st = np.zeros((max(n - 1, 1), max(P, 1)), np.uint8)
    res = np.zeros((max(n - 1, 1), max(P, 1)), np.float32)
    got = C.c_size_t()
    _check(problem, lib.rssync_track_points(problem._h, ptr, n, w, h, pitch, fstride, C.byref(prm),
                                            pa.ctypes.data_as(_PD), pb.ctypes.data_as(_PD), st.ctypes.data,
                                            res.ctypes.data_as(C.POINTER(C.c_float)), P, C.byref(got)))
    del keep
    return pa[:P], pb[:n - 1, :P], st[:n - 1, :P], res[:n - 1, :P]


def track_frames(problem, frames, frame_times, lens, first_frame=0, grid_step=200, **kw):
    """track, then set_track_pixels(first_frame + k, t[k], t[k+1], grid, b_k, lens, H) for every pair k"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = np.ascontiguousarray(frame_times, np.float64)
    if t.shape != (n,):
        raise ValueError("frame_times must hold one time per frame")
    L = np.ascontiguousarray(lens, np.float64)
    if L.shape != (9,):
        raise ValueError("lens = (ro, fx, fy, cx, cy, k1, k2, k3, k4)")
    prm = params(grid_step, **kw)
    _check(problem, lib.rssync_track_frames(problem._h, ptr, n, w, h, pitch, fstride, t.ctypes.data_as(_PD),
                                            int(first_frame), L.ctypes.data, C.byref(prm)))
    del keep


def pyramid(problem, frames, levels=4):
    """the device pyramid, levels 1 .. levels-1: a list of (n, h_l, w_l) float32 arrays (tests)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    sizes, (lw, lh) = [], (w, h)
    for _ in range(1, levels):
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
        sizes.append((lh, lw))
    out = np.zeros((n, max(sum(a * b for a, b in sizes), 1)), np.float32)
    cfg = _Cfg(w, h, 200, 21, levels, 30, 0.01, 1e-4)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_track_pyramid(ctx, ptr, n, pitch, fstride, C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep
    res, at = [], 0
    for lh, lw in sizes:
        res.append(out[:, at:at + lh * lw].reshape(n, lh, lw))
        at += lh * lw
    return res

