"""Grayscale frames with the rolling-shutter skew removed, on the GPU (include/rssync_rectify.h).

With the gyro data installed and the delay found, ``rectify_frames`` renders every frame as a global-shutter camera with
the same lens would have seen it at the orientation of ``ref_row``'s time (csrc/kernels/rectify.hpp);
``rectify_map`` returns the source position of every output pixel, ``rectify_points`` carries tracked points the other
way, from the rolling-shutter frame into the rectified one.

``frames`` is an ``(n, H, W)`` uint8 array: numpy (pitched views included) or a uint8 torch tensor on the problem's
device; the result is of the same kind, or written into ``out``.

Its own ctypes table, bound to the product library only: the rectifier has no CPU test double.
"""
import ctypes as C

import numpy as np

from .problem import RsSyncError, product_library, product_only
from .track import _frames

_PD = C.POINTER(C.c_double)
_PF = C.POINTER(C.c_float)
_SZ = C.c_size_t


class RectifyParams(C.Structure):
    """rssync_rectify_params: ref_row < 0 and iterations 0 = their defaults"""
    _fields_ = [("ref_row", C.c_double), ("iterations", C.c_int32), ("fill", C.c_int32)]


class _Cfg(C.Structure):
    """rship_rectify_cfg (csrc/rectify_hip.h), for the tests' call of the internal launcher with a chunk budget"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("lens", C.c_double * 9), ("start", C.c_double), ("fs", C.c_double),
                ("n_knots", C.c_uint32), ("delay", C.c_double), ("ref_row", C.c_double), ("iterations", C.c_int32),
                ("fill", C.c_int32)]


# name -> (restype, argtypes): every function include/rssync_rectify.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_rectify_map": (C.c_int, [C.c_void_p, _SZ, _SZ, C.c_void_p, C.c_double, C.c_double, C.POINTER(RectifyParams),
                                     C.c_void_p]),
    "rssync_rectify_frames": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double,
                                        C.POINTER(RectifyParams), C.c_void_p, _SZ, _SZ, C.POINTER(C.c_uint64)]),
    "rssync_rectify_points": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, C.c_void_p, C.c_double, C.c_double,
                                        C.POINTER(RectifyParams), C.c_void_p]),
    "rship_rectify_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, _PD, C.POINTER(_Cfg), C.c_void_p, _SZ, _SZ,
                                       C.POINTER(C.c_uint64), _SZ]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}

DEFAULT_ITERATIONS = 3


def library():
    """the product library with the rectifier's signatures attached"""
    return product_library(SIGNATURES)


def params(ref_row=None, iterations=DEFAULT_ITERATIONS, fill=0):
    """ref_row None = the default (rows / 2); everything else is handed on as written"""
    return RectifyParams(-1.0 if ref_row is None else float(ref_row), int(iterations), int(fill))


def _lens(lens):
    L = np.ascontiguousarray(lens, np.float64)
    if L.shape != (9,):
        raise ValueError("lens = (ro, fx, fy, cx, cy, k1, k2, k3, k4)")
    return L


def _check(problem, rc):
    if rc:
        raise RsSyncError(problem._lib.rssync_last_error().decode())


def _lib_of(problem):
    return product_only(problem, library(), "the rectifier")


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _out_like(frames, n, h, w):
    if _is_torch(frames) and frames.is_cuda:
        import torch
        return torch.empty((n, h, w), dtype=torch.uint8, device=frames.device)
    return np.empty((n, h, w), np.uint8)


def _out_view(out, n, h, w):
    """-> (pointer, pitch, frame_stride, keep-alive) of a writable (n, H, W) uint8 array or device tensor (pitched views
    included: only the pixels are written)"""
    if _is_torch(out) and out.is_cuda:
        import torch
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w) or out.stride(2) != 1 or out.stride(1) < w or \
                (n > 1 and out.stride(0) < out.stride(1) * h):
            raise ValueError("out must be an (n, H, W) uint8 tensor with contiguous rows")
        torch.cuda.current_stream(out.device).synchronize()
        return out.data_ptr(), out.stride(1), out.stride(0), out
    a = out.numpy() if _is_torch(out) else out
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.shape != (n, h, w) or not a.flags.writeable or \
            a.strides[2] != 1 or a.strides[1] < w or (n > 1 and a.strides[0] < a.strides[1] * h):
        raise ValueError("out must be a writable (n, H, W) uint8 array with contiguous rows")
    return a.ctypes.data, a.strides[1], a.strides[0], a


def rectify_frames(problem, frames, frame_times, lens, delay, ref_row=None, iterations=DEFAULT_ITERATIONS, fill=0, out=None):
    """-> (rectified frames (n, H, W) uint8 -- `out` if given, else of the kind of `frames` --, n_outside (n,) uint64)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = np.ascontiguousarray(frame_times, np.float64)
    if t.shape != (n,):
        raise ValueError("frame_times must hold one time per frame")
    L = _lens(lens)
    res = _out_like(frames, n, h, w) if out is None else out
    optr, opitch, ostride, okeep = _out_view(res, n, h, w)
    prm = params(ref_row, iterations, fill)
    outside = np.zeros(max(n, 1), np.uint64)
    _check(problem, lib.rssync_rectify_frames(problem._h, ptr, n, w, h, pitch, fstride, t.ctypes.data_as(_PD), L.ctypes.data,
                                              float(delay), C.byref(prm), optr, opitch, ostride,
                                              outside.ctypes.data_as(C.POINTER(C.c_uint64))))
    del keep, okeep
    return res, outside[:n]


def rectify_map(problem, width, height, lens, frame_time, delay, ref_row=None, iterations=DEFAULT_ITERATIONS):
    """-> (H, W, 2) float32: the source position (x, y) of every output pixel, positions outside the frame included"""
    lib = _lib_of(problem)
    L = _lens(lens)
    out = np.zeros((int(height), int(width), 2), np.float32)
    prm = params(ref_row, iterations, 0)
    _check(problem, lib.rssync_rectify_map(problem._h, int(width), int(height), L.ctypes.data, float(frame_time), float(delay),
                                           C.byref(prm), out.ctypes.data))
    return out


def rectify_points(problem, points, width, height, lens, frame_time, delay, ref_row=None):
    """rolling-shutter positions (..., 2) -> their positions in the rectified frame, float64; a float64 torch tensor on
    the problem's device gives one"""
    lib = _lib_of(problem)
    L = _lens(lens)
    prm = params(ref_row, DEFAULT_ITERATIONS, 0)
    if _is_torch(points) and points.is_cuda:
        import torch
        p = points.to(torch.float64).contiguous()
        if p.shape[-1] != 2:
            raise ValueError("points must be (..., 2)")
        out = torch.empty_like(p)
        torch.cuda.current_stream(p.device).synchronize()
        src, dst, count = p.data_ptr(), out.data_ptr(), p.numel() // 2
    else:
        p = np.ascontiguousarray(points.numpy() if _is_torch(points) else points, np.float64)
        if p.ndim < 1 or p.shape[-1] != 2:
            raise ValueError("points must be (..., 2)")
        out = np.zeros_like(p)
        src, dst, count = p.ctypes.data, out.ctypes.data, p.size // 2
    _check(problem, lib.rssync_rectify_points(problem._h, src, count, int(width), int(height), L.ctypes.data, float(frame_time),
                                              float(delay), C.byref(prm), dst))
    return out


def rectify_frames_budget(problem, frames, frame_times, lens, delay, budget_bytes, ref_row=None, iterations=DEFAULT_ITERATIONS,
                          fill=0):
    """rectify_frames through the internal launcher with its device budget for the chunk slots given (tests: small frames
    that span several chunks).  numpy frames -> (frames, n_outside)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = np.ascontiguousarray(frame_times, np.float64)
    fs, start, n_knots = problem.gyro_info()
    cfg = _Cfg(w, h, (C.c_double * 9)(*_lens(lens)), start, fs, n_knots, float(delay),
               0.5 * h if ref_row is None else float(ref_row), int(iterations), int(fill))
    out = np.empty((n, h, w), np.uint8)
    outside = np.zeros(max(n, 1), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_rectify_frames(ctx, ptr, n, pitch, fstride, t.ctypes.data_as(_PD), C.byref(cfg), out.ctypes.data, w, w * h,
                                outside.ctypes.data_as(C.POINTER(C.c_uint64)), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep
    return out, outside[:n]
