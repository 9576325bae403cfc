"""Grayscale frames stabilised on the GPU along a smoothed gyro path (include/rssync_stabilize.h).

With the gyro data installed and the delay found, ``stabilize_frames`` renders every frame as a global-shutter camera
would have seen it at a target orientation that is not the frame's own: the Gaussian-smoothed path (``sigma``), or the
orientations the caller brings (``targets``); the output camera may have another size, be a plain pinhole, and carry a
``zoom``.  ``stabilize_path`` returns the smoothed orientations, ``stabilize_map`` the source position of every output
pixel, ``stabilize_coverage`` the number of output border pixels that see past the frame for a grid of zooms, and
``stabilize_zoom`` the smallest zoom of that grid that keeps the borders out of every frame
(csrc/kernels/stabilize.hpp).

``frames`` is an ``(n, H, W)`` uint8 array: numpy (pitched views included) or a uint8 torch tensor on the problem's
device; the result is ``(n, out_height, out_width)`` of the same kind, or written into ``out``.

Its own ctypes table, bound to the product library only: the stabiliser has no CPU test double.
"""
import ctypes as C

import numpy as np

from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _is_torch, _lens, _out_like, _out_view
from .track import _frames

_PD = C.POINTER(C.c_double)
_SZ = C.c_size_t

CAMERA_LENS, CAMERA_PINHOLE = 0, 1
FILTER_BILINEAR, FILTER_BICUBIC = 0, 1
DEFAULT_ITERATIONS = 3


class StabilizeParams(C.Structure):
    """rssync_stabilize_params: zeros = the defaults"""
    _fields_ = [("sigma", C.c_double), ("zoom", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("camera", C.c_int32), ("iterations", C.c_int32), ("fill", C.c_int32), ("filter", C.c_int32)]


class _Cfg(C.Structure):
    """rship_stabilize_cfg (csrc/stabilize_hip.h), for the tests' call of the internal launcher with a chunk budget"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("out_width", C.c_uint32), ("out_height", C.c_uint32),
                ("lens", C.c_double * 9), ("cam", C.c_double * 4), ("start", C.c_double), ("fs", C.c_double), ("n_knots", C.c_uint32),
                ("delay", C.c_double), ("sigma", C.c_double), ("camera", C.c_int32), ("iterations", C.c_int32), ("fill", C.c_int32),
                ("filter", C.c_int32)]


_PP = C.POINTER(StabilizeParams)
_PU64 = C.POINTER(C.c_uint64)

# name -> (restype, argtypes): every function include/rssync_stabilize.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_stabilize_path": (C.c_int, [C.c_void_p, _PD, _SZ, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "rssync_stabilize_map": (C.c_int, [C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _SZ, C.c_double, C.c_double, _PD, _PP, C.c_void_p]),
    "rssync_stabilize_frames": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double, _PD, _PP,
                                          C.c_void_p, _SZ, _SZ, _SZ, _SZ, _PU64]),
    "rssync_stabilize_coverage": (C.c_int, [C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _SZ, _PD, _SZ, C.c_double, _PD, _PP, _PD, _SZ,
                                            C.POINTER(C.c_uint32)]),
    "rship_stabilize_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, _PD, _PD, C.POINTER(_Cfg), C.c_void_p, _SZ, _SZ,
                                         _PU64, _SZ]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with the stabiliser's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the stabiliser")


def params(sigma=0.0, zoom=1.0, camera=CAMERA_LENS, out_camera=None, iterations=DEFAULT_ITERATIONS, fill=0, filter=FILTER_BILINEAR):
    """out_camera: None = the lens's, scaled to the output; else (fx, fy, cx, cy).  filter: FILTER_BILINEAR or
    FILTER_BICUBIC (Catmull-Rom over 4 x 4 taps: sharper, sixteen taps a pixel).  Everything is handed on as written."""
    fx, fy, cx, cy = (0.0, 0.0, 0.0, 0.0) if out_camera is None else (float(v) for v in out_camera)
    return StabilizeParams(float(sigma), float(zoom), fx, fy, cx, cy, int(camera), int(iterations), int(fill), int(filter))


def _targets(targets, n):
    """-> (pointer or None, keep-alive) of n x 4 float64 orientations"""
    if targets is None:
        return None, None
    t = np.ascontiguousarray(targets, np.float64)
    if t.shape != (n, 4):
        raise ValueError("targets must hold one quaternion (w, x, y, z) per frame")
    return t.ctypes.data_as(_PD), t


def _times(frame_times, n=None):
    t = np.ascontiguousarray(frame_times, np.float64)
    if t.ndim != 1 or (n is not None and t.shape != (n,)):
        raise ValueError("frame_times must hold one time per frame")
    return t


def _launcher_cfg(problem, w, h, ow, oh, lens, delay, sigma, camera, iterations, fill, filter, zoom=1.0, cam=None):
    """rship_stabilize_cfg for the *_budget calls of the internal launchers.  cam: None = the lens's camera scaled to the
    output, its focal lengths times `zoom` (1: a launcher that multiplies by a zoom per frame itself)"""
    fs, start, n_knots = problem.gyro_info()
    if cam is None:
        sx, sy = ow / w, oh / h
        cam = (lens[1] * sx * float(zoom), lens[2] * sy * float(zoom), lens[3] * sx, lens[4] * sy)
    return _Cfg(w, h, ow, oh, (C.c_double * 9)(*lens), (C.c_double * 4)(*cam), start, fs, n_knots, float(delay), float(sigma), int(camera),
                int(iterations), int(fill), int(filter))


def stabilize_path(problem, frame_times, ro, delay, sigma, out=None):
    """-> (n, 4) float64 unit quaternions (w, x, y, z): the Gaussian-smoothed orientation at every frame's centre time.
    out: a contiguous (n, 4) float64 numpy array or tensor on the problem's device to be written instead."""
    lib = _lib_of(problem)
    t = _times(frame_times)
    n = t.shape[0]
    res = np.zeros((n, 4), np.float64) if out is None else out
    if _is_torch(res) and res.is_cuda:
        import torch
        if res.dtype != torch.float64 or tuple(res.shape) != (n, 4) or not res.is_contiguous():
            raise ValueError("out must be a contiguous (n, 4) float64 tensor")
        torch.cuda.current_stream(res.device).synchronize()
        ptr = res.data_ptr()
    else:
        if not isinstance(res, np.ndarray) or res.dtype != np.float64 or res.shape != (n, 4) or not res.flags.c_contiguous:
            raise ValueError("out must be a contiguous (n, 4) float64 array")
        ptr = res.ctypes.data
    _check(problem, lib.rssync_stabilize_path(problem._h, t.ctypes.data_as(_PD), n, float(ro), float(delay), float(sigma), ptr))
    return res


def stabilize_map(problem, width, height, lens, frame_time, delay, target=None, out_size=None, **kw):
    """-> (out_height, out_width, 2) float32: the source position (x, y) in the input frame of every output pixel.
    target: (w, x, y, z), or None = the path at sigma.  out_size: (out_width, out_height), None = the input's.
    kw: sigma, zoom, camera, out_camera, iterations (and filter, which is checked and changes nothing)."""
    lib = _lib_of(problem)
    L = _lens(lens)
    ow, oh = (int(width), int(height)) if out_size is None else (int(out_size[0]), int(out_size[1]))
    out = np.zeros((oh, ow, 2), np.float32)
    prm = params(**kw)
    tptr, tkeep = _targets(None if target is None else np.asarray(target, np.float64).reshape(1, 4), 1)
    _check(problem, lib.rssync_stabilize_map(problem._h, int(width), int(height), L.ctypes.data, ow, oh, float(frame_time),
                                             float(delay), tptr, C.byref(prm), out.ctypes.data))
    del tkeep
    return out


def stabilize_frames(problem, frames, frame_times, lens, delay, targets=None, out_size=None, out=None, **kw):
    """-> (stabilised frames (n, out_height, out_width) uint8 -- `out` if given, else of the kind of `frames` --,
    n_outside (n,) uint64).  kw: sigma, zoom, camera, out_camera, iterations, fill, filter."""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    res = _out_like(frames, n, oh, ow) if out is None else out
    optr, opitch, ostride, okeep = _out_view(res, n, oh, ow)
    prm = params(**kw)
    tptr, tkeep = _targets(targets, n)
    outside = np.zeros(max(n, 1), np.uint64)
    _check(problem, lib.rssync_stabilize_frames(problem._h, ptr, n, w, h, pitch, fstride, t.ctypes.data_as(_PD), L.ctypes.data,
                                                float(delay), tptr, C.byref(prm), optr, ow, oh, opitch, ostride,
                                                outside.ctypes.data_as(_PU64)))
    del keep, okeep, tkeep
    return res, outside[:n]


def stabilize_coverage(problem, width, height, lens, frame_times, delay, zooms, targets=None, out_size=None, **kw):
    """-> (n_frames, n_zooms) uint32: the output's border pixels whose source is outside the frame, per frame and zoom.
    kw: sigma, camera, out_camera, iterations (zoom is replaced by every entry of `zooms`)."""
    lib = _lib_of(problem)
    L = _lens(lens)
    t = _times(frame_times)
    n = t.shape[0]
    z = np.ascontiguousarray(zooms, np.float64)
    if z.ndim != 1:
        raise ValueError("zooms must be a list of zooms")
    ow, oh = (int(width), int(height)) if out_size is None else (int(out_size[0]), int(out_size[1]))
    prm = params(**kw)
    tptr, tkeep = _targets(targets, n)
    out = np.zeros((n, z.shape[0]), np.uint32)
    _check(problem, lib.rssync_stabilize_coverage(problem._h, int(width), int(height), L.ctypes.data, ow, oh, t.ctypes.data_as(_PD), n,
                                                  float(delay), tptr, C.byref(prm), z.ctypes.data_as(_PD), z.shape[0],
                                                  out.ctypes.data_as(C.POINTER(C.c_uint32))))
    del tkeep
    return out


def stabilize_zoom(problem, width, height, lens, frame_times, delay, zooms, **kw):
    """-> the smallest zoom of `zooms` whose border count is 0 in every frame, None if there is none"""
    counts = stabilize_coverage(problem, width, height, lens, frame_times, delay, zooms, **kw)
    ok = sorted(float(z) for z, clear in zip(np.asarray(zooms, np.float64), (counts == 0).all(axis=0)) if clear)
    return ok[0] if ok else None


def stabilize_frames_budget(problem, frames, frame_times, lens, delay, budget_bytes, out_size=None, sigma=0.0,
                            iterations=DEFAULT_ITERATIONS, fill=0, filter=FILTER_BILINEAR):
    """stabilize_frames along the path through the internal launcher with its device budget for the chunk slots given
    (tests: small frames that span several chunks).  LENS camera, zoom 1.  numpy frames -> (frames, n_outside)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, w, h, ow, oh, L, delay, sigma, CAMERA_LENS, iterations, fill, filter)
    out = np.empty((n, oh, ow), np.uint8)
    outside = np.zeros(max(n, 1), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_stabilize_frames(ctx, ptr, n, pitch, fstride, t.ctypes.data_as(_PD), None, C.byref(cfg), out.ctypes.data, ow, ow * oh,
                                  outside.ctypes.data_as(_PU64), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep
    return out, outside[:n]
