"""The stabiliser's borders filled from neighbouring frames (include/rssync_infill.h).

``stabilize_frames_infilled`` is ``stabilize_frames`` with a ``radius``: an output pixel whose source lies outside its own
frame is looked up in the frames f - 1, f + 1, .., f - radius, f + radius of the call, rendered at frame f's target, and
takes the first one that sees it (csrc/kernels/infill.hpp); only what no candidate sees gets ``fill``.  The zoom and the
smoothing stay as they are: the third answer to a border beside ``fit_zoom`` and ``fit_strength``.

Frames and results are those of ``stabilize_frames``: ``(n, H, W)`` uint8 numpy arrays (pitched views included) or
tensors on the problem's device.  Grayscale only.

Its own ctypes table, bound to the product library only, like rssync_amd.zoom.
"""
import ctypes as C

import numpy as np

from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _lens, _out_like, _out_view
from .stabilize import (CAMERA_LENS, DEFAULT_ITERATIONS, FILTER_BILINEAR, StabilizeParams, _Cfg, _launcher_cfg, _targets, _times,
                        params)
from .track import _frames

_PD = C.POINTER(C.c_double)
_PP = C.POINTER(StabilizeParams)
_PU64 = C.POINTER(C.c_uint64)
_SZ = C.c_size_t

# name -> (restype, argtypes): the function include/rssync_infill.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_infill_stabilize": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double, _PD, _PP,
                                          C.c_void_p, _SZ, _SZ, _SZ, _SZ, _PU64, C.c_int32, _PU64]),
    "rship_infill_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, _PD, _PD, C.POINTER(_Cfg), C.c_void_p, _SZ, _SZ,
                                      _PU64, C.c_int32, _PU64, _SZ]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with the infill's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the infill")


def candidates(f, n_frames, radius):
    """-> the frames asked for a pixel of frame f, in order: f, f - 1, f + 1, .., those outside 0 .. n_frames - 1 skipped"""
    steps = [f] + [g for d in range(1, radius + 1) for g in (f - d, f + d)]
    return [g for g in steps if 0 <= g < n_frames]


def stabilize_frames_infilled(problem, frames, frame_times, lens, delay, radius, targets=None, out_size=None, out=None, **kw):
    """stabilize_frames with the borders taken from up to `radius` (0 .. 8) frames on each side -> (stabilised frames
    (n, out_height, out_width) uint8 -- `out` if given, else of the kind of `frames` --, n_outside (n,) uint64: the pixels
    that still got `fill`, n_borrowed (n,) uint64: the pixels taken from another frame).  kw: sigma, zoom, camera,
    out_camera, iterations, fill, filter."""
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
    borrowed = np.zeros(max(n, 1), np.uint64)
    _check(problem, lib.rssync_infill_stabilize(problem._h, ptr, n, w, h, pitch, fstride, t.ctypes.data_as(_PD), L.ctypes.data, float(delay),
                                                tptr, C.byref(prm), optr, ow, oh, opitch, ostride, outside.ctypes.data_as(_PU64),
                                                int(radius), borrowed.ctypes.data_as(_PU64)))
    del keep, okeep, tkeep
    return res, outside[:n], borrowed[:n]


def stabilize_frames_infilled_budget(problem, frames, frame_times, lens, delay, radius, budget_bytes, targets=None, out_size=None,
                                     sigma=0.0, zoom=1.0, camera=CAMERA_LENS, iterations=DEFAULT_ITERATIONS, fill=0,
                                     filter=FILTER_BILINEAR):
    """stabilize_frames_infilled through the internal launcher with its device budget for the chunk slots given (tests:
    small frames that span several chunks, halos that cross chunk edges).  targets: normalised here as the library normalises
    them.  numpy frames -> (frames, n_outside, n_borrowed)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, w, h, ow, oh, L, delay, sigma, camera, iterations, fill, filter, zoom=zoom)
    if targets is not None:             # (rs::limit_unit's operations in its order: the launcher takes unit quaternions)
        q = np.array(targets, np.float64)
        targets = q / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    tptr, tkeep = _targets(targets, n)
    out = np.empty((n, oh, ow), np.uint8)
    outside = np.zeros(max(n, 1), np.uint64)
    borrowed = np.zeros(max(n, 1), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_infill_frames(ctx, ptr, n, pitch, fstride, t.ctypes.data_as(_PD), tptr, C.byref(cfg), out.ctypes.data, ow, ow * oh,
                               outside.ctypes.data_as(_PU64), int(radius), borrowed.ctypes.data_as(_PU64), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep, tkeep
    return out, outside[:n], borrowed[:n]
