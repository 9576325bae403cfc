"""The stabiliser's dynamic zoom (include/rssync_zoom.h): one zoom per frame instead of one per clip.

``fit_zoom`` finds, on the GPU, the smallest zoom of every frame that keeps the output's borders inside the frame (a
bisection between ``lo`` and ``hi`` that runs in one kernel, csrc/kernels/zoom.hpp); ``smooth_zooms`` turns that curve
into an envelope that never undercuts a frame, so the crop does not pump; ``stabilize_frames_zoomed`` renders every frame
at its own zoom, byte for byte what ``stabilize_frames(zoom=...)`` gives for that frame alone.  ``dynamic_zoom`` is the fit
followed by the envelope.

Frames and results are those of ``stabilize_frames``: ``(n, H, W)`` uint8 numpy arrays (pitched views included) or
tensors on the problem's device.  Grayscale only; the fitted zooms do not depend on the pixel format.

Its own ctypes table, bound to the product library only, like rssync_amd.stabilize.
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
_PU32 = C.POINTER(C.c_uint32)
_PU64 = C.POINTER(C.c_uint64)
_SZ = C.c_size_t

ZOOM_CLEAR, ZOOM_NOT_CLEAR = 0, 1
DEFAULT_STEPS = 12

# name -> (restype, argtypes): every function include/rssync_zoom.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_zoom_fit": (C.c_int, [C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _SZ, _PD, _SZ, C.c_double, _PD, _PP, C.c_double, C.c_double,
                                  C.c_int32, _PD, _PU32]),
    "rssync_zoom_smooth": (C.c_int, [C.c_void_p, _PD, _PD, _SZ, C.c_double, _PD]),
    "rssync_zoom_stabilize": (C.c_int, [C.c_void_p, C.c_void_p, _SZ, _SZ, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double, _PD, _PP,
                                        C.c_void_p, _SZ, _SZ, _SZ, _SZ, _PU64, _PD]),
    "rship_zoom_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _SZ, _SZ, _PD, _PD, C.POINTER(_Cfg), _PD, C.c_void_p, _SZ, _SZ,
                                    _PU64, _SZ]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with the dynamic zoom's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the dynamic zoom")


def _zooms(zooms, n):
    z = np.ascontiguousarray(zooms, np.float64)
    if z.shape != (n,):
        raise ValueError("zooms must hold one zoom per frame")
    return z


def fit_zoom(problem, width, height, lens, frame_times, delay, lo, hi, steps=0, targets=None, out_size=None, **kw):
    """-> (zooms (n,) float64, status (n,) uint32): per frame the smallest zoom in [lo, hi] at which no border pixel of the
    output sees past the frame, by `steps` bisection steps (0 = 12) on the device; status ZOOM_NOT_CLEAR where even `hi`
    does not clear the frame (its zoom is `hi` then).  kw: sigma, camera, out_camera, iterations."""
    lib = _lib_of(problem)
    L = _lens(lens)
    t = _times(frame_times)
    n = t.shape[0]
    ow, oh = (int(width), int(height)) if out_size is None else (int(out_size[0]), int(out_size[1]))
    prm = params(**kw)
    tptr, tkeep = _targets(targets, n)
    zooms = np.zeros(n, np.float64)
    status = np.zeros(n, np.uint32)
    _check(problem, lib.rssync_zoom_fit(problem._h, int(width), int(height), L.ctypes.data, ow, oh, t.ctypes.data_as(_PD), n, float(delay),
                                        tptr, C.byref(prm), float(lo), float(hi), int(steps), zooms.ctypes.data_as(_PD),
                                        status.ctypes.data_as(_PU32)))
    del tkeep
    return zooms, status


def smooth_zooms(problem, frame_times, zooms, window):
    """-> (n,) float64: the envelope of `zooms` over `window` seconds (include/rssync_zoom.h): a Gaussian average of the
    running maximum, never below `zooms`; window 0 copies them.  Host arithmetic."""
    lib = _lib_of(problem)
    t = _times(frame_times)
    z = _zooms(zooms, t.shape[0])
    out = np.zeros(t.shape[0], np.float64)
    _check(problem, lib.rssync_zoom_smooth(problem._h, t.ctypes.data_as(_PD), z.ctypes.data_as(_PD), t.shape[0], float(window),
                                           out.ctypes.data_as(_PD)))
    return out


def dynamic_zoom(problem, width, height, lens, frame_times, delay, lo, hi, window, steps=0, targets=None, out_size=None, **kw):
    """-> (n,) float64: fit_zoom followed by smooth_zooms.  Raises where a frame is not clear at `hi`."""
    zooms, status = fit_zoom(problem, width, height, lens, frame_times, delay, lo, hi, steps=steps, targets=targets, out_size=out_size, **kw)
    if status.any():
        raise RsSyncError("dynamic zoom: frames %s are not clear at the largest zoom %g" % (np.flatnonzero(status).tolist(), hi))
    return smooth_zooms(problem, frame_times, zooms, window)


def stabilize_frames_zoomed(problem, frames, frame_times, lens, delay, zooms, targets=None, out_size=None, out=None, **kw):
    """stabilize_frames with zooms[f] for frame f -> (stabilised frames (n, out_height, out_width) uint8 -- `out` if given,
    else of the kind of `frames` --, n_outside (n,) uint64).  kw: sigma, camera, out_camera, iterations, fill, filter."""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = _times(frame_times, n)
    z = _zooms(zooms, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    res = _out_like(frames, n, oh, ow) if out is None else out
    optr, opitch, ostride, okeep = _out_view(res, n, oh, ow)
    prm = params(**kw)
    tptr, tkeep = _targets(targets, n)
    outside = np.zeros(max(n, 1), np.uint64)
    _check(problem, lib.rssync_zoom_stabilize(problem._h, ptr, n, w, h, pitch, fstride, t.ctypes.data_as(_PD), L.ctypes.data, float(delay),
                                              tptr, C.byref(prm), optr, ow, oh, opitch, ostride, outside.ctypes.data_as(_PU64),
                                              z.ctypes.data_as(_PD)))
    del keep, okeep, tkeep
    return res, outside[:n]


def stabilize_frames_zoomed_budget(problem, frames, frame_times, lens, delay, zooms, budget_bytes, out_size=None, sigma=0.0,
                                   camera=CAMERA_LENS, iterations=DEFAULT_ITERATIONS, fill=0, filter=FILTER_BILINEAR):
    """stabilize_frames_zoomed along the path through the internal launcher with its device budget for the chunk slots
    given (tests: small frames that span several chunks).  numpy frames -> (frames, n_outside)"""
    lib = _lib_of(problem)
    ptr, n, h, w, pitch, fstride, keep = _frames(frames)
    t = _times(frame_times, n)
    z = _zooms(zooms, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, w, h, ow, oh, L, delay, sigma, camera, iterations, fill, filter)     # (at zoom 1: the launcher multiplies)
    out = np.empty((n, oh, ow), np.uint8)
    outside = np.zeros(max(n, 1), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_zoom_frames(ctx, ptr, n, pitch, fstride, t.ctypes.data_as(_PD), None, C.byref(cfg), z.ctypes.data_as(_PD), out.ctypes.data,
                             ow, ow * oh, outside.ctypes.data_as(_PU64), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep
    return out, outside[:n]
