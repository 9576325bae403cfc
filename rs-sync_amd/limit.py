"""The path limited to a zoom (include/rssync_limit.h): the opposite of rssync_amd.zoom.

Given the zoom the caller is willing to pay, ``fit_strength`` finds, on the GPU, how far every frame may follow its goal --
the smoothed path or the caller's ``targets`` -- without a border pixel of the output seeing past the frame: a strength
in [0, 1] between the frame's own orientation (0, no smoothing) and the goal (1), by a bisection that runs in one kernel
and rebuilds the frame's row table for every candidate (csrc/kernels/limit.hpp).  ``smooth_strengths`` turns that curve
into a lower envelope, so the smoothing does not pump; ``limited_targets`` is fit, envelope and the resulting targets,
which every renderer of the package takes as ``targets``: ``stabilize_frames``, ``stabilize_frames_zoomed``,
``stabilize_color``, ``stabilize_color_zoomed``, with either filter.

A frame is guaranteed clear only at its fitted strength; below it wherever "clear" is monotone in the strength, which it
was on every frame tried.  ``limited_targets(verify=True)`` checks the result with one coverage call.

Its own ctypes table, bound to the product library only, like rssync_amd.zoom.
"""
import ctypes as C

import numpy as np

from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _lens
from .stabilize import StabilizeParams, _targets, _times, params, stabilize_coverage

_PD = C.POINTER(C.c_double)
_PP = C.POINTER(StabilizeParams)
_PU32 = C.POINTER(C.c_uint32)
_SZ = C.c_size_t

LIMIT_CLEAR, LIMIT_NOT_CLEAR = 0, 1
DEFAULT_STEPS = 12

# name -> (restype, argtypes): every function include/rssync_limit.h declares
SIGNATURES = {
    "rssync_limit_fit": (C.c_int, [C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _SZ, _PD, _SZ, C.c_double, _PD, _PP, _PD, C.c_int32, _PD, _PU32]),
    "rssync_limit_smooth": (C.c_int, [C.c_void_p, _PD, _PD, _SZ, C.c_double, _PD]),
    "rssync_limit_targets": (C.c_int, [C.c_void_p, _PD, _SZ, C.c_double, C.c_double, _PD, C.c_double, _PD, _PD]),
}


def library():
    """the product library with the limiter's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the path limiter")


def _per_frame(values, n, what):
    v = np.ascontiguousarray(values, np.float64)
    if v.shape != (n,):
        raise ValueError("%s must hold one value per frame" % what)
    return v


def fit_strength(problem, width, height, lens, frame_times, delay, zoom=1.0, zooms=None, steps=0, targets=None, out_size=None, **kw):
    """-> (strengths (n,) float64, status (n,) uint32): per frame the largest strength in [0, 1] the bisection finds at
    which no border pixel of the output sees past the frame, at `zoom` or at zooms[f]; `steps` bisection steps (0 = 12) on
    the device.  Strength 1 where the goal itself is clear; status LIMIT_NOT_CLEAR (and strength 0) where the frame shows
    a border even without smoothing.  kw: sigma, camera, out_camera, iterations."""
    lib = _lib_of(problem)
    L = _lens(lens)
    t = _times(frame_times)
    n = t.shape[0]
    ow, oh = (int(width), int(height)) if out_size is None else (int(out_size[0]), int(out_size[1]))
    prm = params(zoom=zoom, **kw)
    tptr, tkeep = _targets(targets, n)
    z = None if zooms is None else _per_frame(zooms, n, "zooms")
    strengths = np.zeros(n, np.float64)
    status = np.zeros(n, np.uint32)
    _check(problem, lib.rssync_limit_fit(problem._h, int(width), int(height), L.ctypes.data, ow, oh, t.ctypes.data_as(_PD), n, float(delay),
                                         tptr, C.byref(prm), None if z is None else z.ctypes.data_as(_PD), int(steps),
                                         strengths.ctypes.data_as(_PD), status.ctypes.data_as(_PU32)))
    del tkeep
    return strengths, status


def smooth_strengths(problem, frame_times, strengths, window):
    """-> (n,) float64: the lower envelope of `strengths` over `window` seconds (include/rssync_limit.h): a Gaussian average
    of the running minimum, never above `strengths`; window 0 copies them.  Host arithmetic."""
    lib = _lib_of(problem)
    t = _times(frame_times)
    a = _per_frame(strengths, t.shape[0], "strengths")
    out = np.zeros(t.shape[0], np.float64)
    _check(problem, lib.rssync_limit_smooth(problem._h, t.ctypes.data_as(_PD), a.ctypes.data_as(_PD), t.shape[0], float(window),
                                            out.ctypes.data_as(_PD)))
    return out


def strength_targets(problem, frame_times, ro, delay, strengths, targets=None, sigma=0.0):
    """-> (n, 4) float64: the candidate target of every frame at its strength (rssync_limit_targets): the goal's bits at
    strength 1, the frame's own orientation at 0.  Not normalised: every call that takes `targets` does that."""
    lib = _lib_of(problem)
    t = _times(frame_times)
    n = t.shape[0]
    a = _per_frame(strengths, n, "strengths")
    tptr, tkeep = _targets(targets, n)
    out = np.zeros((n, 4), np.float64)
    _check(problem, lib.rssync_limit_targets(problem._h, t.ctypes.data_as(_PD), n, float(ro), float(delay), tptr, float(sigma),
                                             a.ctypes.data_as(_PD), out.ctypes.data_as(_PD)))
    del tkeep
    return out


def limited_targets(problem, width, height, lens, frame_times, delay, window, zoom=1.0, zooms=None, steps=0, targets=None, out_size=None,
                    verify=False, **kw):
    """-> (targets (n, 4) float64, strengths (n,) float64, status (n,) uint32): fit_strength, smooth_strengths over
    `window` seconds, then the targets at the smoothed strengths, to be passed as `targets` to any renderer together with
    the same zoom.  verify: one stabilize_coverage at the result; raises RsSyncError naming the frames that are not clear
    (those of status LIMIT_NOT_CLEAR among them)."""
    fitted, status = fit_strength(problem, width, height, lens, frame_times, delay, zoom=zoom, zooms=zooms, steps=steps, targets=targets,
                                  out_size=out_size, **kw)
    strengths = smooth_strengths(problem, frame_times, fitted, window)
    L = _lens(lens)
    res = strength_targets(problem, frame_times, float(L[0]), delay, strengths, targets=targets, sigma=kw.get("sigma", 0.0))
    if verify:
        n = res.shape[0]
        cover = {k: v for k, v in kw.items() if k != "sigma"}
        if zooms is None:
            counts = stabilize_coverage(problem, width, height, lens, frame_times, delay, [zoom], targets=res, out_size=out_size, **cover)[:, 0]
        else:
            z = _per_frame(zooms, n, "zooms")
            uniq, inverse = np.unique(z, return_inverse=True)
            counts = stabilize_coverage(problem, width, height, lens, frame_times, delay, uniq, targets=res, out_size=out_size,
                                        **cover)[np.arange(n), inverse]
        if counts.any():
            raise RsSyncError("limited path: frames %s are not clear at their zoom" % np.flatnonzero(counts).tolist())
    return res, strengths, status
