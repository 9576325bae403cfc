"""The borders of colour video filled from neighbouring frames (include/rssync_colorinfill.h): the infill of
rssync_amd.infill for every format of rssync_amd.color.

``stabilize_color_infilled`` is ``stabilize_color`` with a ``radius``: every plane is a camera of its own and runs the gray
infill's procedure -- a sample whose source lies outside its own frame's plane is looked up in that plane of the frames
f - 1, f + 1, .., f - radius, f + radius of the call, rendered at frame f's target, and takes the first one that sees it
(csrc/kernels/colorinfill.hpp).  Donors are chosen per sample and per plane; U and V share one, and so do the four channels
of RGBA32.  Only what no candidate sees gets the plane's fill.

Frames and results are those of ``stabilize_color``.

Its own ctypes table, bound to the product library only, like rssync_amd.colorzoom.
"""
import ctypes as C

import numpy as np

from .color import CHROMA_CENTER, ColorImage, ColorParams, _Cfg, _as_planes, _image, _launcher_cfg, _out_like, _size, params
from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _lens
from .stabilize import CAMERA_LENS, DEFAULT_ITERATIONS, FILTER_BILINEAR, _targets, _times

_PD = C.POINTER(C.c_double)
_PI = C.POINTER(ColorImage)
_PP = C.POINTER(ColorParams)
_PU64 = C.POINTER(C.c_uint64)
_SZ = C.c_size_t

# name -> (restype, argtypes): the function include/rssync_colorinfill.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_colorinfill_stabilize": (C.c_int, [C.c_void_p, C.c_int, _PI, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double, _PD, _PP, _PI, _SZ, _SZ,
                                               _PU64, C.c_int32, _PU64]),
    "rship_colorinfill_frames": (C.c_int, [C.c_void_p, _PI, C.c_uint32, _PD, _PD, C.POINTER(_Cfg), _PI, _PU64, C.c_int32, _PU64, _SZ]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with the colour infill's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the colour infill")


def _counts(given, n, name):
    """an (n, 2) uint64 array of counts: the caller's, or a new one"""
    if given is None:
        return np.zeros((max(n, 1), 2), np.uint64)
    if not (isinstance(given, np.ndarray) and given.dtype == np.uint64 and given.shape == (n, 2) and given.flags.c_contiguous
            and given.flags.writeable):
        raise ValueError("%s must be a writable C-contiguous uint64 array of the shape (%d, 2)" % (name, n))
    return given


def stabilize_color_infilled(problem, fmt, frames, frame_times, lens, delay, radius, targets=None, out_size=None, out=None,
                             n_borrowed=None, chroma_site=CHROMA_CENTER, fills=None, **kw):
    """stabilize_color with the borders taken from up to `radius` (0 .. 8) frames on each side -> (stabilised frames in the
    layout of `frames` -- `out` if given --, n_outside (n, 2) uint64: the samples of plane 0 and the chroma samples that still
    got the fill, n_borrowed (n, 2) uint64 -- the array `n_borrowed` if given --: those taken from another frame).
    kw: sigma, zoom, camera, out_camera, iterations, fill, filter."""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(fmt, planes)
    borrowed = _counts(n_borrowed, n, "n_borrowed")
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    res = _out_like(fmt, planes, n, oh, ow) if out is None else _as_planes(fmt, out)
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    prm = params(chroma_site, fills, **kw)
    tptr, tkeep = _targets(targets, n)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    _check(problem, lib.rssync_colorinfill_stabilize(problem._h, int(fmt), C.byref(src), n, w, h, t.ctypes.data_as(_PD), L.ctypes.data,
                                                     float(delay), tptr, C.byref(prm), C.byref(dst), ow, oh, outside.ctypes.data_as(_PU64),
                                                     int(radius), borrowed.ctypes.data_as(_PU64)))
    del keep, okeep, tkeep
    if out is not None:
        return out, outside[:n], borrowed[:n]
    return (res[0] if len(res) == 1 else tuple(res)), outside[:n], borrowed[:n]


def stabilize_color_infilled_budget(problem, fmt, frames, frame_times, lens, delay, radius, budget_bytes, targets=None, out_size=None,
                                    out=None, sigma=0.0, zoom=1.0, chroma_site=CHROMA_CENTER, camera=CAMERA_LENS,
                                    iterations=DEFAULT_ITERATIONS, fills=None, filter=FILTER_BILINEAR):
    """stabilize_color_infilled through the internal launcher with its device budget for the chunk slots given (tests: small
    frames that span several chunks, halos that cross chunk edges).  fills: None = the header's defaults for fill 0; targets:
    normalised here as the library normalises them.  -> (planes, n_outside (n, 2), n_borrowed (n, 2))"""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(fmt, planes)
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, fmt, w, h, ow, oh, L, delay, sigma, chroma_site, camera, iterations, fills, filter, zoom=zoom)
    if targets is not None:             # (rs::limit_unit's operations in its order: the launcher takes unit quaternions)
        q = np.array(targets, np.float64)
        targets = q / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    tptr, tkeep = _targets(targets, n)
    res = _out_like(fmt, planes, n, oh, ow) if out is None else _as_planes(fmt, out)
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    borrowed = np.zeros((max(n, 1), 2), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_colorinfill_frames(ctx, C.byref(src), n, t.ctypes.data_as(_PD), tptr, C.byref(cfg), C.byref(dst),
                                    outside.ctypes.data_as(_PU64), int(radius), borrowed.ctypes.data_as(_PU64), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep, okeep, tkeep
    if out is not None:
        return out, outside[:n], borrowed[:n]
    return (res[0] if len(res) == 1 else tuple(res)), outside[:n], borrowed[:n]
