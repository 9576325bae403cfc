"""The borders of 4:2:2 and 4:4:4 video filled from neighbouring frames (include/rssync_infillyuv.h): the infill of
rssync_amd.infill for every format of rssync_amd.yuv, as rssync_amd.colorinfill is for the 4:2:0 family.

``stabilize_yuv_infilled`` is ``stabilize_yuv`` with a ``radius``: every plane is a camera of its own and runs the gray
infill's procedure -- a sample whose source lies outside its own frame's plane is looked up in that plane of the frames
f - 1, f + 1, .., f - radius, f + radius of the call, rendered at frame f's target, and takes the first one that sees it
(csrc/kernels/infillyuv.hpp).  A 4:2:2 luma pixel and the chroma sample over it are decided apart; U and V share one donor;
Y, U and V of a 4:4:4 pixel share one.  Only what no candidate sees gets the plane's fill.

Frames and results are those of ``stabilize_yuv``.

Its own ctypes table, bound to the product library only, like rssync_amd.zoomyuv.
"""
import ctypes as C

import numpy as np

from . import colorinfill as _colorinfill
from .color import CHROMA_CENTER, _PD, _PU64, params
from .colorinfill import _counts
from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _lens
from .stabilize import CAMERA_LENS, DEFAULT_ITERATIONS, FILTER_BILINEAR, _targets, _times
from .stabilize import _launcher_cfg as _stab_launcher_cfg
from .yuv import _as_planes, _image, _launcher_cfg, _out_like, _size, chroma_config, is_422

# name -> (restype, argtypes): the function include/rssync_infillyuv.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_infillyuv_stabilize": _colorinfill.SIGNATURES["rssync_colorinfill_stabilize"],
    "rship_infillyuv_frames": _colorinfill.SIGNATURES["rship_colorinfill_frames"],
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with the 4:2:2 / 4:4:4 infill's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the 4:2:2 / 4:4:4 infill")


def stabilize_yuv_infilled(problem, fmt, frames, frame_times, lens, delay, radius, targets=None, out_size=None, out=None,
                           n_borrowed=None, chroma_site=CHROMA_CENTER, fills=None, **kw):
    """stabilize_yuv with the borders taken from up to `radius` (0 .. 8) frames on each side -> (stabilised planes in the
    layout of `frames` -- `out` if given --, n_outside (n, 2) uint64: the samples of plane 0 and the chroma samples that still
    got the fill, n_borrowed (n, 2) uint64 -- the array `n_borrowed` if given --: those taken from another frame; 4:4:4: the
    same number twice).  kw: sigma, zoom, camera, out_camera, iterations, fill, filter."""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(planes)
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
    _check(problem, lib.rssync_infillyuv_stabilize(problem._h, int(fmt), C.byref(src), n, w, h, t.ctypes.data_as(_PD), L.ctypes.data,
                                                   float(delay), tptr, C.byref(prm), C.byref(dst), ow, oh, outside.ctypes.data_as(_PU64),
                                                   int(radius), borrowed.ctypes.data_as(_PU64)))
    del keep, okeep, tkeep
    if out is not None:
        return out, outside[:n], borrowed[:n]
    return tuple(res), outside[:n], borrowed[:n]


def stabilize_yuv_infilled_budget(problem, fmt, frames, frame_times, lens, delay, radius, budget_bytes, targets=None, out_size=None,
                                  out=None, sigma=0.0, zoom=1.0, chroma_site=CHROMA_CENTER, camera=CAMERA_LENS,
                                  iterations=DEFAULT_ITERATIONS, fills=None, filter=FILTER_BILINEAR):
    """stabilize_yuv_infilled through the internal launcher with its device budget for the chunk slots given (tests: small
    frames that span several chunks, halos that cross chunk edges).  fills: None = the header's defaults for fill 0; targets:
    normalised here as the library normalises them.  -> (planes, n_outside (n, 2), n_borrowed (n, 2))"""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(planes)
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, fmt, w, h, ow, oh, L, delay, sigma, chroma_site, camera, iterations, fills, filter)
    if float(zoom) != 1.0:              # (the one zoom of the call in both planes' output cameras, as color_host.hpp applies it)
        fill, chroma_is_luma = cfg.luma.fill, not is_422(fmt)
        cfg.luma = _stab_launcher_cfg(problem, w, h, ow, oh, L, delay, sigma, camera, iterations, fill, filter, zoom=zoom)
        cfg.chroma = cfg.luma
        if not chroma_is_luma:
            lens_c, cam_c = chroma_config(L, w, h, ow, oh, chroma_site, zoom=float(zoom))
            cfg.chroma = _stab_launcher_cfg(problem, w // 2, h, ow // 2, oh, lens_c, delay, sigma, camera, iterations, fill, filter, cam=cam_c)
    if targets is not None:             # (rs::limit_unit's operations in its order: the launcher takes unit quaternions)
        q = np.array(targets, np.float64)
        targets = q / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    tptr, tkeep = _targets(targets, n)
    res = _out_like(fmt, planes, n, oh, ow) if out is None else _as_planes(fmt, out)
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    borrowed = np.zeros((max(n, 1), 2), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_infillyuv_frames(ctx, C.byref(src), n, t.ctypes.data_as(_PD), tptr, C.byref(cfg), C.byref(dst),
                                  outside.ctypes.data_as(_PU64), int(radius), borrowed.ctypes.data_as(_PU64), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep, okeep, tkeep
    if out is not None:
        return out, outside[:n], borrowed[:n]
    return tuple(res), outside[:n], borrowed[:n]
