"""4:2:2 and 4:4:4 video stabilised on the GPU: I422, NV16 and I444 with 8-bit samples, I210 (yuv422p10le), P210, P216 and
I410 (yuv444p10le) in 16-bit containers (include/rssync_yuv.h).

What ``stabilize_color`` does for the 4:2:0 layouts, every plane of a frame rendered in one pass (csrc/kernels/yuv.hpp).
The luma plane is the stabiliser's result byte for byte.  A 4:2:2 chroma plane is the image of a camera of its own, half as
wide as the luma's and of the same height, whose sample (cu, cv) sits at luma position (2 cu + ox, cv) -- ``chroma_site``
CHROMA_CENTER ox = 0.5, CHROMA_LEFT ox = 0.  The planes of a 4:4:4 frame share the luma's camera.

``frames``, per format (numpy arrays, pitched views included, or torch tensors on the problem's device):

    I422, I210         (Y (n, H, W), U (n, H, W/2), V (n, H, W/2))
    NV16, P210, P216   (Y (n, H, W), UV (n, H, W/2, 2))
    I444, I410         (Y (n, H, W), U (n, H, W), V (n, H, W))

uint8 samples for I422, NV16 and I444, uint16 for the others (torch.uint16 or torch.int16: the bits are taken as unsigned).
P210 keeps a sample's ten bits in the high end of the word (value << 6); I210's and I410's words are the values.

The result is of the same kind and layout with the output's size, or written into ``out``.

Its own ctypes table, bound to the product library only, like the colour front's.
"""
import ctypes as C

import numpy as np

from . import color as _color
from .color import CHROMA_CENTER, CHROMA_LEFT, ColorImage, ColorParams, _Cfg, _PD, _PI, _PP, _PU64, _SZ, params  # noqa: F401
from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _is_torch, _lens
from .stabilize import _launcher_cfg as _stab_launcher_cfg
from .stabilize import _targets, _times, CAMERA_LENS, DEFAULT_ITERATIONS
from .stabilize import FILTER_BILINEAR, FILTER_BICUBIC  # noqa: F401  (re-exported)

I422, NV16, I444 = 32, 33, 34
I210, P210, P216, I410 = 48, 49, 50, 51
SIBLING = {I210: I422, P210: NV16, P216: NV16, I410: I444}       # the 8-bit format with the same planes and geometry
DEPTH = {I210: 10, P210: 10, P216: 16, I410: 10}                 # bits of a sample value
CHROMA_OFFSET = {CHROMA_CENTER: 0.5, CHROMA_LEFT: 0.0}           # ox: 4:2:2 has no vertical offset
_N_PLANES = {I422: 3, NV16: 2, I444: 3, I210: 3, P210: 2, P216: 2, I410: 3}

# name -> (restype, argtypes): every function include/rssync_yuv.h declares, and the internal launcher the tests call
SIGNATURES = {
    "rssync_yuv_stabilize": _color.SIGNATURES["rssync_color_stabilize"],
    "rssync_yuv_map": _color.SIGNATURES["rssync_color_map"],
    "rship_yuv_frames": _color.SIGNATURES["rship_color_frames"],
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with these formats' signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the 4:2:2 / 4:4:4 front")


def is_422(fmt):
    return SIBLING.get(fmt, fmt) in (I422, NV16)


def plane_shapes(fmt, n, h, w):
    """the shapes of a format's planes for n frames of w x h (a 16-bit format's are its sibling's)"""
    fmt = SIBLING.get(fmt, fmt)
    return {I422: [(n, h, w), (n, h, w // 2), (n, h, w // 2)], NV16: [(n, h, w), (n, h, w // 2, 2)],
            I444: [(n, h, w), (n, h, w), (n, h, w)]}[fmt]


def _as_planes(fmt, frames):
    if fmt not in _N_PLANES:
        raise ValueError("format must be I422, NV16, I444, I210, P210, P216 or I410")
    planes = list(frames)
    if len(planes) != _N_PLANES[fmt]:
        raise ValueError("this format has %d planes" % _N_PLANES[fmt])
    return planes


def _image(fmt, planes, n, h, w, writable):
    """-> (ColorImage, keep-alive)"""
    img, keep = ColorImage(), []
    for k, (a, shape) in enumerate(zip(planes, plane_shapes(fmt, n, h, w))):
        if tuple(a.shape) != shape:
            raise ValueError("plane %d must have the shape %s, not %s" % (k, shape, tuple(a.shape)))
        img.plane[k], img.pitch[k], img.stride[k], alive = _color._rows(a, writable, 2 if fmt in SIBLING else 1)
        keep.append(alive)
    return img, keep


def _size(planes):
    y = planes[0]
    if y.ndim != 3:
        raise ValueError("plane 0 must be (n, H, W)")
    return int(y.shape[0]), int(y.shape[1]), int(y.shape[2])


def _out_like(fmt, planes, n, oh, ow):
    y = planes[0]
    if _is_torch(y) and y.is_cuda:
        import torch
        return [torch.empty(s, dtype=torch.uint16 if fmt in SIBLING else torch.uint8, device=y.device) for s in plane_shapes(fmt, n, oh, ow)]
    return [np.empty(s, np.uint16 if fmt in SIBLING else np.uint8) for s in plane_shapes(fmt, n, oh, ow)]


def stabilize_yuv(problem, fmt, frames, frame_times, lens, delay, targets=None, out_size=None, out=None, chroma_site=CHROMA_CENTER,
                  fills=None, **kw):
    """-> (stabilised planes in the layout of `frames` -- `out` if given --, n_outside (n, 2) uint64: filled pixels of plane
    0, filled chroma samples; 4:4:4: the same number twice).  out_size: (out_width, out_height), None = the input's.  kw:
    sigma, zoom, camera, out_camera, iterations, fill, filter."""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(planes)
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    res = _out_like(fmt, planes, n, oh, ow) if out is None else _as_planes(fmt, out)
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    prm = params(chroma_site, fills, **kw)
    tptr, tkeep = _targets(targets, n)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    _check(problem, lib.rssync_yuv_stabilize(problem._h, int(fmt), C.byref(src), n, w, h, t.ctypes.data_as(_PD), L.ctypes.data, float(delay),
                                             tptr, C.byref(prm), C.byref(dst), ow, oh, outside.ctypes.data_as(_PU64)))
    del keep, okeep, tkeep
    if out is not None:
        return out, outside[:n]
    return tuple(res), outside[:n]


def yuv_map(problem, fmt, plane, width, height, lens, frame_time, delay, target=None, out_size=None, chroma_site=CHROMA_CENTER, **kw):
    """-> float32 source positions (x, y) of every output sample of `plane`: (out_height, out_width, 2) for plane 0 and for
    plane 1 of a 4:4:4 format, (out_height, out_width / 2, 2) in chroma-plane coordinates for plane 1 of a 4:2:2 format.
    kw: sigma, zoom, camera, out_camera, iterations."""
    lib = _lib_of(problem)
    L = _lens(lens)
    ow, oh = (int(width), int(height)) if out_size is None else (int(out_size[0]), int(out_size[1]))
    out = np.zeros((oh, ow // 2, 2) if plane and is_422(fmt) else (oh, ow, 2), np.float32)
    prm = params(chroma_site, None, **kw)
    tptr, tkeep = _targets(None if target is None else np.asarray(target, np.float64).reshape(1, 4), 1)
    _check(problem, lib.rssync_yuv_map(problem._h, int(fmt), int(plane), int(width), int(height), L.ctypes.data, ow, oh, float(frame_time),
                                       float(delay), tptr, C.byref(prm), out.ctypes.data))
    del tkeep
    return out


def chroma_config(lens, width, height, out_width, out_height, chroma_site=CHROMA_CENTER, zoom=1.0, out_camera=None):
    """the 4:2:2 chroma plane's camera in the header's operations, float64 -> (chroma lens (9,), chroma output camera
    (fx, fy, cx, cy)); the plane's frame time is the frame's"""
    L = _lens(lens)
    ox = CHROMA_OFFSET[chroma_site]
    if out_camera is None:
        sx, sy = out_width / width, out_height / height
        cam = [L[1] * sx, L[2] * sy, L[3] * sx, L[4] * sy]
    else:
        cam = [float(v) for v in out_camera]
    cam = [cam[0] * zoom, cam[1] * zoom, cam[2], cam[3]]

    def half(fx, fy, cx, cy):
        return (fx * 0.5, fy, (cx - ox) * 0.5, cy)

    return np.array((L[0],) + half(*L[1:5]) + tuple(L[5:]), np.float64), half(*cam)


def _launcher_cfg(problem, fmt, w, h, ow, oh, lens, delay, sigma, chroma_site, camera, iterations, fills, filter):
    """rship_color_cfg for stabilize_yuv_budget, as csrc/color_host.hpp resolves it; fills: None = the header's defaults for
    fill 0"""
    if fills is None:
        fills = (0, 128 << (DEPTH.get(fmt, 8) - 8), 128 << (DEPTH.get(fmt, 8) - 8), 0)
    fill = 0 if fmt in SIBLING else fills[0]            # (16-bit: cfg.fill alone is read)
    cfg = _Cfg()
    cfg.luma = _stab_launcher_cfg(problem, w, h, ow, oh, lens, delay, sigma, camera, iterations, fill, filter)
    cfg.chroma = cfg.luma
    if is_422(fmt):
        lens_c, cam_c = chroma_config(lens, w, h, ow, oh, chroma_site)
        cfg.chroma = _stab_launcher_cfg(problem, w // 2, h, ow // 2, oh, lens_c, delay, sigma, camera, iterations, fill, filter, cam=cam_c)
    cfg.chroma_time = 0.0
    cfg.format = int(fmt)
    for k in range(4):
        cfg.fill[k] = int(fills[k]) if k < len(fills) else 0
    return cfg


def stabilize_yuv_budget(problem, fmt, frames, frame_times, lens, delay, budget_bytes, out_size=None, out=None, sigma=0.0,
                         chroma_site=CHROMA_CENTER, iterations=DEFAULT_ITERATIONS, fills=None, filter=FILTER_BILINEAR):
    """stabilize_yuv along the path through the internal launcher with its device budget for the chunk slots given
    (tests: small frames that span several chunks).  LENS camera, zoom 1; fills: None = the header's defaults for fill 0.
    -> (planes -- `out` if given, else numpy arrays --, n_outside (n, 2))"""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(planes)
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, fmt, w, h, ow, oh, L, delay, sigma, chroma_site, CAMERA_LENS, iterations, fills, filter)
    res = [np.empty(s, np.uint16 if fmt in SIBLING else np.uint8) for s in plane_shapes(fmt, n, oh, ow)] if out is None else _as_planes(fmt, out)
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_yuv_frames(ctx, C.byref(src), n, t.ctypes.data_as(_PD), None, C.byref(cfg), C.byref(dst), outside.ctypes.data_as(_PU64),
                            int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep, okeep
    return tuple(res), outside[:n]
