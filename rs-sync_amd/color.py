"""Colour frames stabilised on the GPU: NV12, I420 and RGBA32 (include/rssync_color.h), and their 10- and 16-bit kin GRAY16,
P010, P016 and I010 (include/rssync_color16.h).

What ``stabilize_frames`` does for 8-bit grayscale, for the layouts decoders hand out and viewers take, every plane of a
frame rendered in one pass (csrc/kernels/color.hpp).  The luma plane (and every channel of RGBA) is the stabiliser's result
byte for byte; a 4:2:0 chroma plane is the image of a camera of its own, half the size, whose sample (cu, cv) sits at luma
position (2 cu + ox, 2 cv + oy) -- ``chroma_site`` CHROMA_CENTER (0.5, 0.5) or CHROMA_LEFT (0, 0.5).

``frames``, per format (numpy arrays, pitched views included, or uint8 torch tensors on the problem's device):

    GRAY8    (n, H, W)
    NV12     (Y (n, H, W), UV (n, H/2, W/2, 2))
    I420     (Y (n, H, W), U (n, H/2, W/2), V (n, H/2, W/2))
    RGBA32   (n, H, W, 4)

The 16-bit formats have their sibling's shapes -- GRAY16 GRAY8's, P010 and P016 NV12's, I010 I420's -- with uint16 samples:
numpy uint16 arrays, or torch.uint16 / torch.int16 tensors on the problem's device (the bits are taken as unsigned).  P010
keeps a sample's ten bits in the high end of the word (value << 6); I010's words are the values.

The result is of the same kind and layout with the output's size, or written into ``out``.

Its own ctypes table, bound to the product library only: the colour front has no CPU test double.
"""
import ctypes as C

import numpy as np

from .problem import RsSyncError, product_library, product_only
from .rectify import _check, _is_torch, _lens
from .stabilize import StabilizeParams, _Cfg as _StabCfg, _targets, _times, params as _stab_params, CAMERA_LENS, DEFAULT_ITERATIONS
from .stabilize import _launcher_cfg as _stab_launcher_cfg
from .stabilize import FILTER_BILINEAR, FILTER_BICUBIC  # noqa: F401  (re-exported: stabilize_color(..., filter=FILTER_BICUBIC))

_PD = C.POINTER(C.c_double)
_SZ = C.c_size_t
_PU64 = C.POINTER(C.c_uint64)

GRAY8, NV12, I420, RGBA32 = 0, 1, 2, 3
GRAY16, P010, P016, I010 = 16, 17, 18, 19
SIBLING = {GRAY16: GRAY8, P010: NV12, P016: NV12, I010: I420}     # the 8-bit format with the same planes and geometry
DEPTH = {GRAY16: 16, P010: 10, P016: 16, I010: 10}               # bits of a sample value
CHROMA_CENTER, CHROMA_LEFT = 0, 1
CHROMA_OFFSET = {CHROMA_CENTER: (0.5, 0.5), CHROMA_LEFT: (0.0, 0.5)}
_N_PLANES = {GRAY8: 1, NV12: 2, I420: 3, RGBA32: 1, GRAY16: 1, P010: 2, P016: 2, I010: 3}


class ColorImage(C.Structure):
    """rssync_color_image"""
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", _SZ * 3), ("stride", _SZ * 3)]


class ColorParams(C.Structure):
    """rssync_color_params: zeros = the defaults"""
    _fields_ = [("stab", StabilizeParams), ("chroma_site", C.c_int32), ("fill_set", C.c_int32), ("fill", C.c_int32 * 4)]


class _Cfg(C.Structure):
    """rship_color_cfg (csrc/color_hip.h), for the tests' call of the internal launcher with a chunk budget"""
    _fields_ = [("luma", _StabCfg), ("chroma", _StabCfg), ("chroma_time", C.c_double), ("format", C.c_int32), ("fill", C.c_int32 * 4)]


_PI = C.POINTER(ColorImage)
_PP = C.POINTER(ColorParams)

# name -> (restype, argtypes): every function include/rssync_color.h and include/rssync_color16.h declare, and the internal
# launcher the tests call
SIGNATURES = {
    "rssync_color_stabilize": (C.c_int, [C.c_void_p, C.c_int, _PI, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double, _PD, _PP, _PI, _SZ, _SZ,
                                         _PU64]),
    "rssync_color16_stabilize": (C.c_int, [C.c_void_p, C.c_int, _PI, _SZ, _SZ, _SZ, _PD, C.c_void_p, C.c_double, _PD, _PP, _PI, _SZ, _SZ,
                                           _PU64]),
    "rssync_color_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _SZ, _SZ, C.c_void_p, _SZ, _SZ, C.c_double, C.c_double, _PD, _PP,
                                   C.c_void_p]),
    "rship_color_frames": (C.c_int, [C.c_void_p, _PI, C.c_uint32, _PD, _PD, C.POINTER(_Cfg), _PI, _PU64, _SZ]),
    "rship_last_error": (C.c_char_p, [C.c_void_p]),
}


def library():
    """the product library with the colour front's signatures attached"""
    return product_library(SIGNATURES)


def _lib_of(problem):
    return product_only(problem, library(), "the colour front")


def params(chroma_site=CHROMA_CENTER, fills=None, **kw):
    """fills: None = the defaults from `fill` (U, V = 128, A = 255; 16-bit formats: `fill` << (depth - 8) and
    1 << (depth - 1)), else the values in the format's order, 16-bit formats: in sample values; kw: the
    stabiliser's sigma, zoom, camera, out_camera, iterations, fill, filter (FILTER_BICUBIC: every plane and channel through
    the Catmull-Rom sampler, clamped to the format's range).  Everything is handed on as written."""
    prm = ColorParams()
    prm.stab = _stab_params(**kw)
    prm.chroma_site = int(chroma_site)
    if fills is not None:
        prm.fill_set = 1
        for k, v in enumerate(fills):
            prm.fill[k] = int(v)
    return prm


def plane_shapes(fmt, n, h, w):
    """the shapes of a format's planes for n frames of w x h (a 16-bit format's are its sibling's)"""
    fmt = SIBLING.get(fmt, fmt)
    return {GRAY8: [(n, h, w)], NV12: [(n, h, w), (n, h // 2, w // 2, 2)], I420: [(n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)],
            RGBA32: [(n, h, w, 4)]}[fmt]


def _as_planes(fmt, frames):
    if fmt not in _N_PLANES:
        raise ValueError("format must be GRAY8, NV12, I420, RGBA32, GRAY16, P010, P016 or I010")
    planes = [frames] if _N_PLANES[fmt] == 1 else list(frames)
    if len(planes) != _N_PLANES[fmt]:
        raise ValueError("this format has %d planes" % _N_PLANES[fmt])
    return planes


def _rows(a, writable, size=1):
    """one plane of `size`-byte samples -> (pointer, pitch, frame stride in bytes, keep-alive): the bytes of a row (its last
    one or two axes) must be contiguous; an input that is laid out otherwise is copied, an output is refused"""
    inner = a.ndim - 2                          # axes that make up a row: 1, or 2 for (W/2, 2) and (W, 4)
    name = "uint8" if size == 1 else "uint16"
    if _is_torch(a) and a.is_cuda:
        import torch
        if a.dtype not in ((torch.uint8,) if size == 1 else (torch.uint16, torch.int16)):
            raise ValueError("planes must be %s%s" % (name, "" if size == 1 else " (or int16: the bits are taken as unsigned)"))
        st, row = a.stride(), int(np.prod(a.shape[2:]))
        ok = st[-1] == 1 and (inner == 1 or st[-2] == a.shape[-1]) and st[1] >= row and (a.shape[0] < 2 or st[0] >= st[1] * a.shape[1])
        if not ok:
            if writable:
                raise ValueError("out planes must have contiguous rows")
            a = a.contiguous()
            st = a.stride()
        torch.cuda.current_stream(a.device).synchronize()
        return a.data_ptr(), st[1] * size, st[0] * size, a
    a = a.numpy() if _is_torch(a) else np.asarray(a)
    if a.dtype != (np.uint8 if size == 1 else np.uint16):
        raise ValueError("planes must be %s" % name)
    st, row = a.strides, int(np.prod(a.shape[2:])) * size
    ok = st[-1] == size and (inner == 1 or st[-2] == a.shape[-1] * size) and st[1] >= row and (a.shape[0] < 2 or st[0] >= st[1] * a.shape[1])
    if writable and not (ok and a.flags.writeable):
        raise ValueError("out planes must be writable %s arrays with contiguous rows" % name)
    if not ok:
        a = np.ascontiguousarray(a)
        st = a.strides
    return a.ctypes.data, st[1], st[0], a


def _image(fmt, planes, n, h, w, writable):
    """-> (ColorImage, keep-alive)"""
    shapes = plane_shapes(fmt, n, h, w)
    img, keep = ColorImage(), []
    for k, (a, shape) in enumerate(zip(planes, shapes)):
        if tuple(a.shape) != shape:
            raise ValueError("plane %d must have the shape %s, not %s" % (k, shape, tuple(a.shape)))
        img.plane[k], img.pitch[k], img.stride[k], alive = _rows(a, writable, 2 if fmt in SIBLING else 1)
        keep.append(alive)
    return img, keep


def _size(fmt, planes):
    y = planes[0]
    if y.ndim != (4 if fmt == RGBA32 else 3) or (fmt == RGBA32 and y.shape[3] != 4):
        raise ValueError("plane 0 must be (n, H, W)%s" % (" x 4" if fmt == RGBA32 else ""))
    return int(y.shape[0]), int(y.shape[1]), int(y.shape[2])


def _out_like(fmt, planes, n, oh, ow):
    y = planes[0]
    if _is_torch(y) and y.is_cuda:
        import torch
        return [torch.empty(s, dtype=torch.uint16 if fmt in SIBLING else torch.uint8, device=y.device) for s in plane_shapes(fmt, n, oh, ow)]
    return [np.empty(s, np.uint16 if fmt in SIBLING else np.uint8) for s in plane_shapes(fmt, n, oh, ow)]


def stabilize_color(problem, fmt, frames, frame_times, lens, delay, targets=None, out_size=None, out=None, chroma_site=CHROMA_CENTER,
                    fills=None, **kw):
    """-> (stabilised frames in the layout of `frames` -- `out` if given --, n_outside (n, 2) uint64: filled pixels of plane
    0, filled chroma samples).  out_size: (out_width, out_height), None = the input's.  kw: sigma, zoom, camera,
    out_camera, iterations, fill, filter."""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(fmt, planes)
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    res = _out_like(fmt, planes, n, oh, ow) if out is None else _as_planes(fmt, out)
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    prm = params(chroma_site, fills, **kw)
    tptr, tkeep = _targets(targets, n)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    entry = lib.rssync_color16_stabilize if fmt in SIBLING else lib.rssync_color_stabilize
    _check(problem, entry(problem._h, int(fmt), C.byref(src), n, w, h, t.ctypes.data_as(_PD), L.ctypes.data, float(delay), tptr, C.byref(prm),
                           C.byref(dst), ow, oh, outside.ctypes.data_as(_PU64)))
    del keep, okeep, tkeep
    if out is not None:
        return out, outside[:n]
    return (res[0] if len(res) == 1 else tuple(res)), outside[:n]


def color_map(problem, fmt, plane, width, height, lens, frame_time, delay, target=None, out_size=None, chroma_site=CHROMA_CENTER, **kw):
    """-> float32 source positions (x, y) of every output sample of `plane`: (out_height, out_width, 2) for plane 0,
    (out_height / 2, out_width / 2, 2) in chroma-plane coordinates for plane 1 of NV12 and I420.
    kw: sigma, zoom, camera, out_camera, iterations."""
    lib = _lib_of(problem)
    L = _lens(lens)
    ow, oh = (int(width), int(height)) if out_size is None else (int(out_size[0]), int(out_size[1]))
    out = np.zeros((oh // 2, ow // 2, 2) if plane else (oh, ow, 2), np.float32)
    prm = params(chroma_site, None, **kw)
    tptr, tkeep = _targets(None if target is None else np.asarray(target, np.float64).reshape(1, 4), 1)
    _check(problem, lib.rssync_color_map(problem._h, int(fmt), int(plane), int(width), int(height), L.ctypes.data, ow, oh,
                                         float(frame_time), float(delay), tptr, C.byref(prm), out.ctypes.data))
    del tkeep
    return out


def chroma_config(lens, width, height, out_width, out_height, chroma_site=CHROMA_CENTER, zoom=1.0, out_camera=None):
    """the chroma plane's camera in the header's operations, float64 -> (chroma lens (9,), chroma output camera
    (fx, fy, cx, cy), ro * (oy / height): what the chroma plane's frame time lies after the frame's)"""
    L = _lens(lens)
    ox, oy = CHROMA_OFFSET[chroma_site]
    if out_camera is None:
        sx, sy = out_width / width, out_height / height
        cam = [L[1] * sx, L[2] * sy, L[3] * sx, L[4] * sy]
    else:
        cam = [float(v) for v in out_camera]
    cam = [cam[0] * zoom, cam[1] * zoom, cam[2], cam[3]]

    def half(fx, fy, cx, cy):
        return (fx * 0.5, fy * 0.5, (cx - ox) * 0.5, (cy - oy) * 0.5)

    lens_c = np.array((L[0],) + half(*L[1:5]) + tuple(L[5:]), np.float64)
    return lens_c, half(*cam), float(L[0] * (oy / height))


def _launcher_cfg(problem, fmt, w, h, ow, oh, lens, delay, sigma, chroma_site, camera, iterations, fills, filter, zoom=1.0):
    """rship_color_cfg for the *_budget calls of the internal launchers, as csrc/color_host.hpp resolves it: the luma
    camera is the lens's scaled to the output, its focal lengths times `zoom` (1: a launcher that multiplies by a zoom per
    frame itself); fills: None = the header's defaults for fill 0"""
    if fills is None:
        fills = (0, 0, 0, 255) if fmt == RGBA32 else (0, 128 << (DEPTH.get(fmt, 8) - 8), 128 << (DEPTH.get(fmt, 8) - 8), 0)
    fill = 0 if fmt in SIBLING else fills[0]            # (16-bit: cfg.fill alone is read)
    cfg = _Cfg()
    cfg.luma = _stab_launcher_cfg(problem, w, h, ow, oh, lens, delay, sigma, camera, iterations, fill, filter, zoom=zoom)
    cfg.chroma = cfg.luma
    if SIBLING.get(fmt, fmt) in (NV12, I420):
        lens_c, cam_c, cfg.chroma_time = chroma_config(lens, w, h, ow, oh, chroma_site, zoom=float(zoom))
        cfg.chroma = _stab_launcher_cfg(problem, w // 2, h // 2, ow // 2, oh // 2, lens_c, delay, sigma, camera, iterations, fill, filter,
                                        cam=cam_c)
    cfg.format = int(fmt)
    for k in range(4):
        cfg.fill[k] = int(fills[k])
    return cfg


def stabilize_color_budget(problem, fmt, frames, frame_times, lens, delay, budget_bytes, out_size=None, sigma=0.0,
                           chroma_site=CHROMA_CENTER, iterations=DEFAULT_ITERATIONS, fills=None, filter=FILTER_BILINEAR):
    """stabilize_color along the path through the internal launcher with its device budget for the chunk slots given
    (tests: small frames that span several chunks).  LENS camera, zoom 1; fills: None = the header's defaults for fill 0.
    numpy frames -> (planes, n_outside (n, 2))"""
    lib = _lib_of(problem)
    planes = _as_planes(fmt, frames)
    n, h, w = _size(fmt, planes)
    src, keep = _image(fmt, planes, n, h, w, False)
    t = _times(frame_times, n)
    L = _lens(lens)
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    cfg = _launcher_cfg(problem, fmt, w, h, ow, oh, L, delay, sigma, chroma_site, CAMERA_LENS, iterations, fills, filter)
    res =[np.empty(s, np.uint16 if fmt in SIBLING else np.uint8) for s in plane_shapes(fmt, n, oh, ow)]
    dst, okeep = _image(fmt, res, n, oh, ow, True)
    outside = np.zeros((max(n, 1), 2), np.uint64)
    ctx = C.c_void_p(problem.device_context())
    if lib.rship_color_frames(ctx, C.byref(src), n, t.ctypes.data_as(_PD), None, C.byref(cfg), C.byref(dst),
                              outside.ctypes.data_as(_PU64), int(budget_bytes)):
        raise RsSyncError(lib.rship_last_error(ctx).decode())
    del keep, okeep
    return (res[0] if len(res) == 1 else tuple(res)), outside[:n]
