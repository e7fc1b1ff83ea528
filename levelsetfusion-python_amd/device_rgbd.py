"""Torch-facing wrappers of the RGB-D sensor front end on the card (include/lsf_hip.h: lsf_rgbd_ray_table,
_register_depth, _rectify_colour; INTEGRATION.md section 3, "RGB-D sensor"; tests/rgbd_restatement.py restates them), and
the host rules of its arguments: the eight distortion coefficients, the four intrinsics, the 4 x 4 transform.  Every
argument is checked on the host before a launch; workspaces are torch tensors; the calls are enqueued and nothing waits.
The public interface is fusion.RgbdSensor and fusion.SequenceFusion3d(sensor=)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import RgbdParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_fusion import _check_others

MAX_FOOTPRINT = _lib.RGBD_MAX_FOOTPRINT
DEFAULT_FOOTPRINT = _lib.RGBD_DEFAULT_FOOTPRINT
RECORD_FIELDS = ("valid", "behind", "outside", "empty", "clipped", "written", "filled", "masked")
INT32_MAX = 2 ** 31 - 1
_DEPTH_CODES = {torch.uint16: _lib.DEPTH_U16, torch.float32: _lib.DEPTH_F32, torch.float64: _lib.DEPTH_F64}


def coefficients(k):
    """(k1, k2, p1, p2, k3, k4, k5, k6) as a float64 (8,): None, or 0, 4, 5 or 8 finite entries in any shape, padded
    with zeros"""
    a = np.zeros(0) if k is None else np.asarray(k, dtype=np.float64).reshape(-1)
    if a.size not in (0, 4, 5, 8):
        raise ValueError("distortion coefficients come as 0, 4, 5 or 8 entries (k1, k2, p1, p2, k3, k4, k5, k6), got %d"
                         % a.size)
    if not np.all(np.isfinite(a)):
        raise ValueError("distortion coefficients must be finite, got %r" % (a,))
    return np.concatenate([a, np.zeros(8 - a.size)])


def intrinsics(matrix, name="intrinsic_matrix"):
    """(fx, fy, cx, cy) as Python floats of a 3 x 3 matrix; the focal lengths finite and not 0, the centre finite"""
    K = np.asarray(matrix, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("%s must be 3 x 3, got shape %s" % (name, K.shape))
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if not (np.isfinite(fx) and np.isfinite(fy) and fx != 0 and fy != 0 and np.isfinite(cx) and np.isfinite(cy)):
        raise ValueError("%s needs finite fx, fy != 0 and a finite centre, got fx=%r fy=%r cx=%r cy=%r"
                         % (name, fx, fy, cx, cy))
    return fx, fy, cx, cy


def transform_of(matrix, name="depth_to_colour"):
    """a 4 x 4 finite float64 with q = R p + t in its first three rows"""
    T = np.asarray(matrix, dtype=np.float64)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise ValueError("%s must be a finite 4 x 4 matrix (q = R p + t), got %r" % (name, matrix))
    return T.copy()


def footprint_of(max_footprint):
    f = int(max_footprint)
    if f != max_footprint or not 1 <= f <= MAX_FOOTPRINT:
        raise ValueError("max_footprint must be a whole number in [1, %d], got %r" % (MAX_FOOTPRINT, max_footprint))
    return f


def _extents(shape, what):
    if len(shape) != 2 or min(shape) < 1:
        raise ValueError("%s needs extents (height, width) >= 1, got %s" % (what, tuple(shape)))
    h, w = int(shape[0]), int(shape[1])
    if (h + 1) * (w + 1) > INT32_MAX:
        raise ValueError("%s of %d x %d has more pixels than int32 indices reach" % (what, h, w))
    return h, w


def params(shape=None, K=None, k=None, out_shape=None, K_out=None, transform=None, depth_unit_ratio=1.0,
           max_footprint=DEFAULT_FOOTPRINT):
    """the lsf_rgbd_params of a call after the host checks; what an entry point does not read stays at its default"""
    p = RgbdParams()
    p.fx = p.fy = p.out_fx = p.out_fy = 1.0
    p.height = p.width = p.out_height = p.out_width = 1
    if shape is not None:
        p.height, p.width = _extents(shape, "the source image")
    if K is not None:
        p.fx, p.fy, p.cx, p.cy = intrinsics(K)
    p.k[:] = list(coefficients(k))
    if out_shape is not None:
        p.out_height, p.out_width = _extents(out_shape, "the output image")
    if K_out is not None:
        p.out_fx, p.out_fy, p.out_cx, p.out_cy = intrinsics(K_out, "output_intrinsics")
    T = np.eye(4) if transform is None else transform_of(transform)
    p.rotation[:] = [float(v) for v in T[:3, :3].reshape(-1)]
    p.translation[:] = [float(v) for v in T[:3, 3]]
    ratio = float(depth_unit_ratio)
    if not (np.isfinite(ratio) and ratio > 0):
        raise ValueError("depth_unit_ratio must be finite and > 0, got %r" % (depth_unit_ratio,))
    p.depth_unit_ratio = ratio
    p.max_footprint = footprint_of(max_footprint)
    return p


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check_buffer(name, t, dtype, shape, device=None, aligned=1):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s must be on the GPU" % name)
    if dtype is not None and t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, str(dtype).split(".")[-1], t.dtype))
    if device is not None and t.device != device:
        raise ValueError("%s is on %s, the call's other buffers on %s: all buffers must be on one device"
                         % (name, t.device, device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, the call needs %s" % (name, tuple(t.shape), tuple(shape)))
    if t.data_ptr() % aligned:
        raise ValueError("%s must be %d-byte aligned" % (name, aligned))


def _no_alias(buffers):
    named = [(n, t) for n, t in buffers if t is not None]
    for i, (name, t) in enumerate(named):
        _check_others(name, t, named[i + 1:])


def ray_table(shape, K, k=None, corner_rays=None, centre_rays=None):
    """lsf_rgbd_ray_table: (corner_rays float64 (H + 1, W + 1, 2), centre_rays float64 (H, W, 2)) device tensors, the
    undistorted normalised coordinates of a camera (matrix K, coefficients k) at its pixels' corners and centres.  Once
    per sensor; one launch, enqueued"""
    require_gpu()
    p = params(shape=shape, K=K, k=k)
    h, w = p.height, p.width
    if corner_rays is None:
        corner_rays = torch.empty((h + 1, w + 1, 2), dtype=torch.float64, device="cuda")
    if centre_rays is None:
        centre_rays = torch.empty((h, w, 2), dtype=torch.float64, device="cuda")
    _check_buffer("corner_rays", corner_rays, torch.float64, (h + 1, w + 1, 2), aligned=8)
    _check_buffer("centre_rays", centre_rays, torch.float64, (h, w, 2), corner_rays.device, aligned=8)
    _no_alias([("corner_rays", corner_rays), ("centre_rays", centre_rays)])
    check(lib.lsf_rgbd_ray_table(_ptr(corner_rays), _ptr(centre_rays), ctypes.byref(p), stream_ptr()),
          "lsf_rgbd_ray_table")
    return corner_rays, centre_rays


def register_depth(depth, corner_rays, centre_rays, depth_to_output, K_out, out_shape, depth_unit_ratio=1.0,
                   max_footprint=DEFAULT_FOOTPRINT, colour_valid=None, zbuffer=None, out_depth=None, record=None):
    """lsf_rgbd_register_depth: the device depth image (uint16 / float32 / float64, (H, W)) lifted along its rays, moved
    by q = R p + t (depth_to_output, 4 x 4) and splatted into the ideal camera K_out of out_shape.  Returns (out_depth
    float32 (Ho, Wo) in metres, 0 where nothing landed or colour_valid is 0; record int64 (8,), RECORD_FIELDS), both on
    the device.  zbuffer: the uint32 (Ho, Wo) workspace, made when None.  Three launches, enqueued; nothing waits"""
    require_gpu()
    if not isinstance(depth, torch.Tensor) or depth.dim() != 2 or depth.dtype not in _DEPTH_CODES:
        raise ValueError("depth must be a 2-D uint16, float32 or float64 device tensor (tsdf.generation.device_depth)")
    _check_buffer("depth", depth, None, None, aligned=depth.element_size())
    p = params(shape=tuple(depth.shape), out_shape=out_shape, K_out=K_out, transform=depth_to_output,
               depth_unit_ratio=depth_unit_ratio, max_footprint=max_footprint)
    h, w, ho, wo = p.height, p.width, p.out_height, p.out_width
    dev = depth.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    zbuffer = new((ho, wo), torch.int32) if zbuffer is None else zbuffer
    out_depth = new((ho, wo), torch.float32) if out_depth is None else out_depth
    record = new((len(RECORD_FIELDS),), torch.int64) if record is None else record
    _check_buffer("corner_rays", corner_rays, torch.float64, (h + 1, w + 1, 2), dev, aligned=8)
    _check_buffer("centre_rays", centre_rays, torch.float64, (h, w, 2), dev, aligned=8)
    if zbuffer.dtype not in (torch.int32, torch.uint32):
        raise ValueError("zbuffer must be a 32-bit integer tensor, got %s" % zbuffer.dtype)
    _check_buffer("zbuffer", zbuffer, None, (ho, wo), dev, aligned=4)
    _check_buffer("out_depth", out_depth, torch.float32, (ho, wo), dev, aligned=4)
    _check_buffer("record", record, torch.int64, (len(RECORD_FIELDS),), dev, aligned=8)
    if colour_valid is not None:
        _check_buffer("colour_valid", colour_valid, torch.uint8, (ho, wo), dev)
    _no_alias([("depth", depth), ("corner_rays", corner_rays), ("centre_rays", centre_rays), ("zbuffer", zbuffer),
               ("colour_valid", colour_valid), ("out_depth", out_depth), ("record", record)])
    check(lib.lsf_rgbd_register_depth(_ptr(depth), _DEPTH_CODES[depth.dtype], _ptr(corner_rays), _ptr(centre_rays),
                                      _ptr(zbuffer), _ptr(colour_valid), _ptr(out_depth), _ptr(record),
                                      ctypes.byref(p), stream_ptr()), "lsf_rgbd_register_depth")
    return out_depth, record


def rectify_colour(src, K_src, k_src, K_out, out_shape, dst=None, valid=None):
    """lsf_rgbd_rectify_colour: the raw uint8 (Hs, Ws, 3) device image of a camera (K_src, k_src) resampled bilinearly
    into the ideal camera K_out of out_shape.  Returns (dst uint8 (Ho, Wo, 3), valid uint8 (Ho, Wo)); a pixel without a
    source is (0, 0, 0) and valid 0.  One launch, enqueued"""
    require_gpu()
    if not isinstance(src, torch.Tensor) or src.dim() != 3 or src.shape[2] != 3:
        raise ValueError("the colour image must be a uint8 (H, W, 3) device tensor")
    _check_buffer("src", src, torch.uint8, None)
    p = params(shape=tuple(src.shape[:2]), K=K_src, k=k_src, out_shape=out_shape, K_out=K_out)
    ho, wo = p.out_height, p.out_width
    dst = torch.empty((ho, wo, 3), dtype=torch.uint8, device=src.device) if dst is None else dst
    valid = torch.empty((ho, wo), dtype=torch.uint8, device=src.device) if valid is None else valid
    _check_buffer("dst", dst, torch.uint8, (ho, wo, 3), src.device)
    _check_buffer("valid", valid, torch.uint8, (ho, wo), src.device)
    _no_alias([("src", src), ("dst", dst), ("valid", valid)])
    check(lib.lsf_rgbd_rectify_colour(_ptr(src), _ptr(dst), _ptr(valid), ctypes.byref(p), stream_ptr()),
          "lsf_rgbd_rectify_colour")
    return dst, valid


def unpack_record(record):
    """{valid, behind, outside, empty, clipped, written, filled, masked} of a host copy of a call's record"""
    r = np.asarray(record).reshape(-1)
    return {name: int(r[i]) for i, name in enumerate(RECORD_FIELDS)}
