"""Torch-facing wrapper of the ray-caster (include/lsf_hip.h: lsf_raycast).  Every argument is checked on the host
before the launch; a call enqueues one launch and returns device tensors without waiting.  The public interface is
fusion.CanonicalVolume.raycast; fusion.SequenceFusion3d(tracking_reference="raycast") tracks against its output.
With the model's colour volume the call is lsf_raycast_colour: the same march, and a float32 (H, W, 4) image of
(R, G, B, Y) at the hit points beside it."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import RaycastParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_fusion import check_colour_volume, check_model
from .device_rigid import twist6
from .tsdf.generation import offsets_of


def image_extents(image_shape):
    s = tuple(int(v) for v in image_shape)
    if len(s) != 2 or min(s) < 1 or s[0] * s[1] > 0x7fffffff:
        raise ValueError("image_shape must be (height, width) with extents >= 1, got %s" % (tuple(image_shape),))
    return s


def checked_intrinsics(camera):
    """(fx, fy, cx, cy) of the camera's intrinsic matrix as floats: finite, fx and fy non-zero"""
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    k = float(P[0, 0]), float(P[1, 1]), float(P[0, 2]), float(P[1, 2])
    if not (np.all(np.isfinite(k)) and k[0] != 0 and k[1] != 0):
        raise ValueError("the intrinsics must be finite with fx, fy != 0")
    return k


def checked_depth_unit_ratio(camera):
    """the camera's depth_unit_ratio as a float: finite"""
    ratio = float(camera.depth_unit_ratio)
    if not np.isfinite(ratio):
        raise ValueError("the camera's depth_unit_ratio must be finite")
    return ratio


DEPTH_DTYPES = {_lib.DEPTH_U16: torch.uint16, _lib.DEPTH_F32: torch.float32, _lib.DEPTH_F64: torch.float64}


def checked_live_depth(live_depth, depth_code, device=None):
    """(H, W) of a tracker's live depth image after its checks: a contiguous 2-D device tensor of the dtype its
    LSF_DEPTH_* depth_code names -- a kernel reads it at that width --, on `device` (the model's) where one is given"""
    if not (isinstance(live_depth, torch.Tensor) and live_depth.is_cuda and live_depth.is_contiguous()):
        raise ValueError("live_depth must be a contiguous device tensor (tsdf.generation.device_depth)")
    if live_depth.dim() != 2:
        raise ValueError("live_depth must be an (H, W) image, got shape %s" % (tuple(live_depth.shape),))
    if device is not None and live_depth.device != device:
        raise ValueError("live_depth is on %s, tsdf on %s" % (live_depth.device, device))
    if depth_code not in DEPTH_DTYPES:
        raise ValueError("depth_code must be an LSF_DEPTH_* code, got %r" % (depth_code,))
    if live_depth.dtype != DEPTH_DTYPES[depth_code]:
        raise ValueError("live_depth is %s, its depth_code says %s" % (live_depth.dtype, DEPTH_DTYPES[depth_code]))
    return int(live_depth.shape[0]), int(live_depth.shape[1])


def params(shape, camera, twist, array_offset, voxel_size, image_shape, fallback_code=None):
    """the lsf_raycast_params of a call, after the host checks"""
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError("ray-casting needs a 3-D (Z, Y, X) volume of extents >= 2, got shape %s" % (tuple(shape),))
    p = RaycastParams()
    p.fx, p.fy, p.cx, p.cy = checked_intrinsics(camera)
    p.depth_unit_ratio = float(camera.depth_unit_ratio)
    p.voxel_size = float(voxel_size)
    if not (np.isfinite(p.voxel_size) and p.voxel_size > 0):
        raise ValueError("voxel_size must be finite and positive")
    p.offset_x, p.offset_y, p.offset_z = (float(v) for v in offsets_of(array_offset))
    p.t_x, p.t_y, p.t_z, p.r_x, p.r_y, p.r_z = (float(v) for v in twist6(twist))
    if not np.all(np.isfinite([p.offset_x, p.offset_y, p.offset_z, p.t_x, p.t_y, p.t_z, p.r_x, p.r_y, p.r_z])):
        raise ValueError("array_offset and twist must be finite")
    p.depth, p.height, p.width = (int(v) for v in shape)
    p.image_height, p.image_width = image_extents(image_shape)
    if fallback_code is not None:
        checked_depth_unit_ratio(camera)
        p.fallback_dtype = int(fallback_code)
    return p


def raycast(tsdf, weight, camera, twist, array_offset, voxel_size=0.004, image_shape=(480, 640), normals=False,
            fallback_depth=None, fallback_code=None, hit_count=None, colour=None):
    """one launch of lsf_raycast on the (Z, Y, X) model.  fallback_depth: a contiguous device depth image of
    image_shape (tsdf.generation.device_depth) and its LSF_DEPTH_* code, scaled by camera.depth_unit_ratio where a ray
    hits nothing.  hit_count: a device int64 tensor of one element the hit count is added to, or None for a fresh
    one.  Returns (depth (H, W), normals (H, W, 3) or None, hit_count) as device tensors; nothing waits.  colour: the
    model's float32 (Z, Y, X, 4) colour volume; with it the launch is lsf_raycast_colour's and the float32 (H, W, 4)
    image of (R, G, B, Y), NaN where a pixel has no hit or no colour, is returned as a fourth value."""
    require_gpu()
    check_model(tsdf, weight)
    if colour is not None:
        check_colour_volume(colour, tsdf, weight)
    p = params(tuple(tsdf.shape), camera, twist, array_offset, voxel_size, image_shape,
               None if fallback_depth is None else fallback_code)
    h, w = p.image_height, p.image_width
    if fallback_depth is not None:
        if fallback_code is None:
            raise ValueError("fallback_depth needs its LSF_DEPTH_* code (tsdf.generation.device_depth)")
        if not isinstance(fallback_depth, torch.Tensor) or not fallback_depth.is_cuda or \
                not fallback_depth.is_contiguous():
            raise ValueError("fallback_depth must be a contiguous device tensor (tsdf.generation.device_depth)")
        if tuple(fallback_depth.shape) != (h, w):
            raise ValueError("fallback_depth has shape %s, the image %s" % (tuple(fallback_depth.shape), (h, w)))
        if fallback_depth.device != tsdf.device:
            raise ValueError("fallback_depth is on %s, tsdf on %s" % (fallback_depth.device, tsdf.device))
    if hit_count is None:
        hit_count = torch.zeros(1, dtype=torch.int64, device=tsdf.device)
    elif not (isinstance(hit_count, torch.Tensor) and hit_count.is_cuda and hit_count.dtype == torch.int64 and
              hit_count.numel() == 1):
        raise ValueError("hit_count must be a device int64 tensor of one element")
    depth = torch.empty((h, w), dtype=torch.float32, device=tsdf.device)
    out_normals = torch.empty((h, w, 3), dtype=torch.float32, device=tsdf.device) if normals else None
    fb = None if fallback_depth is None else ctypes.c_void_p(fallback_depth.data_ptr())
    nrm = None if out_normals is None else ctypes.c_void_p(out_normals.data_ptr())
    if colour is None:
        check(lib.lsf_raycast(ctypes.c_void_p(tsdf.data_ptr()), ctypes.c_void_p(weight.data_ptr()), fb,
                              ctypes.c_void_p(depth.data_ptr()), nrm, ctypes.c_void_p(hit_count.data_ptr()),
                              ctypes.byref(p), stream_ptr()), "lsf_raycast")
        return depth, out_normals, hit_count
    out_colour = torch.empty((h, w, 4), dtype=torch.float32, device=tsdf.device)
    check(lib.lsf_raycast_colour(ctypes.c_void_p(tsdf.data_ptr()), ctypes.c_void_p(weight.data_ptr()),
                                 ctypes.c_void_p(colour.data_ptr()), fb, ctypes.c_void_p(depth.data_ptr()), nrm,
                                 ctypes.c_void_p(out_colour.data_ptr()), ctypes.c_void_p(hit_count.data_ptr()),
                                 ctypes.byref(p), stream_ptr()), "lsf_raycast_colour")
    return depth, out_normals, hit_count, out_colour
