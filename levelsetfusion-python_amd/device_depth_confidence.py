"""Torch-facing wrapper of the per-pixel confidence image (include/lsf_hip.h: lsf_depth_confidence):
c = |n . r| min(1, (reference_depth / z)^2) of a depth image in metres and its camera-space normals -- level 0 of
device_depth_pyramid.depth_pyramid's outputs.  Every argument is checked on the host before the launch; a call is one
launch with no host wait.  The public interface is fusion.DepthConfidence; device_fusion.integrate_depth_weighted takes
the image as its pixel_weight."""
import ctypes
import math

import torch

from ._lib import DepthConfidenceParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_raycast import checked_intrinsics, image_extents

REFERENCE_DEPTH = 0.5


def checked_reference_depth(reference_depth):
    """reference_depth as a float: metres, finite and > 0"""
    z = float(reference_depth)
    if not (math.isfinite(z) and z > 0):
        raise ValueError("reference_depth must be finite and > 0, got %r" % (reference_depth,))
    return z


def depth_confidence(depth_m, normals, camera, reference_depth=REFERENCE_DEPTH):
    """the float32 (H, W) confidence image of a float32 (H, W) device depth image in metres and its float32 (H, W, 3)
    device normals, enqueued: 0 where the depth is not > 0 or the normal is the zero vector"""
    z_ref = checked_reference_depth(reference_depth)
    require_gpu()
    for name, t in (("depth_m", depth_m), ("normals", normals)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError("%s must be a contiguous float32 device tensor" % name)
    if depth_m.dim() != 2 or tuple(normals.shape) != tuple(depth_m.shape) + (3,):
        raise ValueError("depth_m must be (H, W) and normals (H, W, 3), got %s and %s"
                         % (tuple(depth_m.shape), tuple(normals.shape)))
    if normals.device != depth_m.device:
        raise ValueError("normals is on %s, depth_m on %s: all buffers must be on one device"
                         % (normals.device, depth_m.device))
    p = DepthConfidenceParams()
    p.fx, p.fy, p.cx, p.cy = checked_intrinsics(camera)
    p.reference_depth = z_ref
    p.height, p.width = image_extents(tuple(depth_m.shape))
    out = torch.empty((p.height, p.width), dtype=torch.float32, device=depth_m.device)
    check(lib.lsf_depth_confidence(ctypes.c_void_p(depth_m.data_ptr()), ctypes.c_void_p(normals.data_ptr()),
                                   ctypes.c_void_p(out.data_ptr()), ctypes.byref(p), stream_ptr()),
          "lsf_depth_confidence")
    return out
