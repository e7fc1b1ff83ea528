"""Torch-facing wrapper of the live depth pyramid (include/lsf_hip.h: lsf_depth_pyramid): the bilateral filter, the
depth-gated 2 x 2 means and the per-level normals KinectFusion computes before ICP.  Every argument is checked on the
host before the launches; a call enqueues levels + 1 launches with no host wait.  The public interface is
rigid_opt.DepthPyramid; device_icp.icp_run_pyramid tracks against its output."""
import ctypes
import math

import torch

from . import _lib
from ._lib import DepthPyramidParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_raycast import checked_depth_unit_ratio, checked_intrinsics, image_extents

LEVELS, RADIUS, SIGMA_SPACE, SIGMA_RANGE, DEPTH_GATE = 3, 3, 3.0, 0.03, 0.03


def settings(levels=LEVELS, radius=RADIUS, sigma_space=SIGMA_SPACE, sigma_range=SIGMA_RANGE, depth_gate=DEPTH_GATE):
    """the checked settings as (levels, radius, sigma_space, sigma_range, depth_gate)"""
    levels, radius = int(levels), int(radius)
    if not 1 <= levels <= _lib.ICP_MAX_LEVELS:
        raise ValueError("levels must be 1 to %d, got %d" % (_lib.ICP_MAX_LEVELS, levels))
    if not 0 <= radius <= _lib.PYRAMID_MAX_RADIUS:
        raise ValueError("radius must be 0 to %d, got %d" % (_lib.PYRAMID_MAX_RADIUS, radius))
    sigma_space, sigma_range, depth_gate = float(sigma_space), float(sigma_range), float(depth_gate)
    if not (math.isfinite(sigma_space) and sigma_space > 0 and math.isfinite(sigma_range) and sigma_range > 0):
        raise ValueError("sigma_space and sigma_range must be finite and positive")
    if not depth_gate > 0:
        raise ValueError("depth_gate must be positive")
    return levels, radius, sigma_space, sigma_range, depth_gate


def level_shapes(image_shape, levels):
    """(height >> l, width >> l) for l < levels; every extent must stay >= 1"""
    h, w = image_extents(image_shape)
    if (h >> (levels - 1)) < 1 or (w >> (levels - 1)) < 1:
        raise ValueError("a %d x %d image has no %d-level pyramid" % (h, w, levels))
    return [(h >> l, w >> l) for l in range(levels)]


def level_intrinsics(camera, levels):
    """(fx, fy, cx, cy) of every level, float64: fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2 per level"""
    fx, fy, cx, cy = checked_intrinsics(camera)
    out = [(fx, fy, cx, cy)]
    for _ in range(1, levels):
        fx, fy, cx, cy = fx / 2.0, fy / 2.0, (cx - 0.5) / 2.0, (cy - 0.5) / 2.0
        out.append((fx, fy, cx, cy))
    return out


def params(camera, image_shape, depth_code, levels=LEVELS, radius=RADIUS, sigma_space=SIGMA_SPACE,
           sigma_range=SIGMA_RANGE, depth_gate=DEPTH_GATE):
    """the lsf_depth_pyramid_params of a call, after the host checks"""
    levels, radius, sigma_space, sigma_range, depth_gate = settings(levels, radius, sigma_space, sigma_range,
                                                                    depth_gate)
    p = DepthPyramidParams()
    p.fx, p.fy, p.cx, p.cy = level_intrinsics(camera, 1)[0]
    p.depth_unit_ratio = checked_depth_unit_ratio(camera)
    p.sigma_space, p.sigma_range, p.depth_gate = sigma_space, sigma_range, depth_gate
    p.height, p.width = image_extents(image_shape)
    level_shapes((p.height, p.width), levels)
    p.depth_dtype = int(depth_code)
    p.levels, p.radius = levels, radius
    return p


def depth_pyramid(depth, depth_code, camera, levels=LEVELS, radius=RADIUS, sigma_space=SIGMA_SPACE,
                  sigma_range=SIGMA_RANGE, depth_gate=DEPTH_GATE):
    """the pyramid of a device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*, scaled by
    camera.depth_unit_ratio), enqueued: (depth, normals), two contiguous float32 device buffers holding the levels back to
    back, level 0 first -- (pixels,) metres and (pixels, 3) camera-space normals.  levels + 1 launches, no host wait."""
    require_gpu()
    if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.is_contiguous()):
        raise ValueError("depth must be a contiguous device tensor (tsdf.generation.device_depth)")
    p = params(camera, tuple(depth.shape), depth_code, levels, radius, sigma_space, sigma_range, depth_gate)
    pixels = sum(h * w for h, w in level_shapes((p.height, p.width), p.levels))
    out_depth = torch.empty(pixels, dtype=torch.float32, device=depth.device)
    out_normals = torch.empty((pixels, 3), dtype=torch.float32, device=depth.device)
    check(lib.lsf_depth_pyramid(ctypes.c_void_p(depth.data_ptr()), ctypes.c_void_p(out_depth.data_ptr()),
                                ctypes.c_void_p(out_normals.data_ptr()), ctypes.byref(p), stream_ptr()),
          "lsf_depth_pyramid")
    return out_depth, out_normals


def split_levels(buffer, shapes):
    """views of a pyramid buffer, one per level: (h, w) for depth, (h, w, 3) for normals"""
    out, at = [], 0
    for h, w in shapes:
        out.append(buffer[at:at + h * w].view((h, w) + tuple(buffer.shape[1:])))
        at += h * w
    return out
