"""Torch-facing wrapper of point-to-SDF tracking (include/lsf_hip.h: lsf_point_sdf_run).  Every pointer, dtype and
element count is checked on the host before the launches; a call enqueues sum(iterations) + 1 launches with no host
wait and copies the twist and the records back once (device_rigid.enqueue_run).  The public interfaces are
rigid_opt.PointToSdf3d and fusion.SequenceFusion3d(tracking_reference="sdf").  The records are device_icp's
(device_icp.unpack_record): angle_rejected holds the pixels that had a depth but no valid sample, weight_sum and
outliers are written with a rigid_opt.RobustLoss, the photometric slots are 0."""
import numpy as np
import torch

from . import _lib
from ._lib import PointSdfParams, lib
from .device_core import require_gpu
from .device_fusion import check_model
from .device_icp import ITERATIONS, MAX_DISTANCE, RECORD, STRIDES, levels, robust_settings, unpack_record  # noqa: F401
from .device_raycast import checked_depth_unit_ratio, checked_intrinsics, image_extents
from .device_rigid import enqueue_run, twist6
from .tsdf.generation import offsets_of


def params(shape, camera, image_shape, depth_code, array_offset, voxel_size=0.004, narrow_band_width_voxels=20,
           iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE, robust=None):
    """the lsf_point_sdf_params of a call, after the host checks; robust: None or a rigid_opt.RobustLoss"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError("point-to-SDF tracking needs a 3-D (Z, Y, X) volume of extents >= 2, got shape %s" % (shape,))
    it, st = levels(iterations, strides)
    p = PointSdfParams()
    p.fx, p.fy, p.cx, p.cy = checked_intrinsics(camera)
    p.depth_unit_ratio = checked_depth_unit_ratio(camera)
    p.max_distance = float(max_distance)
    if not p.max_distance > 0:
        raise ValueError("max_distance must be positive")
    p.voxel_size, p.narrow_band_width_voxels = float(voxel_size), float(narrow_band_width_voxels)
    for name, value in (("voxel_size", p.voxel_size), ("narrow_band_width_voxels", p.narrow_band_width_voxels)):
        if not (np.isfinite(value) and value > 0):
            raise ValueError("%s must be finite and positive, got %r" % (name, value))
    p.offset_x, p.offset_y, p.offset_z = (float(v) for v in offsets_of(array_offset))
    if not np.all(np.isfinite([p.offset_x, p.offset_y, p.offset_z])):
        raise ValueError("array_offset must be finite")
    p.depth, p.height, p.width = shape
    p.image_height, p.image_width = image_extents(image_shape)
    p.depth_dtype = int(depth_code)
    if p.depth_dtype not in (_lib.DEPTH_U16, _lib.DEPTH_F32, _lib.DEPTH_F64):
        raise ValueError("depth_code must be an LSF_DEPTH_* code, got %r" % (depth_code,))
    p.levels = len(it)
    p.iterations[:len(it)] = list(it)
    p.strides[:len(st)] = list(st)
    p.loss, p.scale = _lib.POINT_SDF_LOSS_NONE, np.inf
    if robust is not None:
        p.loss, p.scale, _ = robust_settings(robust)
    return p


_DEPTH_DTYPES = {_lib.DEPTH_U16: torch.uint16, _lib.DEPTH_F32: torch.float32, _lib.DEPTH_F64: torch.float64}


def point_sdf_run(tsdf, weight, live_depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                  narrow_band_width_voxels=20, iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE,
                  robust=None, residuals=False):
    """the whole run enqueued: sum(iterations) + 1 launches and one copy back.  tsdf, weight: the model's float32
    (Z, Y, X) device tensors; live_depth: device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*, scaled
    by camera.depth_unit_ratio); twist: the starting 6-vector; robust: None or a rigid_opt.RobustLoss (its scale weighs
    the residual in metres).  Returns (final twist float64 (6,), records float64 (sum(iterations), ICP_RECORD_DOUBLES),
    and with residuals=True the last iteration's residual image (H, W) as a float32 device tensor -- NaN where a pixel
    has no pair -- and, with a loss, its weight image, else two Nones)."""
    require_gpu()
    check_model(tsdf, weight)
    if not (isinstance(live_depth, torch.Tensor) and live_depth.is_cuda and live_depth.is_contiguous()):
        raise ValueError("live_depth must be a contiguous device tensor (tsdf.generation.device_depth)")
    if live_depth.dim() != 2:
        raise ValueError("live_depth must be an (H, W) image, got shape %s" % (tuple(live_depth.shape),))
    if live_depth.device != tsdf.device:
        raise ValueError("live_depth is on %s, tsdf on %s" % (live_depth.device, tsdf.device))
    h, w = (int(v) for v in live_depth.shape)
    p = params(tuple(tsdf.shape), camera, (h, w), depth_code, array_offset, voxel_size, narrow_band_width_voxels,
               iterations, strides, max_distance, robust)
    if live_depth.dtype != _DEPTH_DTYPES[p.depth_dtype]:
        raise ValueError("live_depth is %s, its depth_code says %s" % (live_depth.dtype, _DEPTH_DTYPES[p.depth_dtype]))
    start = twist6(twist)
    if not np.all(np.isfinite(start)):
        raise ValueError("twist must be finite")
    res = weights = None
    if residuals:
        res = torch.empty((h, w), dtype=torch.float32, device=tsdf.device)
        if robust is not None:
            weights = torch.empty((h, w), dtype=torch.float32, device=tsdf.device)
    out, records = enqueue_run(lib.lsf_point_sdf_run, "lsf_point_sdf_run", (tsdf, weight, live_depth), p, start, 6, 8,
                               RECORD, _lib.POINT_SDF_SCRATCH_BYTES, sum(p.iterations[:p.levels]), (res, weights))
    return out, records, res, weights
