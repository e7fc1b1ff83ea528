"""Torch-facing wrappers of point-to-SDF tracking (include/lsf_hip.h: lsf_point_sdf_run, and with a colour term
against the colour volume lsf_point_sdf_run_photometric on the strided image and lsf_point_sdf_run_pyramid on the
depth pyramid).  Every pointer, dtype and
element count is checked on the host before the launches; a call enqueues sum(iterations) + 1 launches with no host
wait and copies the twist and the records back once (device_rigid.enqueue_run).  The public interfaces are
rigid_opt.PointToSdf3d and fusion.SequenceFusion3d(tracking_reference="sdf").  The records are device_icp's
(device_icp.unpack_record): angle_rejected holds the pixels that had a depth but no valid sample, weight_sum and
outliers are written with a rigid_opt.RobustLoss, the photometric slots are 0 without a colour term."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import PointSdfParams, PointSdfPhotometricParams, PointSdfPyramidParams, lib
from .device_core import require_gpu
from .device_fusion import check_colour_image, check_colour_volume, check_model
from .device_icp import (ITERATIONS, MAX_DISTANCE, RECORD, STRIDES, last_level, levels, output_images,  # noqa: F401
                         photometric_settings, pyramid_iterations, robust_settings, unpack_record)
from .device_raycast import checked_depth_unit_ratio, checked_intrinsics, checked_live_depth, image_extents
from .device_rigid import enqueue_run, twist6
from .tsdf.generation import offsets_of


def params(shape, camera, image_shape, depth_code, array_offset, voxel_size=0.004, narrow_band_width_voxels=20,
           iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE, robust=None, into=None):
    """the lsf_point_sdf_params of a call, after the host checks; robust: None or a rigid_opt.RobustLoss (into: another
    struct with its members to fill instead; with strides None the iterations are taken as they are, for a pyramid)"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError("point-to-SDF tracking needs a 3-D (Z, Y, X) volume of extents >= 2, got shape %s" % (shape,))
    it, st = (tuple(iterations), ()) if strides is None else levels(iterations, strides)
    p = PointSdfParams() if into is None else into
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


def _colour_into(p, robust, photometric_weight, max_intensity_difference):
    """the members the two colour structs have beyond lsf_point_sdf_params: lambda and its gate (0 and the gate alone
    without a photometric_weight) and the loss's intensity scale"""
    p.photometric_weight, p.max_intensity_difference = 0.0, photometric_settings(1.0, max_intensity_difference)[1]
    if photometric_weight is not None:
        p.photometric_weight, _ = photometric_settings(photometric_weight)
    p.intensity_scale = math.inf if robust is None else robust_settings(robust)[2]
    return p


def photometric_params(shape, camera, image_shape, depth_code, array_offset, voxel_size=0.004,
                       narrow_band_width_voxels=20, iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE,
                       robust=None, photometric_weight=None, max_intensity_difference=math.inf):
    """the lsf_point_sdf_photometric_params of a call, after the host checks; photometric_weight None: geometry only"""
    p = params(shape, camera, image_shape, depth_code, array_offset, voxel_size, narrow_band_width_voxels, iterations,
               strides, max_distance, robust, PointSdfPhotometricParams())
    return _colour_into(p, robust, photometric_weight, max_intensity_difference)


def pyramid_params(shape, camera, image_shape, pyramid_levels, array_offset, voxel_size=0.004,
                   narrow_band_width_voxels=20, iterations=ITERATIONS, max_distance=MAX_DISTANCE, robust=None,
                   photometric_weight=None, max_intensity_difference=math.inf):
    """the lsf_point_sdf_pyramid_params of a call, after the host checks: image_shape is level 0's, iterations has one
    entry per tracked level, at most pyramid_levels"""
    levels_ = int(pyramid_levels)
    h, w = image_extents(image_shape)
    if not 1 <= levels_ <= _lib.ICP_MAX_LEVELS or (h >> (levels_ - 1)) < 1 or (w >> (levels_ - 1)) < 1:
        raise ValueError("a %d x %d image has no %d-level pyramid" % (h, w, levels_))
    p = params(shape, camera, (h, w), _lib.DEPTH_F32, array_offset, voxel_size, narrow_band_width_voxels,
               pyramid_iterations(iterations, levels_), None, max_distance, robust, PointSdfPyramidParams())
    p.depth_unit_ratio = 1.0  # the pyramid is in metres
    p.pyramid_levels = levels_
    return _colour_into(p, robust, photometric_weight, max_intensity_difference)


# the entry point of a run by (pyramid, colour): its name in the library, its struct and its scratch bytes.  The loss is
# a member of all three structs, so it is no part of the key
_PYRAMID = ("lsf_point_sdf_run_pyramid", PointSdfPyramidParams, _lib.POINT_SDF_COLOUR_SCRATCH_BYTES)
ENTRIES = {
    (False, False): ("lsf_point_sdf_run", PointSdfParams, _lib.POINT_SDF_SCRATCH_BYTES),
    (False, True): ("lsf_point_sdf_run_photometric", PointSdfPhotometricParams, _lib.POINT_SDF_COLOUR_SCRATCH_BYTES),
    (True, False): _PYRAMID,  # the pyramid entry point takes the colour term as an option
    (True, True): _PYRAMID,
}


def _level_buffer(x, name, pixels, device):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 device tensor (device_depth_pyramid / "
                         "device_intensity_pyramid)" % name)
    if tuple(x.shape) != (pixels,):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(x.shape), (pixels,)))
    if x.device != device:
        raise ValueError("%s is on %s, tsdf on %s" % (name, x.device, device))
    return x


def _colour_given(tsdf, weight, colour, live, photometric_weight, live_name):
    """whether a run has the colour term: the colour volume and the live colour input go with a photometric_weight, and
    only with one"""
    photometric = photometric_weight is not None
    if (colour is None) == photometric or (live is None) == photometric:
        raise ValueError("colour, %s and photometric_weight go together" % live_name)
    if photometric:
        check_colour_volume(colour, tsdf, weight)
    return photometric


def _enqueue(key, p, tsdf, weight, colour, live, twist, residual_shape, photometric, robust):
    """the run of the filled struct p enqueued on key's entry point (device_rigid.enqueue_run).  live: the checked live
    inputs, (depth,) or (depth, the colour term's); an entry point without the term takes neither colour nor the
    intensity residual image.  Returns (twist, records, residual image, intensity residual image, weight image); the
    images are None without residual_shape, the intensity one also without the colour term, the weight image without a
    loss"""
    name, _, scratch_bytes = ENTRIES[key]
    start = twist6(twist)
    if not np.all(np.isfinite(start)):
        raise ValueError("twist must be finite")
    images = output_images(residual_shape, tsdf.device, photometric, robust is not None)
    plain = len(live) == 1
    out, records = enqueue_run(getattr(lib, name), name, (tsdf, weight) + (() if plain else (colour,)) + live, p, start,
                               6, 8, RECORD, scratch_bytes, sum(p.iterations[:p.levels]),
                               images[::2] if plain else images)
    return (out, records) + images


def run_strided(key, tsdf, weight, live_depth, depth_code, camera, array_offset, twist, voxel_size,
                narrow_band_width_voxels, iterations, strides, max_distance, robust, residuals, colour=None,
                live_colour=None, photometric_weight=None, max_intensity_difference=math.inf):
    """the strided run of the entry point of key (an ENTRIES key with pyramid False), checked and enqueued:
    point_sdf_run_photometric's five values.  point_sdf_run and point_sdf_run_photometric are this at a fixed key"""
    require_gpu()
    check_model(tsdf, weight)
    h, w = checked_live_depth(live_depth, depth_code, tsdf.device)
    p = params(tuple(tsdf.shape), camera, (h, w), depth_code, array_offset, voxel_size, narrow_band_width_voxels,
               iterations, strides, max_distance, robust, ENTRIES[key][1]())
    photometric = False
    if key[1]:
        _colour_into(p, robust, photometric_weight, max_intensity_difference)
        photometric = _colour_given(tsdf, weight, colour, live_colour, photometric_weight, "live_colour")
    if photometric:
        check_colour_image(live_colour, live_depth, (("tsdf", tsdf), ("weight", weight), ("colour", colour)))
    return _enqueue(key, p, tsdf, weight, colour, (live_depth, live_colour) if key[1] else (live_depth,), twist,
                    (h, w) if residuals else None, photometric, robust)


def point_sdf_run(tsdf, weight, live_depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                  narrow_band_width_voxels=20, iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE,
                  robust=None, residuals=False):
    """the whole run enqueued: sum(iterations) + 1 launches and one copy back.  tsdf, weight: the model's float32
    (Z, Y, X) device tensors; live_depth: device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*, scaled
    by camera.depth_unit_ratio); twist: the starting 6-vector; robust: None or a rigid_opt.RobustLoss (its scale weighs
    the residual in metres).  Returns (final twist float64 (6,), records float64 (sum(iterations), ICP_RECORD_DOUBLES),
    and with residuals=True the last iteration's residual image (H, W) as a float32 device tensor -- NaN where a pixel
    has no pair -- and, with a loss, its weight image, else two Nones)."""
    out, records, res, _, weights = run_strided((False, False), tsdf, weight, live_depth, depth_code, camera,
                                                array_offset, twist, voxel_size, narrow_band_width_voxels, iterations,
                                                strides, max_distance, robust, residuals)
    return out, records, res, weights


def point_sdf_run_photometric(tsdf, weight, live_depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                              narrow_band_width_voxels=20, iterations=ITERATIONS, strides=STRIDES,
                              max_distance=MAX_DISTANCE, robust=None, colour=None, live_colour=None,
                              photometric_weight=None, max_intensity_difference=math.inf, residuals=False):
    """point_sdf_run with the colour term: the same launches and one copy back.  colour: the model's float32
    (Z, Y, X, 4) device colour volume; live_colour: the frame's uint8 (H, W, 3) device image, registered to
    live_depth; photometric_weight: lambda, finite and > 0; the three go together, and without them the call is
    point_sdf_run's.  max_intensity_difference: the gate on |r_I| in units of Y.  Returns (final twist, records, and
    with residuals=True the last iteration's residual image, intensity residual image (None without the colour term)
    and weight image (None without a loss), else three Nones); the records carry photometric_count and
    photometric_energy, with a loss also photometric_weight_sum (unpack_record)."""
    return run_strided((False, True), tsdf, weight, live_depth, depth_code, camera, array_offset, twist, voxel_size,
                       narrow_band_width_voxels, iterations, strides, max_distance, robust, residuals, colour,
                       live_colour, photometric_weight, max_intensity_difference)


def point_sdf_run_pyramid(tsdf, weight, pyramid_depth, pyramid_levels, image_shape, camera, array_offset, twist,
                          voxel_size=0.004, narrow_band_width_voxels=20, iterations=ITERATIONS,
                          max_distance=MAX_DISTANCE, robust=None, colour=None, pyramid_intensity=None,
                          photometric_weight=None, max_intensity_difference=math.inf, residuals=False):
    """point-to-SDF tracking over a live depth pyramid, enqueued: sum(iterations) + 1 launches and one copy back.
    pyramid_depth: device_depth_pyramid.depth_pyramid's depth buffer of pyramid_levels
    levels for a frame of image_shape (H, W); iterations: one entry per tracked level, coarse first, entry k on level
    len(iterations) - 1 - k.  colour, pyramid_intensity (device_intensity_pyramid.intensity_pyramid's buffer of the
    frame's colour image, "colour") and photometric_weight go together: the colour term at every pixel's own level.
    There is no normal-angle gate.  Returns point_sdf_run_photometric's five values; the three images have the extents
    of the last iteration's level."""
    require_gpu()
    check_model(tsdf, weight)
    h, w = image_extents(image_shape)
    p = pyramid_params(tuple(tsdf.shape), camera, (h, w), pyramid_levels, array_offset, voxel_size,
                       narrow_band_width_voxels, iterations, max_distance, robust, photometric_weight,
                       max_intensity_difference)
    pixels = sum((h >> l) * (w >> l) for l in range(p.pyramid_levels))
    _level_buffer(pyramid_depth, "pyramid_depth", pixels, tsdf.device)
    photometric = _colour_given(tsdf, weight, colour, pyramid_intensity, photometric_weight, "pyramid_intensity")
    if photometric:
        _level_buffer(pyramid_intensity, "pyramid_intensity", pixels, tsdf.device)
    last = last_level(p.iterations[:p.levels])
    return _enqueue((True, photometric), p, tsdf, weight, colour, (pyramid_depth, pyramid_intensity), twist,
                    (h >> last, w >> last) if residuals else None, photometric, robust)
