"""Torch-facing wrapper of projective point-to-plane ICP (include/lsf_hip.h: lsf_icp_run).  Every argument is checked on
the host before the launches; a call enqueues sum(iterations) + 1 launches with no host wait and copies the twist and
the records back once.  The public interfaces are rigid_opt.ProjectiveIcp3d and
fusion.SequenceFusion3d(tracking_reference="icp").  icp_run_pyramid (lsf_icp_run_pyramid) is the same schedule over a
live depth pyramid (device_depth_pyramid), with an optional normal-angle gate.  icp_run_photometric
(lsf_icp_run_photometric) is icp_run with an intensity term against the ray-cast colour image
(device_raycast.raycast(..., colour=)) in the same normal equations; icp_run_pyramid_photometric
(lsf_icp_run_pyramid_photometric) is icp_run_pyramid with that term taken at each pixel's own level, between two
intensity pyramids (device_intensity_pyramid).  icp_run_robust (lsf_icp_run_robust) and icp_run_pyramid_robust
(lsf_icp_run_pyramid_robust) are the strided and the pyramid run, with or without the photometric term, with every
pair scaled by the Huber or Tukey weight of a rigid_opt.RobustLoss.  All six are run_strided or run_pyramid at one key
of ENTRIES, the table of the C entry points."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import (IcpParams, IcpPhotometricParams, IcpPyramidParams, IcpPyramidPhotometricParams,
                   IcpPyramidRobustParams, IcpRobustParams, lib)
from .device_core import require_gpu
from .device_fusion import check_colour_image
from .device_raycast import checked_depth_unit_ratio, checked_intrinsics, checked_live_depth, image_extents
from .device_rigid import enqueue_run, twist6

RECORD = _lib.ICP_RECORD_DOUBLES
ITERATIONS, STRIDES, MAX_DISTANCE = (4, 4, 6), (4, 2, 1), 0.02


def levels(iterations, strides):
    """the pyramid as two tuples of ints, coarse first: iterations >= 0 and strides >= 1 per level, at most
    ICP_MAX_LEVELS levels"""
    it = tuple(int(v) for v in np.atleast_1d(iterations))
    st = tuple(int(v) for v in np.atleast_1d(strides))
    if not 1 <= len(it) <= _lib.ICP_MAX_LEVELS or len(it) != len(st):
        raise ValueError("iterations and strides need one entry per level, 1 to %d levels, got %s and %s"
                         % (_lib.ICP_MAX_LEVELS, it, st))
    if min(it) < 0 or min(st) < 1:
        raise ValueError("iterations must be >= 0 and strides >= 1, got %s and %s" % (it, st))
    return it, st


def _common(p, camera, image_shape, twist_p, max_distance, iterations):
    """the fields lsf_icp_params and lsf_icp_pyramid_params share, checked, into p"""
    p.fx, p.fy, p.cx, p.cy = checked_intrinsics(camera)
    p.max_distance = float(max_distance)
    if not p.max_distance > 0:
        raise ValueError("max_distance must be positive")
    tp = twist6(twist_p)
    if not np.all(np.isfinite(tp)):
        raise ValueError("twist_p must be finite")
    p.twist_p[:] = list(tp)
    p.height, p.width = image_extents(image_shape)
    p.levels = len(iterations)
    p.iterations[:len(iterations)] = list(iterations)
    return p


def params(camera, image_shape, twist_p, depth_code, iterations=ITERATIONS, strides=STRIDES,
           max_distance=MAX_DISTANCE, into=None):
    """the lsf_icp_params of a call, after the host checks (into: another struct with its members to fill instead)"""
    it, st = levels(iterations, strides)
    p = _common(IcpParams() if into is None else into, camera, image_shape, twist_p, max_distance, it)
    p.depth_unit_ratio = checked_depth_unit_ratio(camera)
    p.depth_dtype = int(depth_code)
    p.strides[:len(st)] = list(st)
    return p


def photometric_settings(photometric_weight, max_intensity_difference=math.inf):
    """(lambda, gate) as floats after the checks: lambda finite and > 0, the gate > 0 (inf allowed)"""
    lam, gate = float(photometric_weight), float(max_intensity_difference)
    if not (math.isfinite(lam) and lam > 0):
        raise ValueError("photometric_weight must be finite and positive, got %r" % (photometric_weight,))
    if not gate > 0:
        raise ValueError("max_intensity_difference must be positive (inf allowed), got %r"
                         % (max_intensity_difference,))
    return lam, gate


def robust_settings(robust):
    """(loss code, scale, intensity_scale) of a rigid_opt.RobustLoss after the checks: a known loss, both scales > 0
    (inf allowed)"""
    code = getattr(robust, "code", None)
    scale, intensity_scale = getattr(robust, "scale", None), getattr(robust, "intensity_scale", None)
    if code not in (_lib.ICP_LOSS_HUBER, _lib.ICP_LOSS_TUKEY) or not isinstance(scale, float) or \
            not isinstance(intensity_scale, float):
        raise ValueError("robust must be a rigid_opt.RobustLoss, got %r" % (robust,))
    if not (scale > 0 and intensity_scale > 0):
        raise ValueError("the scales of a RobustLoss must be positive (inf allowed), got %r" % (robust,))
    return code, scale, intensity_scale


def _terms_into(p, photometric_weight, max_intensity_difference, robust=None):
    """the members a struct has beyond its geometric twin: a robust struct's loss (robust: a rigid_opt.RobustLoss), and
    lambda and its gate, which a photometric struct requires; on a robust one they are optional, and without a
    photometric_weight lambda is 0 and the gate is not read"""
    optional = hasattr(p, "loss")
    if optional:
        p.loss, p.scale, p.intensity_scale = robust_settings(robust)
    if optional and photometric_weight is None:
        p.photometric_weight, p.max_intensity_difference = 0.0, math.inf
    else:
        p.photometric_weight, p.max_intensity_difference = photometric_settings(photometric_weight,
                                                                                max_intensity_difference)
    return p


def photometric_params(camera, image_shape, twist_p, depth_code, photometric_weight, max_intensity_difference=math.inf,
                       iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE):
    """the lsf_icp_photometric_params of a call, after the host checks"""
    p = params(camera, image_shape, twist_p, depth_code, iterations, strides, max_distance, IcpPhotometricParams())
    return _terms_into(p, photometric_weight, max_intensity_difference)


def robust_params(camera, image_shape, twist_p, depth_code, robust, photometric_weight=None,
                  max_intensity_difference=math.inf, iterations=ITERATIONS, strides=STRIDES,
                  max_distance=MAX_DISTANCE):
    """the lsf_icp_robust_params of a call, after the host checks; photometric_weight None: the geometric solve"""
    p = params(camera, image_shape, twist_p, depth_code, iterations, strides, max_distance, IcpRobustParams())
    return _terms_into(p, photometric_weight, max_intensity_difference, robust)


def pyramid_iterations(iterations, pyramid_levels):
    """the iterations of a pyramid run as a tuple of ints >= 0, coarse first: one entry per tracked level, at most
    pyramid_levels of them; entry k runs on pyramid level len(iterations) - 1 - k"""
    it = tuple(int(v) for v in np.atleast_1d(iterations))
    if not 1 <= len(it) <= int(pyramid_levels) or min(it) < 0:
        raise ValueError("iterations need 1 to %d entries >= 0 (one per pyramid level), got %s"
                         % (int(pyramid_levels), it))
    return it


def cos_max_angle(max_normal_angle):
    """the gate's cosine of an angle in radians, 0 .. pi"""
    a = float(max_normal_angle)
    if not 0.0 <= a <= math.pi:
        raise ValueError("max_normal_angle must be in [0, pi] radians, got %r" % (max_normal_angle,))
    return max(-1.0, min(1.0, math.cos(a)))


def pyramid_params(camera, image_shape, pyramid_levels, twist_p, iterations=ITERATIONS, max_distance=MAX_DISTANCE,
                   max_normal_angle=None, into=None):
    """the lsf_icp_pyramid_params of a call, after the host checks; max_normal_angle None: no gate (into: another
    struct with its members to fill instead)"""
    p = IcpPyramidParams() if into is None else into
    p.height, p.width = image_extents(image_shape)
    p.pyramid_levels = int(pyramid_levels)
    if not 1 <= p.pyramid_levels <= _lib.ICP_MAX_LEVELS or (p.height >> (p.pyramid_levels - 1)) < 1 or \
            (p.width >> (p.pyramid_levels - 1)) < 1:
        raise ValueError("a %d x %d image has no %d-level pyramid" % (p.height, p.width, p.pyramid_levels))
    _common(p, camera, image_shape, twist_p, max_distance, pyramid_iterations(iterations, p.pyramid_levels))
    p.angle_gate = 0 if max_normal_angle is None else 1
    p.cos_max_angle = -1.0 if max_normal_angle is None else cos_max_angle(max_normal_angle)
    return p


def pyramid_photometric_params(camera, image_shape, pyramid_levels, twist_p, photometric_weight,
                               max_intensity_difference=math.inf, iterations=ITERATIONS, max_distance=MAX_DISTANCE,
                               max_normal_angle=None):
    """the lsf_icp_pyramid_photometric_params of a call, after the host checks"""
    p = pyramid_params(camera, image_shape, pyramid_levels, twist_p, iterations, max_distance, max_normal_angle,
                       IcpPyramidPhotometricParams())
    return _terms_into(p, photometric_weight, max_intensity_difference)


def pyramid_robust_params(camera, image_shape, pyramid_levels, twist_p, robust, photometric_weight=None,
                          max_intensity_difference=math.inf, iterations=ITERATIONS, max_distance=MAX_DISTANCE,
                          max_normal_angle=None):
    """the lsf_icp_pyramid_robust_params of a call, after the host checks"""
    p = pyramid_params(camera, image_shape, pyramid_levels, twist_p, iterations, max_distance, max_normal_angle,
                       IcpPyramidRobustParams())
    return _terms_into(p, photometric_weight, max_intensity_difference, robust)


def last_level(iterations):
    """the pyramid level of a run's last iteration (0 when there is none)"""
    it = tuple(iterations)
    ks = [k for k, n in enumerate(it) if n > 0]
    return len(it) - 1 - ks[-1] if ks else 0


# the entry point of a run by (pyramid, photometric, robust): its name in the library, its struct and its scratch bytes.
# A robust entry point takes the photometric term as an option, so its two keys share one row
_ROBUST = ("lsf_icp_run_robust", IcpRobustParams, _lib.ICP_ROBUST_SCRATCH_BYTES)
_PYRAMID_ROBUST = ("lsf_icp_run_pyramid_robust", IcpPyramidRobustParams, _lib.ICP_PYRAMID_ROBUST_SCRATCH_BYTES)
ENTRIES = {
    (False, False, False): ("lsf_icp_run", IcpParams, _lib.ICP_SCRATCH_BYTES),
    (False, True, False): ("lsf_icp_run_photometric", IcpPhotometricParams, _lib.ICP_PHOTOMETRIC_SCRATCH_BYTES),
    (False, False, True): _ROBUST,
    (False, True, True): _ROBUST,
    (True, False, False): ("lsf_icp_run_pyramid", IcpPyramidParams, _lib.ICP_PYRAMID_SCRATCH_BYTES),
    (True, True, False): ("lsf_icp_run_pyramid_photometric", IcpPyramidPhotometricParams,
                          _lib.ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES),
    (True, False, True): _PYRAMID_ROBUST,
    (True, True, True): _PYRAMID_ROBUST,
}


def _prediction(x, name, shape):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 device tensor (device_raycast.raycast)" % name)
    if tuple(x.shape) != shape:
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(x.shape), shape))
    return x


def output_images(shape, device, photometric, robust):
    """the three optional float32 images of a run: the residuals, the intensity residuals (with the term) and the
    weights (with a loss); three Nones without a shape"""
    if shape is None:
        return None, None, None
    return tuple(torch.empty(shape, dtype=torch.float32, device=device) if wanted else None
                 for wanted in (True, photometric, robust))


def _enqueue(key, p, live, term, pred_depth, pred_normals, twist, residual_shape):
    """the run of the filled struct p enqueued on key's entry point (device_rigid.enqueue_run) after the checks of the
    prediction.  live: the checked live inputs; term: the checked pair of the intensity term's images (live,
    prediction), or two Nones.  Returns (twist, records, residual image, intensity residual image, weight image)"""
    name, _, scratch_bytes = ENTRIES[key]
    _, photometric, robust = key
    pred = (_prediction(pred_depth, "pred_depth", (p.height, p.width)),
            _prediction(pred_normals, "pred_normals", (p.height, p.width, 3)))
    slots = 3 if robust else 2 if photometric else 1  # of the images in the entry point's prototype
    inputs = live + pred if slots == 1 else live + term[:1] + pred + term[1:]
    images = output_images(residual_shape, pred_depth.device, photometric, robust)
    out, records = enqueue_run(getattr(lib, name), name, inputs, p, twist, 6, 8, RECORD, scratch_bytes,
                               sum(p.iterations[:p.levels]), images[:slots])
    return (out, records) + images


def _term_given(photometric_weight, live, pred, names):
    """whether a robust run has the photometric term: its two images and photometric_weight are optional and go
    together"""
    photometric = photometric_weight is not None
    if (live is None) == photometric or (pred is None) == photometric:
        raise ValueError("%s, %s and photometric_weight go together" % names)
    return photometric


def run_strided(key, live_depth, depth_code, pred_depth, pred_normals, camera, twist_p, twist, iterations, strides,
                 max_distance, residuals, live_colour=None, pred_colour=None, photometric_weight=None,
                 max_intensity_difference=math.inf, robust=None):
    """the strided run of the entry point of key (an ENTRIES key with pyramid False), checked and enqueued: the final
    twist, the records and the three images of icp_run_robust, None where the key has none.  The six icp_run*
    functions are this and run_pyramid at a fixed key"""
    _, photometric, weighted = key
    require_gpu()
    h, w = checked_live_depth(live_depth, depth_code)
    p = params(camera, (h, w), twist_p, depth_code, iterations, strides, max_distance, ENTRIES[key][1]())
    if photometric or weighted:
        _terms_into(p, photometric_weight, max_intensity_difference, robust)
    if photometric:
        check_colour_image(live_colour, live_depth, (("pred_depth", pred_depth), ("pred_normals", pred_normals),
                                                     ("pred_colour", pred_colour)))
        _prediction(pred_colour, "pred_colour", (h, w, 4))
    return _enqueue(key, p, (live_depth,), (live_colour, pred_colour), pred_depth, pred_normals,
                    twist_p if twist is None else twist, (h, w) if residuals else None)


def run_pyramid(key, pyramid_depth, pyramid_normals, pyramid_levels, pred_depth, pred_normals, camera, twist_p,
                 twist, iterations, max_distance, max_normal_angle, residuals, pyramid_intensity=None,
                 pred_intensity=None, photometric_weight=None, max_intensity_difference=math.inf, robust=None):
    """the pyramid run of the entry point of key (pyramid True), checked and enqueued: run_strided's five values, the
    images at the extents of the last iteration's level"""
    _, photometric, weighted = key
    require_gpu()
    if not (isinstance(pred_depth, torch.Tensor) and pred_depth.dim() == 2):
        raise ValueError("pred_depth must be an (H, W) device tensor (device_raycast.raycast)")
    h, w = (int(v) for v in pred_depth.shape)
    p = pyramid_params(camera, (h, w), pyramid_levels, twist_p, iterations, max_distance, max_normal_angle,
                       ENTRIES[key][1]())
    if photometric or weighted:
        _terms_into(p, photometric_weight, max_intensity_difference, robust)
    pixels = sum((h >> l) * (w >> l) for l in range(p.pyramid_levels))
    live = (_prediction(pyramid_depth, "pyramid_depth", (pixels,)),
            _prediction(pyramid_normals, "pyramid_normals", (pixels, 3)))
    if photometric:
        _prediction(pyramid_intensity, "pyramid_intensity", (pixels,))
        _prediction(pred_intensity, "pred_intensity", (pixels,))
    last = last_level(p.iterations[:p.levels])
    return _enqueue(key, p, live, (pyramid_intensity, pred_intensity), pred_depth, pred_normals,
                    twist_p if twist is None else twist, (h >> last, w >> last) if residuals else None)


def icp_run(live_depth, depth_code, pred_depth, pred_normals, camera, twist_p, twist=None, iterations=ITERATIONS,
            strides=STRIDES, max_distance=MAX_DISTANCE, residuals=False):
    """the whole pyramid enqueued: sum(iterations) + 1 launches and one copy back.  live_depth: device depth image
    (uint16 / float32 / float64, depth_code LSF_DEPTH_*, scaled by camera.depth_unit_ratio); pred_depth (H, W) and
    pred_normals (H, W, 3): device_raycast.raycast's float32 outputs at twist_p; twist: the starting 6-vector (twist_p
    by default).  Returns (final twist float64 (6,), records float64 (sum(iterations), ICP_RECORD_DOUBLES), and the
    last iteration's residual image (H, W) as a float32 device tensor with residuals=True, else None)."""
    return run_strided((False, False, False), live_depth, depth_code, pred_depth, pred_normals, camera, twist_p,
                        twist, iterations, strides, max_distance, residuals)[:3]


def icp_run_photometric(live_depth, depth_code, live_colour, pred_depth, pred_normals, pred_colour, camera, twist_p,
                        photometric_weight, twist=None, iterations=ITERATIONS, strides=STRIDES,
                        max_distance=MAX_DISTANCE, max_intensity_difference=math.inf, residuals=False):
    """icp_run with the photometric term: the same launches and one copy back.  live_colour: the frame's uint8
    (H, W, 3) device image, registered to live_depth; pred_colour: the float32 (H, W, 4) device image of
    device_raycast.raycast(..., colour=) at twist_p; photometric_weight: lambda, finite and > 0;
    max_intensity_difference: the gate on |r_I| in units of Y.  Returns icp_run's triple and, fourth, the last
    iteration's intensity residual image (H, W) with residuals=True, else None; the records carry photometric_count
    and photometric_energy (unpack_record)."""
    return run_strided((False, True, False), live_depth, depth_code, pred_depth, pred_normals, camera, twist_p,
                        twist, iterations, strides, max_distance, residuals, live_colour, pred_colour,
                        photometric_weight, max_intensity_difference)[:4]


def icp_run_robust(live_depth, depth_code, pred_depth, pred_normals, camera, twist_p, robust, twist=None,
                   iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE, live_colour=None,
                   pred_colour=None, photometric_weight=None, max_intensity_difference=math.inf, residuals=False):
    """icp_run, or with live_colour, pred_colour and photometric_weight icp_run_photometric, with robust weights: the
    same launches and one copy back.  robust: a rigid_opt.RobustLoss.  Returns (final twist, records, and with
    residuals=True the last iteration's residual image, intensity residual image (None without the photometric term)
    and weight image -- w where the residual is finite, NaN elsewhere -- else three Nones); the records carry
    weight_sum, photometric_weight_sum and outliers (unpack_record)."""
    term = _term_given(photometric_weight, live_colour, pred_colour, ("live_colour", "pred_colour"))
    return run_strided((False, term, True), live_depth, depth_code, pred_depth, pred_normals, camera, twist_p, twist,
                        iterations, strides, max_distance, residuals, live_colour, pred_colour, photometric_weight,
                        max_intensity_difference, robust)


def icp_run_pyramid(pyramid_depth, pyramid_normals, pyramid_levels, pred_depth, pred_normals, camera, twist_p,
                    twist=None, iterations=ITERATIONS, max_distance=MAX_DISTANCE, max_normal_angle=None,
                    residuals=False):
    """ICP over a live pyramid (device_depth_pyramid.depth_pyramid's two buffers of pyramid_levels levels, at the
    prediction's extents), enqueued: sum(iterations) + 1 launches and one copy back.  iterations: one entry per tracked
    level, coarse first.  max_normal_angle (radians): the normal-angle gate, None for none.  Returns icp_run's triple;
    the residual image has the extents of the last iteration's level."""
    return run_pyramid((True, False, False), pyramid_depth, pyramid_normals, pyramid_levels, pred_depth,
                        pred_normals, camera, twist_p, twist, iterations, max_distance, max_normal_angle,
                        residuals)[:3]


def icp_run_pyramid_photometric(pyramid_depth, pyramid_normals, pyramid_intensity, pyramid_levels, pred_depth,
                                pred_normals, pred_intensity, camera, twist_p, photometric_weight, twist=None,
                                iterations=ITERATIONS, max_distance=MAX_DISTANCE, max_normal_angle=None,
                                max_intensity_difference=math.inf, residuals=False):
    """icp_run_pyramid with the photometric term at every pixel's own level: the same launches and one copy back.
    pyramid_intensity and pred_intensity: the buffers of device_intensity_pyramid.intensity_pyramid for the frame's
    colour image ("colour") and for the ray-cast colour image at twist_p ("prediction"), both of pyramid_levels levels
    at the prediction's extents.  Returns icp_run_photometric's four values; both residual images have the extents of
    the last iteration's level."""
    return run_pyramid((True, True, False), pyramid_depth, pyramid_normals, pyramid_levels, pred_depth, pred_normals,
                        camera, twist_p, twist, iterations, max_distance, max_normal_angle, residuals,
                        pyramid_intensity, pred_intensity, photometric_weight, max_intensity_difference)[:4]


def icp_run_pyramid_robust(pyramid_depth, pyramid_normals, pyramid_levels, pred_depth, pred_normals, camera, twist_p,
                           robust, twist=None, iterations=ITERATIONS, max_distance=MAX_DISTANCE,
                           max_normal_angle=None, pyramid_intensity=None, pred_intensity=None,
                           photometric_weight=None, max_intensity_difference=math.inf, residuals=False):
    """icp_run_pyramid, or with pyramid_intensity, pred_intensity and photometric_weight
    icp_run_pyramid_photometric, with robust weights.  Returns icp_run_robust's five values; the three images have the
    extents of the last iteration's level."""
    term = _term_given(photometric_weight, pyramid_intensity, pred_intensity,
                       ("pyramid_intensity", "pred_intensity"))
    return run_pyramid((True, term, True), pyramid_depth, pyramid_normals, pyramid_levels, pred_depth, pred_normals,
                        camera, twist_p, twist, iterations, max_distance, max_normal_angle, residuals,
                        pyramid_intensity, pred_intensity, photometric_weight, max_intensity_difference, robust)


def unpack_record(r):
    """one host record as a dict: the layout of include/lsf_hip.h (LSF_ICP_RECORD_DOUBLES); angle_rejected is 0 on
    every lsf_icp_run record, photometric_count and photometric_energy are 0 on every record that is not
    lsf_icp_run_photometric's or lsf_icp_run_pyramid_photometric's; weight_sum, photometric_weight_sum and outliers
    are 0 on every record that is not lsf_icp_run_robust's or lsf_icp_run_pyramid_robust's"""
    return {"delta": r[0:6].reshape(6, 1).copy(), "twist": r[6:12].reshape(6, 1).copy(), "energy": float(r[12]),
            "matrix_a": r[13:49].reshape(6, 6).copy(), "vector_b": r[49:55].reshape(6, 1).copy(),
            "skipped": int(r[55]), "count": int(r[56]), "level": int(r[57]), "angle_rejected": int(r[58]),
            "photometric_count": int(r[59]), "photometric_energy": float(r[60]), "weight_sum": float(r[61]),
            "photometric_weight_sum": float(r[62]), "outliers": int(r[63])}
