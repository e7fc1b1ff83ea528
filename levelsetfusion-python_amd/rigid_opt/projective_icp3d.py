"""ProjectiveIcp3d: frame-to-model tracking by projective point-to-plane ICP (the KinectFusion tracker), which the
reference does not have.  INTEGRATION.md section 3 ("Projective ICP") defines the arithmetic and
tests/icp_restatement.py restates it.

The model's prediction -- depth and camera-space normals ray-cast at prediction_twist (CanonicalVolume.raycast with
normals=True) -- is the target.  Each live pixel with depth > 0 is taken to the world under the current twist,
projected into the prediction's camera and paired with the prediction pixel it lands on (rint on both axes) when that
pixel has a depth and a normal and the two points are at most max_distance apart.  Every iteration solves the 6 x 6
point-to-plane normal equations and composes the step into the twist; levels run coarse first, a level of stride s
using the live pixels (s i, s j) only.  The whole pyramid is one enqueue (device_icp.icp_run: sum(iterations) + 1
launches of csrc/lsf_icp.hip) and one copy back; the per-iteration records stay on the tracker as `last_records` (a
list of dicts: delta, twist, energy, matrix_a, vector_b, skipped, count, level, angle_rejected).

With a DepthPyramid (pyramid=...) the live frame is first turned into a filtered pyramid on the device, and level k of
the iterations (coarse first) uses every pixel of pyramid level len(iterations) - 1 - k instead of a stride;
max_normal_angle (radians) adds the normal-angle gate.  The pyramid of the last call stays as `last_pyramid`.

With photometric_weight (lambda; on the strided path, or on a pyramid with an intensity_pyramid) the solve is the
joint geometric and photometric one of INTEGRATION.md section 3 ("Photometric ICP"; tests/photometric_restatement.py restates it): every live pixel with a
geometric pair also compares its own intensity with the bilinear interpolant of the prediction's intensity image --
the Y channel of the model's ray-cast colour (CanonicalVolume.raycast with colours=True) -- at its unrounded projection,
and lambda times that residual and its Jacobian go into the same normal equations.  It holds the pose where geometry
does not: on a flat wall t_x, t_y and r_z leave the geometric A singular.  track and optimize then take the frame's
uint8 (H, W, 3) colour image and the prediction's (H, W, 4) colour image; max_intensity_difference gates |r_I|; the
records carry photometric_count and photometric_energy, and `last_intensity_residuals` keeps r_I beside
`last_residuals`.  lambda has no default: no value is right across scenes.

With pyramid, intensity_pyramid (an IntensityPyramid of the pyramid's levels) and photometric_weight together the joint
solve runs on the depth pyramid (device_icp.icp_run_pyramid_photometric; tests/pyramid_photometric_restatement.py
restates it): track builds an intensity pyramid of the frame's colour image and one of the prediction's Y, and a pixel
of level L with a geometric pair takes its intensity term at level L of both, with that level's intrinsics.
max_normal_angle still applies.  The two pyramids of the last call stay as `last_intensity_pyramids` (live,
prediction).  A pyramid with photometric_weight and without an intensity_pyramid is refused: there is no intensity
pyramid to take the term from.

With robust (a RobustLoss) every configuration above becomes an iteratively reweighted solve (INTEGRATION.md section 3,
"Robust ICP"; tests/robust_icp_restatement.py restates it): each pair's rows are scaled by the Huber or Tukey weight of
its own residual at the current twist, the geometric term by `scale`, the photometric one by `intensity_scale`.  A part
of the scene that moves against the rest sits inside the distance gate and drags a least-squares pose; a Tukey weight
takes it out of the solve.  The gates stay in front of the weights, a pair with weight 0 still counts, and the records
carry weight_sum, photometric_weight_sum and outliers; `last_weights` keeps the geometric weight image beside
`last_residuals`.  The scale has no default: none is right across sensors."""
import math

import numpy as np
import torch

from .. import device_icp
from ..device_core import require_gpu
from ..device_rigid import twist6
from .depth_pyramid import DepthPyramid
from .intensity_pyramid import IntensityPyramid
from .robust_loss import RobustLoss
from ..tsdf.generation import device_depth

__all__ = ["ProjectiveIcp3d"]


def _prediction(x, trailing):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to("cuda").to(torch.float32).contiguous()
    if t.dim() != 2 + len(trailing) or tuple(t.shape[2:]) != trailing:
        raise ValueError("the prediction must be depth (H, W), normals (H, W, 3) and colour (H, W, 4), got shape %s"
                         % (tuple(t.shape),))
    return t


class ProjectiveIcp3d:
    def __init__(self, camera, iterations=device_icp.ITERATIONS, strides=device_icp.STRIDES,
                 max_distance=device_icp.MAX_DISTANCE, pyramid=None, max_normal_angle=None, photometric_weight=None,
                 max_intensity_difference=math.inf, intensity_pyramid=None, robust=None):
        """pyramid: None (the strided live image) or a DepthPyramid, with which strides is not used and iterations has
        one entry per tracked level, at most pyramid.levels; max_normal_angle: the gate in radians (pyramid only);
        photometric_weight: None (geometric only) or lambda, finite and > 0 (with a pyramid it needs an
        intensity_pyramid); max_intensity_difference: the gate on |r_I|, > 0; intensity_pyramid: None or an
        IntensityPyramid of pyramid.levels levels, which needs both a pyramid and a photometric_weight; robust: None
        (least squares) or a RobustLoss, with any of the above"""
        self.camera = camera
        if pyramid is not None and not isinstance(pyramid, DepthPyramid):
            raise ValueError("pyramid must be a rigid_opt.DepthPyramid or None, got %r" % (pyramid,))
        self.pyramid, self.max_normal_angle = pyramid, None
        if max_normal_angle is not None:
            if pyramid is None:
                raise ValueError("max_normal_angle needs a pyramid: the strided path has no live normals")
            device_icp.cos_max_angle(max_normal_angle)
            self.max_normal_angle = float(max_normal_angle)
        if pyramid is None:
            self.iterations, self.strides = device_icp.levels(iterations, strides)
        else:
            self.iterations = device_icp.pyramid_iterations(iterations, pyramid.levels)
            self.strides = None
        if not float(max_distance) > 0:
            raise ValueError("max_distance must be positive")
        self.max_distance = float(max_distance)
        self.photometric_weight = None
        _, self.max_intensity_difference = device_icp.photometric_settings(1.0, max_intensity_difference)
        if intensity_pyramid is not None:
            if not isinstance(intensity_pyramid, IntensityPyramid):
                raise ValueError("intensity_pyramid must be a rigid_opt.IntensityPyramid or None, got %r"
                                 % (intensity_pyramid,))
            if pyramid is None or photometric_weight is None:
                raise ValueError("intensity_pyramid needs both a pyramid and a photometric_weight")
            if intensity_pyramid.levels != pyramid.levels:
                raise ValueError("intensity_pyramid has %d levels, the pyramid %d: they must be equal"
                                 % (intensity_pyramid.levels, pyramid.levels))
        self.intensity_pyramid = intensity_pyramid
        if photometric_weight is not None:
            if pyramid is not None and intensity_pyramid is None:
                raise ValueError("photometric_weight needs the strided path: there is no intensity pyramid")
            self.photometric_weight, _ = device_icp.photometric_settings(photometric_weight)
        if robust is not None and not isinstance(robust, RobustLoss):
            raise ValueError("robust must be a rigid_opt.RobustLoss or None, got %r" % (robust,))
        self.robust = robust
        self.last_records = []
        self.last_residuals = None
        self.last_weights = None  # the geometric weight image of the last robust call with residuals=True
        self.last_intensity_residuals = None
        self.last_pyramid = None
        self.last_intensity_pyramids = None  # (live, prediction) IntensityLevels of the last joint pyramid call

    def track(self, depth, code, prediction_depth, prediction_normals, twist_p, twist, residuals=False,
              colour_image=None, prediction_colour=None):
        """optimize() on device inputs (tsdf.generation.device_depth's depth and LSF_DEPTH_* code, the prediction's
        float32 device depth and normals at twist_p): (final twist, the unpacked records, the residual image or None).
        With a photometric_weight also the frame's uint8 (H, W, 3) device colour image and the prediction's float32
        (H, W, 4) one; the intensity residual image is kept as `last_intensity_residuals`"""
        if (self.photometric_weight is None) != (colour_image is None) or \
                (colour_image is None) != (prediction_colour is None):
            raise ValueError("colour_image and prediction_colour go with a tracker made with photometric_weight, and "
                             "only with one")
        if self.robust is not None:
            return self._track_robust(depth, code, prediction_depth, prediction_normals, twist_p, twist, residuals,
                                      colour_image, prediction_colour)
        if self.intensity_pyramid is not None:
            self.last_pyramid = self.pyramid.build_device(depth, code, self.camera)
            live, pred = self.last_intensity_pyramids = (self.intensity_pyramid.build_device(colour_image),
                                                         self.intensity_pyramid.build_prediction(prediction_colour))
            out, records, res, self.last_intensity_residuals = device_icp.icp_run_pyramid_photometric(
                *self.last_pyramid.buffers, live.buffer, self.pyramid.levels, prediction_depth, prediction_normals,
                pred.buffer, self.camera, twist_p, self.photometric_weight, twist, self.iterations, self.max_distance,
                self.max_normal_angle, self.max_intensity_difference, residuals)
        elif self.photometric_weight is not None:
            out, records, res, self.last_intensity_residuals = device_icp.icp_run_photometric(
                depth, code, colour_image, prediction_depth, prediction_normals, prediction_colour, self.camera,
                twist_p, self.photometric_weight, twist, self.iterations, self.strides, self.max_distance,
                self.max_intensity_difference, residuals)
        elif self.pyramid is None:
            out, records, res = device_icp.icp_run(depth, code, prediction_depth, prediction_normals, self.camera,
                                                   twist_p, twist, self.iterations, self.strides, self.max_distance,
                                                   residuals)
        else:
            self.last_pyramid = self.pyramid.build_device(depth, code, self.camera)
            out, records, res = device_icp.icp_run_pyramid(
                *self.last_pyramid.buffers, self.pyramid.levels, prediction_depth, prediction_normals, self.camera,
                twist_p, twist, self.iterations, self.max_distance, self.max_normal_angle, residuals)
        return out, [device_icp.unpack_record(r) for r in records], res

    def _track_robust(self, depth, code, prediction_depth, prediction_normals, twist_p, twist, residuals,
                      colour_image, prediction_colour):
        """track() through the robust entry points: the same four configurations"""
        if self.pyramid is None:
            out, records, res, self.last_intensity_residuals, self.last_weights = device_icp.icp_run_robust(
                depth, code, prediction_depth, prediction_normals, self.camera, twist_p, self.robust, twist,
                self.iterations, self.strides, self.max_distance, colour_image, prediction_colour,
                self.photometric_weight, self.max_intensity_difference, residuals)
        else:
            self.last_pyramid = self.pyramid.build_device(depth, code, self.camera)
            live = pred = None
            if self.intensity_pyramid is not None:
                live, pred = self.last_intensity_pyramids = (self.intensity_pyramid.build_device(colour_image),
                                                             self.intensity_pyramid.build_prediction(prediction_colour))
                live, pred = live.buffer, pred.buffer
            out, records, res, self.last_intensity_residuals, self.last_weights = device_icp.icp_run_pyramid_robust(
                *self.last_pyramid.buffers, self.pyramid.levels, prediction_depth, prediction_normals, self.camera,
                twist_p, self.robust, twist, self.iterations, self.max_distance, self.max_normal_angle, live, pred,
                self.photometric_weight, self.max_intensity_difference, residuals)
        return out, [device_icp.unpack_record(r) for r in records], res

    def optimize(self, live_depth, prediction_depth, prediction_normals, prediction_twist, twist=None,
                 residuals=False, colour_image=None, prediction_colour=None):
        """the float64 (6,) twist of the live depth frame (uint16 / float32 / float64, scaled by the camera's
        depth_unit_ratio), started from twist (prediction_twist by default).  residuals=True also keeps the last
        iteration's residual image (float32 device tensor, NaN without a correspondence) as `last_residuals`; with a
        pyramid it has the extents of the last iteration's level.  A tracker made with photometric_weight also takes
        colour_image (uint8 (H, W, 3), numpy or device) and prediction_colour ((H, W, 4) float32, numpy or device)."""
        require_gpu()
        depth, code = device_depth(live_depth)
        twist_p = twist6(prediction_twist)
        if colour_image is not None and not isinstance(colour_image, torch.Tensor):
            a = np.asarray(colour_image)
            if a.dtype != np.uint8:
                raise ValueError("colour_image must be uint8, got %s" % a.dtype)
            colour_image = torch.from_numpy(np.ascontiguousarray(a))
        if colour_image is not None:
            colour_image = colour_image.to("cuda")
        if prediction_colour is not None:
            prediction_colour = _prediction(prediction_colour, (4,))
        out, self.last_records, self.last_residuals = self.track(
            depth, code, _prediction(prediction_depth, ()), _prediction(prediction_normals, (3,)), twist_p,
            twist_p if twist is None else twist, residuals, colour_image, prediction_colour)
        return out
