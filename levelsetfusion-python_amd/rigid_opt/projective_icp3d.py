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
from .frame_tracker import FrameTracker, device_colour_image
from ..tsdf.generation import device_depth

__all__ = ["ProjectiveIcp3d"]


def _prediction(x, trailing):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to("cuda").to(torch.float32).contiguous()
    if t.dim() != 2 + len(trailing) or tuple(t.shape[2:]) != trailing:
        raise ValueError("the prediction must be depth (H, W), normals (H, W, 3) and colour (H, W, 4), got shape %s"
                         % (tuple(t.shape),))
    return t


class ProjectiveIcp3d(FrameTracker):
    def __init__(self, camera, iterations=device_icp.ITERATIONS, strides=device_icp.STRIDES,
                 max_distance=device_icp.MAX_DISTANCE, pyramid=None, max_normal_angle=None, photometric_weight=None,
                 max_intensity_difference=math.inf, intensity_pyramid=None, robust=None):
        """pyramid: None (the strided live image) or a DepthPyramid, with which strides is not used and iterations has
        one entry per tracked level, at most pyramid.levels; max_normal_angle: the gate in radians (pyramid only);
        photometric_weight: None (geometric only) or lambda, finite and > 0 (with a pyramid it needs an
        intensity_pyramid); max_intensity_difference: the gate on |r_I|, > 0; intensity_pyramid: None or an
        IntensityPyramid of pyramid.levels levels, which needs both a pyramid and a photometric_weight; robust: None
        (least squares) or a RobustLoss, with any of the above"""
        super().__init__(camera, iterations, strides, max_distance, pyramid, photometric_weight,
                         max_intensity_difference, intensity_pyramid, robust)
        self.max_normal_angle = None
        if max_normal_angle is not None:
            if pyramid is None:
                raise ValueError("max_normal_angle needs a pyramid: the strided path has no live normals")
            device_icp.cos_max_angle(max_normal_angle)
            self.max_normal_angle = float(max_normal_angle)
        self.last_intensity_pyramids = None  # (live, prediction) IntensityLevels of the last joint pyramid call

    def track(self, depth, code, prediction_depth, prediction_normals, twist_p, twist, residuals=False,
              colour_image=None, prediction_colour=None):
        """optimize() on device inputs (tsdf.generation.device_depth's depth and LSF_DEPTH_* code, the prediction's
        float32 device depth and normals at twist_p): (final twist, the unpacked records, the residual image or None).
        With a photometric_weight also the frame's uint8 (H, W, 3) device colour image and the prediction's float32
        (H, W, 4) one; the intensity residual image is kept as `last_intensity_residuals`, a loss's weight image as
        `last_weights`"""
        if (self.photometric_weight is None) != (colour_image is None) or \
                (colour_image is None) != (prediction_colour is None):
            raise ValueError("colour_image and prediction_colour go with a tracker made with photometric_weight, and "
                             "only with one")
        # the entry point is the configuration's (device_icp.ENTRIES): a tracker without a loss never runs a robust one
        key = (self.pyramid is not None, self.photometric_weight is not None, self.robust is not None)
        term = (self.photometric_weight, self.max_intensity_difference, self.robust)
        if self.pyramid is None:
            return self._keep(device_icp.run_strided(
                key, depth, code, prediction_depth, prediction_normals, self.camera, twist_p, twist, self.iterations,
                self.strides, self.max_distance, residuals, colour_image, prediction_colour, *term))
        self.last_pyramid = self.pyramid.build_device(depth, code, self.camera)
        live = pred = None
        if self.intensity_pyramid is not None:
            self.last_intensity_pyramids = (self.intensity_pyramid.build_device(colour_image),
                                            self.intensity_pyramid.build_prediction(prediction_colour))
            live, pred = (levels.buffer for levels in self.last_intensity_pyramids)
        return self._keep(device_icp.run_pyramid(
            key, *self.last_pyramid.buffers, self.pyramid.levels, prediction_depth, prediction_normals, self.camera,
            twist_p, twist, self.iterations, self.max_distance, self.max_normal_angle, residuals, live, pred, *term))

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
        if prediction_colour is not None:
            prediction_colour = _prediction(prediction_colour, (4,))
        out, self.last_records, self.last_residuals = self.track(
            depth, code, _prediction(prediction_depth, ()), _prediction(prediction_normals, (3,)), twist_p,
            twist_p if twist is None else twist, residuals, device_colour_image(colour_image), prediction_colour)
        return out
