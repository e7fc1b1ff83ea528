"""PointToSdf3d: frame-to-model tracking of the live depth points against the canonical TSDF itself (Bylow et al.,
"Real-Time Camera Tracking and 3D Reconstruction Using Signed Distance Functions", RSS 2013), which the reference does
not have.  INTEGRATION.md section 3 ("Point-to-SDF tracking") defines the arithmetic and
tests/point_sdf_restatement.py restates it.

Each live pixel with depth > 0 is taken to the world under the current twist and the model's signed distance is read
there trilinearly -- valid only where all 8 corner weights are > 0, the ray-caster's sample.  That value, in metres, is
the residual; the same 8 corners give its gradient; a pixel is a pair when |r| <= max_distance and the gradient is not
zero.  Every iteration solves the 6 x 6 normal equations and composes the step into the twist, ProjectiveIcp3d's
update; levels run coarse first, a level of stride s using the live pixels (s i, s j) only.  There is no prediction
image, no normal and no association step, and the model is read at the current estimate in every iteration.  The whole
run is one enqueue (device_point_sdf.point_sdf_run: sum(iterations) + 1 launches of csrc/lsf_point_sdf.hip) and one copy
back; the per-iteration records stay on the tracker as `last_records` (device_icp.unpack_record's dicts;
angle_rejected holds the pixels that had a depth but no valid sample).

With a DepthPyramid (pyramid=...) the live frame is first turned into a filtered pyramid on the device, and entry k of
the iterations (coarse first) uses every pixel of pyramid level len(iterations) - 1 - k, back-projected with that
level's intrinsics, instead of a stride (device_point_sdf.point_sdf_run_pyramid).  There is no normal-angle gate: the
model has no normal image here and the pyramid's normals are not read.  The pyramid of the last call stays as
`last_pyramid`; the residual images have the extents of the last iteration's level.

With photometric_weight (lambda; tests/point_sdf_colour_restatement.py restates it) a pixel with a geometric pair also
reads the model's colour volume at the same 8 corners -- all 8 colour weights must be > 0 -- and compares the trilinear
luminance there with its own intensity: the live colour image's pixel on the strided path
(device_point_sdf.point_sdf_run_photometric), the pixel of its level of an IntensityPyramid of the frame's colour image
on a pyramid (intensity_pyramid=..., of the pyramid's levels).  lambda times that residual and its Jacobian -- the
luminance gradient in the volume -- go into the same normal equations, which holds the pose where geometry does not: on
a flat wall every SDF gradient is parallel to the normal and A is singular.  track and optimize then take the model's
colour volume (`colour=`) and the frame's uint8 (H, W, 3) image (`colour_image=`); max_intensity_difference gates
|r_I|; the records carry photometric_count and photometric_energy and `last_intensity_residuals` keeps r_I beside
`last_residuals`, `last_intensity_pyramid` the frame's intensity pyramid.  lambda has no default: no value is right
across scenes.

With robust (a RobustLoss) each pair's rows are scaled by the Huber or Tukey weight of its own residual, the geometric
term at `scale` (metres), the colour term at `intensity_scale` (units of Y); the records carry weight_sum,
photometric_weight_sum and outliers and `last_weights` keeps the geometric weight image beside `last_residuals`.  On a
clean scene it is not more accurate than ProjectiveIcp3d; what it saves is the ray-cast of the prediction
(profiles/point_sdf_cost.md, profiles/point_sdf_colour_cost.md)."""
import math

import numpy as np
import torch

from .. import device_icp, device_point_sdf
from ..device_core import require_gpu
from ..device_rigid import twist6
from .frame_tracker import FrameTracker, device_colour_image
from ..tsdf.generation import device_depth

__all__ = ["PointToSdf3d"]


def _volume(x):
    """a model array (numpy or tensor) as a contiguous float32 device tensor"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to("cuda").to(torch.float32).contiguous()


class PointToSdf3d(FrameTracker):
    def __init__(self, camera, iterations=device_icp.ITERATIONS, strides=device_icp.STRIDES,
                 max_distance=device_icp.MAX_DISTANCE, robust=None, pyramid=None, photometric_weight=None,
                 max_intensity_difference=math.inf, intensity_pyramid=None):
        """iterations and strides: one entry per level, coarse first; max_distance: the gate on |r| in metres, > 0;
        robust: None (least squares) or a RobustLoss; pyramid: None (the strided live image) or a DepthPyramid, with
        which strides is not used and iterations has one entry per tracked level, at most pyramid.levels;
        photometric_weight: None (geometry only) or lambda, finite and > 0 (with a pyramid it needs an
        intensity_pyramid); max_intensity_difference: the gate on |r_I|, > 0; intensity_pyramid: None or an
        IntensityPyramid of pyramid.levels levels, which needs both a pyramid and a photometric_weight"""
        super().__init__(camera, iterations, strides, max_distance, pyramid, photometric_weight,
                         max_intensity_difference, intensity_pyramid, robust)
        self.last_intensity_pyramid = None  # the frame's IntensityLevels of the last joint pyramid call

    def track(self, depth, code, tsdf, weight, array_offset, twist, voxel_size=0.004, narrow_band_width_voxels=20,
              residuals=False, colour=None, colour_image=None):
        """optimize() on device inputs (tsdf.generation.device_depth's depth and LSF_DEPTH_* code, the model's float32
        device tsdf and weight): (final twist, the unpacked records, the residual image or None); the weight image is
        kept as `last_weights`.  With a photometric_weight also the model's float32 (Z, Y, X, 4) device colour volume
        and the frame's uint8 (H, W, 3) device colour image; the intensity residual image is kept as
        `last_intensity_residuals`"""
        if (self.photometric_weight is None) != (colour is None) or (colour is None) != (colour_image is None):
            raise ValueError("colour and colour_image go with a tracker made with photometric_weight, and only with "
                             "one")
        if self.pyramid is None:  # the entry point with the colour members only for a tracker with the term
            return self._keep(device_point_sdf.run_strided(
                (False, self.photometric_weight is not None), tsdf, weight, depth, code, self.camera, array_offset,
                twist, voxel_size, narrow_band_width_voxels, self.iterations, self.strides, self.max_distance,
                self.robust, residuals, colour, colour_image, self.photometric_weight, self.max_intensity_difference))
        self.last_pyramid = self.pyramid.build_device(depth, code, self.camera)
        live = None
        if self.intensity_pyramid is not None:
            self.last_intensity_pyramid = self.intensity_pyramid.build_device(colour_image)
            live = self.last_intensity_pyramid.buffer
        return self._keep(device_point_sdf.point_sdf_run_pyramid(
            tsdf, weight, self.last_pyramid.buffers[0], self.pyramid.levels, tuple(depth.shape), self.camera,
            array_offset, twist, voxel_size, narrow_band_width_voxels, self.iterations, self.max_distance, self.robust,
            colour, live, self.photometric_weight, self.max_intensity_difference, residuals))

    def optimize(self, depth_image, tsdf, weight, array_offset, twist=None, voxel_size=0.004,
                 narrow_band_width_voxels=20, residuals=False, colour=None, colour_image=None):
        """the float64 (6,) twist of the live depth frame (uint16 / float32 / float64, numpy or device, scaled by the
        camera's depth_unit_ratio) against the model tsdf / weight ((Z, Y, X), numpy or device; a CanonicalVolume's),
        started from twist (zero by default).  residuals=True also keeps the last iteration's residual image (float32
        device tensor, NaN without a pair) as `last_residuals`, and with a loss the weight image as `last_weights`.  A
        tracker made with photometric_weight also takes colour (the model's (Z, Y, X, 4) colour volume, numpy or
        device) and colour_image (uint8 (H, W, 3), numpy or device)."""
        require_gpu()
        depth, code = device_depth(depth_image)
        out, self.last_records, self.last_residuals = self.track(
            depth, code, _volume(tsdf), _volume(weight), array_offset,
            np.zeros(6) if twist is None else twist6(twist), voxel_size, narrow_band_width_voxels, residuals,
            None if colour is None else _volume(colour), device_colour_image(colour_image))
        return out
