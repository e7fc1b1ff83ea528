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

With robust (a RobustLoss) each pair's rows are scaled by the Huber or Tukey weight of its own residual at `scale`
(metres; intensity_scale is not used); the records carry weight_sum and outliers and `last_weights` keeps the weight
image beside `last_residuals`.  On a clean scene it is not more accurate than ProjectiveIcp3d; what it saves is the
ray-cast of the prediction (profiles/point_sdf_cost.md)."""
import numpy as np
import torch

from .. import device_icp, device_point_sdf
from ..device_core import require_gpu
from ..device_rigid import twist6
from .robust_loss import RobustLoss
from ..tsdf.generation import device_depth

__all__ = ["PointToSdf3d"]


def _volume(x):
    """a model array (numpy or tensor) as a contiguous float32 device tensor"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to("cuda").to(torch.float32).contiguous()


class PointToSdf3d:
    def __init__(self, camera, iterations=device_icp.ITERATIONS, strides=device_icp.STRIDES,
                 max_distance=device_icp.MAX_DISTANCE, robust=None):
        """iterations and strides: one entry per level, coarse first; max_distance: the gate on |r| in metres, > 0;
        robust: None (least squares) or a RobustLoss"""
        self.camera = camera
        self.iterations, self.strides = device_icp.levels(iterations, strides)
        if not float(max_distance) > 0:
            raise ValueError("max_distance must be positive")
        self.max_distance = float(max_distance)
        if robust is not None and not isinstance(robust, RobustLoss):
            raise ValueError("robust must be a rigid_opt.RobustLoss or None, got %r" % (robust,))
        self.robust = robust
        self.last_records = []
        self.last_residuals = None
        self.last_weights = None  # the weight image of the last robust call with residuals=True

    def track(self, depth, code, tsdf, weight, array_offset, twist, voxel_size=0.004, narrow_band_width_voxels=20,
              residuals=False):
        """optimize() on device inputs (tsdf.generation.device_depth's depth and LSF_DEPTH_* code, the model's float32
        device tsdf and weight): (final twist, the unpacked records, the residual image or None); the weight image is
        kept as `last_weights`"""
        out, records, res, self.last_weights = device_point_sdf.point_sdf_run(
            tsdf, weight, depth, code, self.camera, array_offset, twist, voxel_size, narrow_band_width_voxels,
            self.iterations, self.strides, self.max_distance, self.robust, residuals)
        return out, [device_icp.unpack_record(r) for r in records], res

    def optimize(self, depth_image, tsdf, weight, array_offset, twist=None, voxel_size=0.004,
                 narrow_band_width_voxels=20, residuals=False):
        """the float64 (6,) twist of the live depth frame (uint16 / float32 / float64, numpy or device, scaled by the
        camera's depth_unit_ratio) against the model tsdf / weight ((Z, Y, X), numpy or device; a CanonicalVolume's),
        started from twist (zero by default).  residuals=True also keeps the last iteration's residual image (float32
        device tensor, NaN without a pair) as `last_residuals`, and with a loss the weight image as `last_weights`."""
        require_gpu()
        depth, code = device_depth(depth_image)
        out, self.last_records, self.last_residuals = self.track(
            depth, code, _volume(tsdf), _volume(weight), array_offset,
            np.zeros(6) if twist is None else twist6(twist), voxel_size, narrow_band_width_voxels, residuals)
        return out
