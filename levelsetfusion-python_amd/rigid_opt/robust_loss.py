"""RobustLoss: the weights of the iteratively reweighted ICP solve.  INTEGRATION.md section 3 ("Robust ICP") defines the
arithmetic and tests/robust_icp_restatement.py restates it.  Every pair's rows of the normal equations are scaled by a
weight of its own residual at the current twist: with a = |r| and the scale s,
    "huber"  w = 1 where a <= s, s / a beyond it: an outlier pulls with a constant force instead of its residual
    "tukey"  w = (1 - (r / s)^2)^2 where a < s, 0 from s on: an outlier does not pull at all
The geometric term takes `scale` (metres), the photometric term `intensity_scale` (units of Y, 0 .. 1) on its unscaled
residual; math.inf leaves a term least squares.  The gates of the tracker (max_distance, max_normal_angle,
max_intensity_difference) stay in front of the weights.  Tukey has a basin: a scale below the residuals of the starting
pose gives every pair the weight 0, the solve is singular, every iteration is skipped and the twist stays where it
started.  ProjectiveIcp3d(robust=) and SequenceFusion3d(icp_robust=)
take one; the kernel is csrc/lsf_icp.hip's RobustSource (device_icp.icp_run_robust, icp_run_pyramid_robust)."""
import math

from .. import _lib

__all__ = ["RobustLoss"]

_KINDS = {"huber": _lib.ICP_LOSS_HUBER, "tukey": _lib.ICP_LOSS_TUKEY}


class RobustLoss:
    def __init__(self, kind, scale, intensity_scale=math.inf):
        """kind: "huber" or "tukey"; scale: of the geometric residual in metres, > 0 (inf: least squares);
        intensity_scale: of the intensity residual in units of Y, > 0 (inf: that term stays least squares).  scale has
        no default: it follows the sensor's noise and the size of the motion to reject, and no value is right across
        sensors"""
        if kind not in _KINDS:
            raise ValueError("kind must be 'huber' or 'tukey', got %r" % (kind,))
        self.kind, self.code = kind, _KINDS[kind]
        self.scale, self.intensity_scale = float(scale), float(intensity_scale)
        for name, value in (("scale", self.scale), ("intensity_scale", self.intensity_scale)):
            if not value > 0:  # NaN is not > 0
                raise ValueError("%s must be positive (inf allowed), got %r" % (name, value))

    def __repr__(self):
        return "RobustLoss(%r, %r, %r)" % (self.kind, self.scale, self.intensity_scale)
