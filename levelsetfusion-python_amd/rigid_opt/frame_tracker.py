"""What the two frame-to-model trackers over a live depth image share (ProjectiveIcp3d, PointToSdf3d): the settings
of the levels, the distance gate, the photometric term and the loss with their checks, the results the last call leaves
on the tracker, and the upload of a frame's colour image."""
import numpy as np
import torch

from .. import device_icp
from .depth_pyramid import DepthPyramid
from .intensity_pyramid import IntensityPyramid
from .robust_loss import RobustLoss


def device_colour_image(colour_image):
    """a frame's colour image (uint8 (H, W, 3), numpy or tensor) as a device tensor; None stays None"""
    if colour_image is None:
        return None
    if isinstance(colour_image, torch.Tensor):
        return colour_image if colour_image.is_cuda else colour_image.to("cuda")
    a = np.asarray(colour_image)
    if a.dtype != np.uint8:
        raise ValueError("colour_image must be uint8, got %s" % a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class FrameTracker:
    def __init__(self, camera, iterations, strides, max_distance, pyramid, photometric_weight,
                 max_intensity_difference, intensity_pyramid, robust):
        """the settings both trackers take, as their own constructors describe them"""
        self.camera = camera
        if pyramid is not None and not isinstance(pyramid, DepthPyramid):
            raise ValueError("pyramid must be a rigid_opt.DepthPyramid or None, got %r" % (pyramid,))
        self.pyramid = pyramid
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
        self.last_intensity_residuals = None  # r_I of the last call with a photometric_weight and residuals=True
        self.last_pyramid = None  # the PyramidLevels of the last call with a pyramid

    def _keep(self, run):
        """the five values of a device run (twist, records, residuals, intensity residuals, weights) as track()
        returns them: the last two stay on the tracker when the configuration has them"""
        out, records, res, intensity, weights = run
        if self.photometric_weight is not None:
            self.last_intensity_residuals = intensity
        if self.robust is not None:
            self.last_weights = weights
        return out, [device_icp.unpack_record(r) for r in records], res
