"""DepthConfidence: the settings of the per-pixel confidence image that weights a frame's fusion (the package's
docstring has the rule)."""
from .. import device_depth_confidence
from ..device_core import require_gpu
from ..rigid_opt.depth_pyramid import DepthPyramid
from ..tsdf.generation import device_depth


def _filter_settings(pyramid):
    """what decides a pyramid's level 0: the filter and the normals' gate"""
    return pyramid.radius, pyramid.sigma_space, pyramid.sigma_range, pyramid.depth_gate


class DepthConfidence:
    """the settings of the per-pixel confidence image c = |n . r| min(1, (reference_depth / z)^2)
    (device_depth_confidence.depth_confidence).  reference_depth: metres, finite and > 0, the depth up to which a
    frontal pixel counts fully; pyramid: a rigid_opt.DepthPyramid whose filter settings give the level-0 depth and
    normals (its levels are not used), DepthPyramid()'s own by default."""

    def __init__(self, reference_depth=device_depth_confidence.REFERENCE_DEPTH, pyramid=None):
        self.reference_depth = device_depth_confidence.checked_reference_depth(reference_depth)
        if pyramid is not None and not isinstance(pyramid, DepthPyramid):
            raise ValueError("pyramid must be a rigid_opt.DepthPyramid or None, got %r" % (pyramid,))
        self.pyramid = DepthPyramid() if pyramid is None else pyramid

    def shares(self, pyramid):
        """whether level 0 of `pyramid` (a DepthPyramid or None) is the one this confidence is computed from"""
        return pyramid is not None and _filter_settings(pyramid) == _filter_settings(self.pyramid)

    def from_levels(self, levels, camera):
        """the float32 (H, W) device weight image of a built pyramid's level 0 (a PyramidLevels), enqueued"""
        return device_depth_confidence.depth_confidence(levels.depth[0], levels.normals[0], camera,
                                                        self.reference_depth)

    def build_device(self, depth, code, camera):
        """the weight image of a device depth image and its LSF_DEPTH_* code: a one-level pyramid, then from_levels"""
        settings = dict(self.pyramid.settings(), levels=1)
        return self.from_levels(DepthPyramid(**settings).build_device(depth, code, camera), camera)

    def build(self, depth_image, camera):
        """build_device of a depth image (uint16 / float32 / float64, numpy or device)"""
        require_gpu()
        return self.build_device(*device_depth(depth_image), camera)
