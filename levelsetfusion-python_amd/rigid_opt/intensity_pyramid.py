"""IntensityPyramid: what the photometric term needs to run on a DepthPyramid -- the frame's intensity and the
prediction's at every level of the depth pyramid.  INTEGRATION.md section 3 ("Intensity pyramid") defines the arithmetic
and tests/pyramid_photometric_restatement.py restates it.  Each build is `levels` launches of
csrc/lsf_intensity_pyramid.hip (device_intensity_pyramid.intensity_pyramid) with no host wait;
ProjectiveIcp3d(pyramid=, intensity_pyramid=, photometric_weight=) and SequenceFusion3d(icp_intensity_pyramid=) track
against a pair of them."""
from collections import namedtuple

from .. import device_intensity_pyramid as P
from ..device_depth_pyramid import level_shapes, split_levels

__all__ = ["IntensityPyramid", "IntensityLevels"]

# intensity: one float32 (h, w) device tensor per level, Y in 0..1, NaN where the prediction has no colour; buffer: the
# contiguous device buffer the views share, levels back to back (device_icp.icp_run_pyramid_photometric's input)
IntensityLevels = namedtuple("IntensityLevels", ["intensity", "buffer"])


class IntensityPyramid:
    def __init__(self, levels=3):
        """levels: 1 .. ICP_MAX_LEVELS, the levels of the DepthPyramid it goes with"""
        self.levels = P.checked_levels(levels)

    def _build(self, image, source):
        buffer = P.intensity_pyramid(image, source, self.levels)
        return IntensityLevels(split_levels(buffer, level_shapes(tuple(image.shape[:2]), self.levels)), buffer)

    def build_device(self, colour_image):
        """the live pyramid of a frame's uint8 (H, W, 3) device colour image, enqueued without waiting: level 0 is
        Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 of the bytes"""
        return self._build(colour_image, "colour")

    def build_prediction(self, prediction_colour):
        """the prediction's pyramid of the float32 (H, W, 4) device image of CanonicalVolume.raycast(..., colours=True),
        enqueued without waiting: level 0 is its Y channel bit for bit, NaN where there is no colour"""
        return self._build(prediction_colour, "prediction")
