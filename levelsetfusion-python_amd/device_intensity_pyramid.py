"""Torch-facing wrapper of the intensity pyramids (include/lsf_hip.h: lsf_intensity_pyramid): level 0 from a frame's
uint8 colour image (Y of its bytes) or from a ray-cast colour image (its Y channel, bit for bit), every coarser level the
mean of 2 x 2 blocks whose four values are finite, NaN otherwise.  Every argument is checked on the host before the
launches; a call enqueues `levels` launches with no host wait.  The public interface is rigid_opt.IntensityPyramid;
device_icp.icp_run_pyramid_photometric tracks against two of its outputs."""
import ctypes

import torch

from . import _lib
from ._lib import IntensityPyramidParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_depth_pyramid import level_shapes
from .device_raycast import image_extents

SOURCES = {"colour": (_lib.INTENSITY_SOURCE_COLOUR, torch.uint8, 3),
           "prediction": (_lib.INTENSITY_SOURCE_PREDICTION, torch.float32, 4)}


def checked_levels(levels):
    levels = int(levels)
    if not 1 <= levels <= _lib.ICP_MAX_LEVELS:
        raise ValueError("levels must be 1 to %d, got %d" % (_lib.ICP_MAX_LEVELS, levels))
    return levels


def params(image_shape, levels, source):
    """the lsf_intensity_pyramid_params of a call, after the host checks; source: "colour" or "prediction" """
    if source not in SOURCES:
        raise ValueError("source must be one of %s, got %r" % (sorted(SOURCES), source))
    p = IntensityPyramidParams()
    p.height, p.width = image_extents(image_shape)
    p.levels = checked_levels(levels)
    level_shapes((p.height, p.width), p.levels)
    p.source = SOURCES[source][0]
    return p


def intensity_pyramid(image, source, levels):
    """the pyramid of a contiguous device image, enqueued: one contiguous float32 device buffer (pixels,) holding the
    levels back to back, level 0 first.  source "colour": a uint8 (H, W, 3) image; "prediction": the float32 (H, W, 4)
    image of device_raycast.raycast(..., colour=).  `levels` launches, no host wait."""
    require_gpu()
    if source not in SOURCES:
        raise ValueError("source must be one of %s, got %r" % (sorted(SOURCES), source))
    _, dtype, channels = SOURCES[source]
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.is_contiguous() and image.dtype == dtype and
            image.dim() == 3 and image.shape[2] == channels):
        raise ValueError("a %s image must be a contiguous %s (H, W, %d) device tensor" % (source, dtype, channels))
    p = params(tuple(image.shape[:2]), levels, source)
    pixels = sum(h * w for h, w in level_shapes((p.height, p.width), p.levels))
    out = torch.empty(pixels, dtype=torch.float32, device=image.device)
    check(lib.lsf_intensity_pyramid(ctypes.c_void_p(image.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                    ctypes.byref(p), stream_ptr()), "lsf_intensity_pyramid")
    return out
