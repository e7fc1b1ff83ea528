"""DepthPyramid: the measurement stage KinectFusion puts in front of ICP, which the reference does not have -- a
bilateral filter on the live depth, depth-gated 2 x 2 means for the coarser levels and forward-difference normals at
every level.  INTEGRATION.md section 3 ("Depth pyramid") defines the arithmetic and tests/depth_pyramid_restatement.py
restates it.  build() is levels + 1 launches of csrc/lsf_depth_pyramid.hip (device_depth_pyramid.depth_pyramid) with
no host wait; ProjectiveIcp3d(pyramid=...) and SequenceFusion3d(icp_pyramid=...) track against its output."""
from collections import namedtuple

from .. import device_depth_pyramid as P
from ..device_core import require_gpu
from ..tsdf.generation import device_depth

__all__ = ["DepthPyramid", "PyramidLevels"]

# depth: one float32 (h, w) device tensor per level, metres, 0 where invalid; normals: (h, w, 3) camera-space unit
# normals, 0 where none; intrinsics: (fx, fy, cx, cy) per level; buffers: the two contiguous device buffers the views
# share, levels back to back (device_icp.icp_run_pyramid's inputs)
PyramidLevels = namedtuple("PyramidLevels", ["depth", "normals", "intrinsics", "buffers"])


class DepthPyramid:
    def __init__(self, levels=P.LEVELS, radius=P.RADIUS, sigma_space=P.SIGMA_SPACE, sigma_range=P.SIGMA_RANGE,
                 depth_gate=P.DEPTH_GATE):
        """levels: 1 .. ICP_MAX_LEVELS; radius: the filter's half window in pixels, 0 (no filter) .. PYRAMID_MAX_RADIUS;
        sigma_space (pixels) and sigma_range (metres): the filter's Gaussians; depth_gate (metres): the largest depth
        step a 2 x 2 mean or a normal spans"""
        (self.levels, self.radius, self.sigma_space, self.sigma_range,
         self.depth_gate) = P.settings(levels, radius, sigma_space, sigma_range, depth_gate)

    def settings(self):
        return dict(levels=self.levels, radius=self.radius, sigma_space=self.sigma_space,
                    sigma_range=self.sigma_range, depth_gate=self.depth_gate)

    def build(self, live_depth, camera):
        """the pyramid of a depth image (uint16 / float32 / float64, numpy or device, scaled by the camera's
        depth_unit_ratio), enqueued without waiting: a PyramidLevels"""
        require_gpu()
        return self.build_device(*device_depth(live_depth), camera)

    def build_device(self, depth, code, camera):
        """build() of a device depth image and its LSF_DEPTH_* code (tsdf.generation.device_depth)"""
        d, n = P.depth_pyramid(depth, code, camera, **self.settings())
        shapes = P.level_shapes(tuple(depth.shape), self.levels)
        return PyramidLevels(P.split_levels(d, shapes), P.split_levels(n, shapes),
                             P.level_intrinsics(camera, self.levels), (d, n))
