"""SDF-2-SDF rigid tracking (reference rigid_opt/): Sdf2SdfOptimizer2d, its datasets and calculate_gradient_wrt_twist,
and their 6-DoF 3-D generalisation Sdf2SdfOptimizer3d and calculate_gradient_wrt_twist_3d; ProjectiveIcp3d tracks a depth
frame against a ray-cast prediction by point-to-plane ICP, optionally over a DepthPyramid of the live frame (bilateral
filter, 2 x 2 means, normals) and, with an IntensityPyramid of the frame's and the prediction's colour, with the
photometric term at every level; a RobustLoss scales every pair by a Huber or Tukey weight of its own residual; PointToSdf3d
tracks a depth frame against the canonical TSDF itself, point to signed distance, without a prediction.  The
optimizers' whole loops run on the GPU (csrc/lsf_rigid.hip, csrc/lsf_rigid3d.hip, csrc/lsf_icp.hip,
csrc/lsf_depth_pyramid.hip, csrc/lsf_intensity_pyramid.hip, csrc/lsf_point_sdf.hip)."""
from .depth_pyramid import DepthPyramid  # noqa: F401
from .intensity_pyramid import IntensityPyramid  # noqa: F401
from .robust_loss import RobustLoss  # noqa: F401
from .projective_icp3d import ProjectiveIcp3d  # noqa: F401
from .point_to_sdf3d import PointToSdf3d  # noqa: F401
