"""levelsetfusion-python_amd -- MI355X-native non-rigid level-set (KillingFusion / SobolevFusion style) optimizers.

Drop-in for the numpy path of Algomorph/LevelSetFusion-Python's warp-field gradient descent:
    SlavchevaOptimizer2d(...).optimize(live_field, canonical_field)
    HierarchicalOptimizer2d(...).optimize(canonical_field, live_field)
plus their 3-D generalisations, the SDF-2-SDF rigid 2-D tracker rigid_opt.Sdf2SdfOptimizer2d and its 6-DoF 3-D
form rigid_opt.Sdf2SdfOptimizer3d, the point-to-plane ICP tracker rigid_opt.ProjectiveIcp3d, the point-to-SDF tracker
rigid_opt.PointToSdf3d, and
fusion.SequenceFusion3d, which tracks a depth sequence against a weighted canonical TSDF (fusion.CanonicalVolume) and fuses every frame into it; the model's surface comes out as a triangle mesh
(CanonicalVolume.extract_mesh, written by mesh_io.write_ply).  Host code is Python; device buffers are
PyTorch-ROCm tensors; every per-voxel operation is a hand-written HIP kernel (gfx950) behind the C ABI in include/lsf_hip.h.  There is no CPU
execution path: importing the package without liblsf_hip.so raises.

The directory name contains a hyphen, so import it through the loader module `levelsetfusion_python_amd`
at the repository root.
"""
from . import _lib  # noqa: F401  (raises ImportError loudly when the HIP library is missing)
from .nonrigid_opt.hierarchical.hierarchical_optimizer2d import HierarchicalOptimizer2d
from .nonrigid_opt.hierarchical.hierarchical_optimizer3d import HierarchicalOptimizer3d
from .nonrigid_opt.slavcheva.slavcheva_optimizer2d import (AdaptiveLearningRateMethod, ComputeMethod,
                                                           SlavchevaOptimizer2d)
from .nonrigid_opt.slavcheva.slavcheva_optimizer3d import SlavchevaOptimizer3d
from .nonrigid_opt.slavcheva.data_term import DataTermMethod
from .nonrigid_opt.slavcheva.smoothing_term import SmoothingTermMethod
from .nonrigid_opt.slavcheva.sobolev_filter import generate_1d_sobolev_kernel
from .nonrigid_opt.slavcheva import data_term, level_set_term, smoothing_term
from . import rigid_opt
from .math_utils import transformation
from .rigid_opt import (sdf_2_sdf_optimizer2d, sdf_2_sdf_optimizer3d, sdf_2_sdf_visualizer, sdf_generation,
                        sdf_gradient_field)
from .rigid_opt.sdf_2_sdf_optimizer2d import Sdf2SdfOptimizer2d
from .rigid_opt.sdf_2_sdf_optimizer3d import Sdf2SdfOptimizer3d
from .rigid_opt.projective_icp3d import ProjectiveIcp3d
from .rigid_opt.point_to_sdf3d import PointToSdf3d
from . import fusion, mesh_io
from .fusion import CanonicalVolume, DepthConfidence, SequenceFusion3d

__all__ = ["HierarchicalOptimizer2d", "HierarchicalOptimizer3d", "SlavchevaOptimizer2d", "SlavchevaOptimizer3d",
           "ComputeMethod", "AdaptiveLearningRateMethod", "DataTermMethod", "SmoothingTermMethod",
           "generate_1d_sobolev_kernel", "data_term", "smoothing_term", "level_set_term", "rigid_opt",
           "transformation", "Sdf2SdfOptimizer2d", "Sdf2SdfOptimizer3d", "ProjectiveIcp3d", "PointToSdf3d", "fusion",
           "CanonicalVolume",
           "SequenceFusion3d", "DepthConfidence", "mesh_io"]
