"""Sdf2SdfOptimizer3d: rigid 6-DoF alignment of a live depth frame to a canonical one after SDF-2-SDF, on 3-D TSDF
volumes.  The reference has no 3-D tracker; this is its 2-D loop (rigid_opt/sdf_2_sdf_optimizer2d.py:60-137) lifted to
3-D with the same dtypes, the twist (t_x, t_y, t_z, r_x, r_y, r_z) in twist_vector_to_matrix3d's layout
(INTEGRATION.md section 3 defines the arithmetic).

optimize() generates the canonical volume once, then enqueues the whole loop on the GPU (device_rigid.rigid_run_3d:
`iteration` fused launches of csrc/lsf_rigid3d.hip and one finishing launch, one copy back).  Every iteration
regenerates the live volume under twist_vector_to_matrix3d of the float32-rounded twist, takes the twist gradient
g = [grad ; p x grad] / voxel_size, accumulates in float64 A = sum g g^T (products float32),
b = sum ((c - l) + g . twist) g and the energy 0.5 sum (c [c > -eta] - l [l > -eta])^2, then sets
twist += rate (A^-1 b - twist).

Singular A: as in the 2-D tracker, the update is skipped and "SINGULAR MATRIX!" printed when A has a non-finite entry or
its float64 LU with partial pivoting meets an exact zero pivot.  In 3-D this is common: a flat wall facing the camera
leaves the t_x, t_y and r_z columns of A zero.  A nearly singular A is inverted.

Verbosity prints come from the per-iteration records after the call, in the 2-D tracker's text and order with six
components; the records stay on the optimizer as `last_records` (a list of dicts: twist_star, twist, energy, matrix_a,
vector_b, skipped)."""
from .. import device_rigid
from ..tsdf.generation import FilteringMethod, device_depth
from . import sdf_2_sdf_optimizer2d
from .sdf_2_sdf_optimizer2d import (BOLD_LIGHT_CYAN, BOLD_YELLOW, RESET, SKIP_SINGULAR,  # noqa: F401
                                    Sdf2SdfOptimizerBase)
from .sdf_2_sdf_visualizer import Sdf2SdfVisualizer


def unpack_record(r):
    return sdf_2_sdf_optimizer2d.unpack_record(r, 6)


class Sdf2SdfOptimizer3d(Sdf2SdfOptimizerBase):
    def optimize(self, data_to_use, voxel_size=0.004, narrow_band_width_voxels=20., iteration=60, eta=.01):
        """the (6, 1) float64 twist aligning data_to_use's live depth frame to its canonical one"""
        canonical_field = data_to_use.generate_3d_canonical_field(narrow_band_width_voxels=narrow_band_width_voxels,
                                                                  method=FilteringMethod.NONE, as_tensor=True)
        depth, depth_code = device_depth(data_to_use.live_depth_image())
        self.visualizer = Sdf2SdfVisualizer(parameters=self.visualization_parameters,
                                            field_size=canonical_field.shape[0])
        twist, records = device_rigid.rigid_run_3d(
            canonical_field, depth, depth_code, data_to_use.depth_camera, data_to_use.offset, iteration, self.rate,
            eta, voxel_size, 0.004, narrow_band_width_voxels)
        self.last_records = [unpack_record(r) for r in records]
        self._report(self.last_records)
        del self.visualizer
        return twist.reshape(6, 1)
