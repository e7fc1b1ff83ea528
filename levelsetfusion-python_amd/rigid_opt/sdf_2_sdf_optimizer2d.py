"""Sdf2SdfOptimizer2d (reference rigid_opt/sdf_2_sdf_optimizer2d.py:60-137): rigid 2-D alignment of a live depth row
to a canonical one after SDF-2-SDF, the twist (t_x, t_z, theta) found by Gauss-Newton steps damped by `rate`.

optimize() generates the canonical field once, then enqueues the whole loop on the GPU (device_rigid.rigid_run:
`iteration` fused launches and one finishing launch, one copy back).  Every iteration regenerates the live field
under twist_vector_to_matrix3d([t0, 0, t1, 0, t2, 0]) of the float32-rounded twist, takes the twist gradient g and
accumulates in float64 A = sum g g^T (products float32), b = sum ((c - l) + g . twist) g and the energy
0.5 sum (c [c > -eta] - l [l > -eta])^2, then sets twist += rate (A^-1 b - twist).  The sums are tree reductions, so A, b
and the energy differ from the reference's sequential loop in the last bits (tests/test_gpu_rigid.py states the
tolerances); the per-voxel values are the reference's to the bit.

Singular A: the reference skips the update when np.linalg.cond(A) is not finite -- a non-finite entry, or a smallest
singular value of exactly 0, as for A == 0 or an A with a zero row and column (a twist-gradient component that is 0 at
every voxel, e.g. a flat wall facing the camera).  The device skips when A has a non-finite entry or its float64 LU with
partial pivoting meets an exact zero pivot, which covers those cases, and "SINGULAR MATRIX!" is printed after the call.
A nearly singular A is inverted, as in the reference.  The one documented difference: an exactly singular A with no
zero row or column, whose LU pivots happen to be exact zeros but whose singular values LAPACK returns as tiny non-zero
numbers, is skipped here, where the reference would call np.linalg.inv on it.

Verbosity prints come from the per-iteration records after the call, in the reference's text and order; the records
stay on the optimizer as `last_records` (a list of dicts: twist_star, twist, energy, matrix_a, vector_b, skipped)."""

from .. import device_rigid
from ..tsdf.generation import FilteringMethod, device_depth
from .sdf_2_sdf_visualizer import Sdf2SdfVisualizer

BOLD_YELLOW = "\033[33;1;m"
BOLD_LIGHT_CYAN = "\033[36;1;m"
RESET = "\033[0m"

SKIP_NONE, SKIP_SINGULAR = 0, 1


def unpack_record(r, n=3):
    """one host record of an n-DoF tracker (n = 3 here, 6 in sdf_2_sdf_optimizer3d) as a dict; the layout of
    csrc/lsf_rigid_solve.h: [twist* (n)][twist (n)][energy][A (n x n)][b (n)][skipped]"""
    a = 2 * n + 1
    b = a + n * n
    return {"twist_star": r[0:n].reshape(n, 1).copy(), "twist": r[n:2 * n].reshape(n, 1).copy(),
            "energy": float(r[2 * n]), "matrix_a": r[a:b].reshape(n, n).copy(),
            "vector_b": r[b:b + n].reshape(n, 1).copy(), "skipped": int(r[b + n])}


class Sdf2SdfOptimizerBase:
    """what the 2-D and the 6-DoF optimizer share: the constructor and the verbosity prints from the records"""

    class VerbosityParameters:
        """what optimize() prints per iteration"""

        def __init__(self, print_max_warp_update=False, print_iteration_energy=False):
            self.print_max_warp_update = print_max_warp_update
            self.print_iteration_energy = print_iteration_energy
            self.per_iteration_flags = [self.print_max_warp_update,
                                        self.print_iteration_energy]
            self.print_per_iteration_info = any(self.per_iteration_flags)

    def __init__(self, rate=0.5, verbosity_parameters=None, visualization_parameters=None):
        self.rate = rate
        self.verbosity_parameters = verbosity_parameters if verbosity_parameters else self.VerbosityParameters()
        self.visualization_parameters = visualization_parameters if visualization_parameters else \
            Sdf2SdfVisualizer.Parameters()
        self.visualizer = None
        self.last_records = []

    def _report(self, records):
        v = self.verbosity_parameters
        for iteration_count, rec in enumerate(records):
            if v.print_per_iteration_info:
                print("%s[ITERATION %d COMPLETED]%s" % (BOLD_LIGHT_CYAN, iteration_count, RESET), end="")
                if v.print_iteration_energy:
                    print(" energy: %f" % rec["energy"], end="")
                    print("")
            if rec["skipped"] == SKIP_SINGULAR:
                print("%sSINGULAR MATRIX!%s" % (BOLD_YELLOW, RESET))
                continue
            if v.print_max_warp_update:
                ts, tw = rec["twist_star"].reshape(-1), rec["twist"].reshape(-1)
                print("optimal twist: %s, twist: %s" % (", ".join("%f" % x for x in ts),
                                                         ", ".join("%f" % x for x in tw)), end="")
                print("")


class Sdf2SdfOptimizer2d(Sdf2SdfOptimizerBase):
    def optimize(self, data_to_use, voxel_size=0.004, narrow_band_width_voxels=20., iteration=60, eta=.01):
        """the (3, 1) float64 twist aligning data_to_use's live depth row to its canonical one"""
        canonical_field = data_to_use.generate_2d_canonical_field(narrow_band_width_voxels=narrow_band_width_voxels,
                                                                  method=FilteringMethod.NONE, as_tensor=True)
        depth, depth_code = device_depth(data_to_use.live_depth_image())
        self.visualizer = Sdf2SdfVisualizer(parameters=self.visualization_parameters,
                                            field_size=canonical_field.shape[0])
        twist, records = device_rigid.rigid_run(
            canonical_field, depth, depth_code, data_to_use.depth_camera, data_to_use.image_pixel_row,
            data_to_use.offset, iteration, self.rate, eta, voxel_size, 0.004, narrow_band_width_voxels)
        self.last_records = [unpack_record(r) for r in records]
        self._report(self.last_records)
        del self.visualizer
        return twist.reshape(3, 1)
