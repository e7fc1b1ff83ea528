"""ctypes binding of liblsf_hip.so (C ABI: include/lsf_hip.h).

There is NO fallback: if the HIP library is missing, importing this module raises.  The numpy oracle under
oracle/ is test infrastructure and is never imported from the package.
"""
import ctypes
import os

# torch FIRST: the PyTorch-ROCm wheel ships its own libamdhip64.so; liblsf_hip.so must bind to that already-loaded
# HIP runtime (same soname), otherwise the process ends up with two runtimes and launches on torch's streams fail
# with hipErrorNoDevice.
import torch  # noqa: F401

from ._build import LIB_PATH

c_float_p = ctypes.c_void_p  # device pointers travel as integers (tensor.data_ptr())

MAX_KERNEL_TAPS = 31
ABI_VERSION = 4
# _build.abi_hash() of the include/lsf_hip.h THIS binding was written against (structures and prototypes below mirror
# it).  The library carries the hash of the header it was compiled from (lsf_abi_hash()); a mismatch is refused at load
# time, and tests/test_cabi_and_host.py checks this constant against the header in the tree -- so editing a struct or
# a prototype in the header without revisiting the binding fails on the CPU, and a stale or variant .so cannot be
# called through structures of another shape.
HEADER_ABI_HASH = "d176ab41b23512aa"

ERRORS = {-1: "LSF_ERR_BAD_ARGUMENT", -2: "LSF_ERR_BAD_DIMS", -3: "LSF_ERR_KERNEL_TOO_LONG",
          -4: "LSF_ERR_RCCL_UNAVAILABLE", -5: "LSF_ERR_RCCL_FAILED", -6: "LSF_ERR_NOT_RESIDENT"}

SMOOTHING_TIKHONOV, SMOOTHING_KILLING = 0, 1
DATA_BASIC, DATA_THRESHOLDED_FDM = 0, 2
ENERGY_NONE, ENERGY_DIRECT, ENERGY_VECTORIZED = 0, 1, 2
GATE_HIERARCHICAL, GATE_SLAVCHEVA, GATE_OPEN = 0, 1, 2


class Grid(ctypes.Structure):
    _fields_ = [("dims", ctypes.c_int32), ("nz", ctypes.c_int32), ("ny", ctypes.c_int32), ("nx", ctypes.c_int32),
                ("z_begin", ctypes.c_int32), ("z_end", ctypes.c_int32), ("z_global_offset", ctypes.c_int32),
                ("y_global_offset", ctypes.c_int32), ("energy_z_begin", ctypes.c_int32), ("energy_z_end", ctypes.c_int32),
                ("ny_global", ctypes.c_int32), ("energy_y_begin", ctypes.c_int32), ("energy_y_end", ctypes.c_int32)]


BAND_ALL, BAND_INTERIOR, BAND_BOUNDARY = 0, 1, 2
RECORD_SLOTS = 8


class RecordSlot(ctypes.Structure):
    _fields_ = [("max_packed", ctypes.c_uint64), ("data_energy", ctypes.c_double),
                ("smoothing_energy", ctypes.c_double), ("level_set_energy", ctypes.c_double),
                ("pad", ctypes.c_uint64 * 508)]


class IterationRecord(ctypes.Structure):
    """8 partial records 4 KiB apart (one per XCD: separate memory channels); value = max over the slots' max_packed,
    sum over their energies"""
    _fields_ = [("slot", RecordSlot * RECORD_SLOTS)]


RECORD_BYTES = ctypes.sizeof(IterationRecord)  # 32768
SLOT_WORDS = ctypes.sizeof(RecordSlot) // 8    # 512


class Gate(ctypes.Structure):
    _fields_ = [("prev_record", ctypes.c_void_p), ("mode", ctypes.c_int32), ("a", ctypes.c_float),
                ("b", ctypes.c_float)]


SLAB_LAUNCH, SLAB_EXCHANGE, SLAB_EXCHANGE_DEFERRED, SLAB_RESUME = 0, 1, 2, 3


class SlabLayoutC(ctypes.Structure):
    _fields_ = [("nz", ctypes.c_int32), ("ny", ctypes.c_int32), ("nx", ctypes.c_int32), ("z_begin", ctypes.c_int32),
                ("z_end", ctypes.c_int32), ("halo", ctypes.c_int32), ("lo_rank", ctypes.c_int32),
                ("hi_rank", ctypes.c_int32)]


class SlabPart(ctypes.Structure):
    _fields_ = [("grid", Grid), ("band_list", ctypes.c_void_p * 2), ("band_count", ctypes.c_int64 * 2),
                ("band_subset", ctypes.c_int32 * 2), ("n_lists", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SlabFaces(ctypes.Structure):
    _fields_ = [("send_list", ctypes.c_void_p * 2), ("recv_list", ctypes.c_void_p * 2),
                ("send_msg", ctypes.c_void_p * 2), ("recv_msg", ctypes.c_void_p * 2),
                ("send_count", ctypes.c_int64 * 2), ("recv_count", ctypes.c_int64 * 2)]


class BandBox(ctypes.Structure):
    """lsf_band_box: a 4 x 4 x 4 box of the volume and which of its voxels are INTERIOR band voxels"""
    _fields_ = [("origin", ctypes.c_int32), ("reserved", ctypes.c_int32), ("mask", ctypes.c_uint64)]


class StateRun(ctypes.Structure):
    """lsf_state_run: the buffers of a whole fixed-count call enqueued by the library (lsf_state_run_begin / _finish)"""
    _fields_ = [("live", ctypes.c_void_p), ("canonical", ctypes.c_void_p), ("state", ctypes.c_void_p * 2),
                ("prepare_scratch", ctypes.c_void_p), ("totals_device", ctypes.c_void_p),
                ("totals_host", ctypes.c_void_p), ("grid", Grid), ("sparse_reach", ctypes.c_int32),
                ("second_state_late", ctypes.c_int32), ("box_scratch", ctypes.c_void_p), ("box_all", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


# one energy term on its own (lsf_term_gradient)
TERM_DATA_BASIC, TERM_DATA_THRESHOLDED_FDM, TERM_TIKHONOV, TERM_TIKHONOV_LOCAL, TERM_KILLING, TERM_LEVEL_SET = range(6)
TERM_COPY_IF_ZERO, TERM_IGNORE_IF_ZERO, TERM_INTERLEAVED = 1, 2, 4
SELECT_ALL, SELECT_BAND, SELECT_LIST = 0, 1, 2
TERM_ENERGY_LOCAL, TERM_ENERGY_NP_GRADIENT = 0, 1


class TermParams(ctypes.Structure):
    _fields_ = [("isomorphic_enforcement_factor_f64", ctypes.c_double), ("isomorphic_enforcement_factor", ctypes.c_float),
                ("epsilon", ctypes.c_float), ("scaling_factor", ctypes.c_float), ("term", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class StateRunResult(ctypes.Structure):
    _fields_ = [("max_value", ctypes.c_void_p), ("argmax", ctypes.c_void_p), ("energies3", ctypes.c_void_p),
                ("executed", ctypes.c_void_p), ("final_state", ctypes.c_int32), ("n_lists", ctypes.c_int32),
                ("reach_exceeded", ctypes.c_int32), ("compact_faces", ctypes.c_int32)]


class RunLoop(ctypes.Structure):
    """lsf_run_loop: the loop condition of slavcheva_optimizer2d.py:360-362 for lsf_state_run_finish"""
    _fields_ = [("min_iterations", ctypes.c_int32), ("max_iterations", ctypes.c_int32), ("lower_threshold", ctypes.c_float),
                ("upper_threshold", ctypes.c_float), ("check_interval", ctypes.c_int32), ("reserved", ctypes.c_int32)]


SLAB_MAX_CUTS = 72


class SlabRun(ctypes.Structure):
    """lsf_slab_run: a whole fixed-count call of a z-slab rank enqueued by the library (lsf_slab_run_begin / _finish)"""
    _fields_ = [("base", StateRun), ("layout", SlabLayoutC), ("exchange_interval", ctypes.c_int32),
                ("n_cuts", ctypes.c_int32), ("cut_slices", ctypes.c_int32 * SLAB_MAX_CUTS),
                ("cut_entries", (ctypes.c_int64 * SLAB_MAX_CUTS) * 2), ("out_index_entries", ctypes.c_int64),
                ("out_face_entries", ctypes.c_int64)]


class HierParams(ctypes.Structure):
    _fields_ = [("data_term_amplifier", ctypes.c_float), ("tikhonov_strength", ctypes.c_float),
                ("rate", ctypes.c_float), ("tikhonov_enabled", ctypes.c_int32), ("apply_update", ctypes.c_int32),
                ("compute_energy", ctypes.c_int32), ("previous_max", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("packed_nz", ctypes.c_int32), ("packed_z_global_offset", ctypes.c_int32)]


class SlavchevaParams(ctypes.Structure):
    _fields_ = [("isomorphic_enforcement_factor_f64", ctypes.c_double), ("rate", ctypes.c_float),
                ("data_term_weight", ctypes.c_float), ("smoothing_term_weight", ctypes.c_float),
                ("level_set_term_weight", ctypes.c_float), ("isomorphic_enforcement_factor", ctypes.c_float),
                ("killing_c1", ctypes.c_float), ("smoothing_method", ctypes.c_int32),
                ("data_method", ctypes.c_int32), ("level_set_enabled", ctypes.c_int32),
                ("energy_mode", ctypes.c_int32), ("zero_gradient_on_snap", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class TsdfParams(ctypes.Structure):
    _fields_ = [("intrinsics", ctypes.c_double * 4), ("depth_unit_ratio", ctypes.c_double),
                ("voxel_size", ctypes.c_double), ("narrow_band_half_width", ctypes.c_double),
                ("extrinsic", ctypes.c_float * 16), ("array_offset", ctypes.c_int32 * 3),
                ("image_width", ctypes.c_int32), ("image_height", ctypes.c_int32),
                ("image_y_coordinate", ctypes.c_int32), ("default_value", ctypes.c_float),
                ("intrinsics_are_f32", ctypes.c_int32)]


DEPTH_U16, DEPTH_F32, DEPTH_F64 = 0, 1, 2
RIGID_RECORD_DOUBLES = 24
RIGID_MAX_BLOCKS = 256
RIGID_SCRATCH_BYTES = 2 * RIGID_MAX_BLOCKS * 10 * 8


class RigidParams(ctypes.Structure):
    """lsf_rigid_params: the SDF-2-SDF rigid tracker (lsf_rigid_gradient, lsf_rigid_run)"""
    _fields_ = [("tsdf", TsdfParams), ("array_offset", ctypes.c_double * 3), ("voxel_size", ctypes.c_double),
                ("twist", ctypes.c_double * 3),
                ("rate", ctypes.c_double), ("eta", ctypes.c_float), ("depth_dtype", ctypes.c_int32),
                ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


RIGID3D_RECORD_DOUBLES = 64
RIGID3D_MAX_BLOCKS = 256
RIGID3D_SCRATCH_BYTES = 2 * RIGID3D_MAX_BLOCKS * 28 * 8


class Rigid3dParams(ctypes.Structure):
    """lsf_rigid3d_params: the 6-DoF SDF-2-SDF rigid tracker (lsf_rigid3d_gradient, lsf_rigid3d_run)"""
    _fields_ = [("tsdf", TsdfParams), ("array_offset", ctypes.c_double * 3), ("voxel_size", ctypes.c_double),
                ("twist", ctypes.c_double * 6),
                ("rate", ctypes.c_double), ("eta", ctypes.c_float), ("depth_dtype", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("iterations", ctypes.c_int32)]


FUSION_RECORD_DOUBLES = 8
FUSION_MAX_BLOCKS = 2048
FUSION_SCRATCH_BYTES = FUSION_MAX_BLOCKS * 4 * 8


class FusionParams(ctypes.Structure):
    """lsf_fusion_params: fusion into a canonical TSDF volume (lsf_fusion_integrate_volume, lsf_fusion_integrate_depth)"""
    _fields_ = [("tsdf", TsdfParams), ("twist", ctypes.c_double * 6), ("array_offset", ctypes.c_double * 3),
                ("depth", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("weight", ctypes.c_float), ("max_weight", ctypes.c_float), ("depth_dtype", ctypes.c_int32)]


FUSION_WEIGHTED_SCRATCH_BYTES = FUSION_MAX_BLOCKS * 6 * 8


class FusionWeightedParams(ctypes.Structure):
    """lsf_fusion_weighted_params: weighted depth-mode fusion with carving (lsf_fusion_integrate_depth_weighted)"""
    _fields_ = [("fusion", FusionParams), ("carve", ctypes.c_int32), ("has_pixel_weight", ctypes.c_int32)]


FUSION_COLOUR_SCRATCH_BYTES = FUSION_MAX_BLOCKS * 8 * 8


class FusionColourParams(ctypes.Structure):
    """lsf_fusion_colour_params: weighted depth-mode fusion that also fuses colour (lsf_fusion_integrate_depth_colour)"""
    _fields_ = [("weighted", FusionWeightedParams), ("colour_band", ctypes.c_float)]


FUSION_WARPED_RECORD_DOUBLES = 9
FUSION_WARPED_SCRATCH_BYTES = FUSION_MAX_BLOCKS * 9 * 8


class FusionWarpedParams(ctypes.Structure):
    """lsf_fusion_warped_params: weighted depth-mode fusion through a warp field (lsf_fusion_integrate_depth_warped)"""
    _fields_ = [("colour", FusionColourParams), ("has_colour", ctypes.c_int32)]


class DepthConfidenceParams(ctypes.Structure):
    """lsf_depth_confidence_params: the per-pixel confidence image (lsf_depth_confidence)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "reference_depth")] + \
               [(n, ctypes.c_int32) for n in ("height", "width")]


RAYCAST_STEPS_PER_VOXEL = 2
RAYCAST_TILE = 16


class RaycastParams(ctypes.Structure):
    """lsf_raycast_params: ray-casting the canonical TSDF (lsf_raycast)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "depth_unit_ratio", "voxel_size", "offset_x",
                                               "offset_y", "offset_z", "t_x", "t_y", "t_z", "r_x", "r_y", "r_z")] + \
               [(n, ctypes.c_int32) for n in ("depth", "height", "width", "image_height", "image_width",
                                              "fallback_dtype")]


MESH_TILE = 2048
MESH_MAX_TRIANGLES = 5


class MeshParams(ctypes.Structure):
    """lsf_mesh_params: a triangle mesh of the canonical TSDF (lsf_mesh_count, lsf_mesh_emit)"""
    _fields_ = [(n, ctypes.c_double) for n in ("voxel_size", "offset_x", "offset_y", "offset_z", "iso",
                                               "min_weight")] + \
               [(n, ctypes.c_int32) for n in ("depth", "height", "width")]


MESH_SIMPLIFY_TILE = 256
MESH_SIMPLIFY_SCAN_THREADS = 256
MESH_SIMPLIFY_MAX_ITEMS = 1 << 29
MESH_SIMPLIFY_VERTEX_WORDS = 5
MESH_SIMPLIFY_CLUSTER_WORDS = 4
MESH_SIMPLIFY_FACE_WORDS = 7
MESH_SIMPLIFY_RECORD_FIELDS = ("vertices_in", "faces_in", "invalid_vertices", "invalid_faces", "clusters",
                               "degenerate_faces", "face_groups", "cancelled_groups", "multi_cover_groups",
                               "orphan_clusters", "vertices_out", "faces_out", "table_overflow")
MESH_SIMPLIFY_RECORD_WORDS = len(MESH_SIMPLIFY_RECORD_FIELDS)


class MeshSimplifyParams(ctypes.Structure):
    """lsf_mesh_simplify_params: welding and vertex clustering of a mesh (lsf_mesh_simplify_count, _emit)"""
    _fields_ = [(n, ctypes.c_double) for n in ("cell_size", "origin_x", "origin_y", "origin_z")] + \
               [(n, ctypes.c_int32) for n in ("vertex_count", "face_count", "table_slots", "cluster", "has_normals",
                                              "has_colours")]


MESH_COMPONENTS_TILE = 256
MESH_COMPONENTS_SCAN_THREADS = 256
MESH_COMPONENTS_MAX_BLOCKS = 512
MESH_COMPONENTS_MAX_ITEMS = 1 << 29
MESH_COMPONENTS_VERTEX_WORDS = 12
MESH_COMPONENTS_RECORD_FIELDS = ("vertices_in", "faces_in", "invalid_vertices", "invalid_faces", "components",
                                 "step_cap", "components_kept", "vertices_out", "faces_out")
MESH_COMPONENTS_RECORD_WORDS = len(MESH_COMPONENTS_RECORD_FIELDS)


class MeshComponentsParams(ctypes.Structure):
    """lsf_mesh_components_params: connected components of a mesh (lsf_mesh_components_label, _table, _select, _emit)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("vertex_count", "face_count", "has_normals", "has_colours",
                                              "max_blocks")]


MESH_SMOOTH_TILE = 256
MESH_SMOOTH_SCAN_THREADS = 256
MESH_SMOOTH_MAX_BLOCKS = 512
MESH_SMOOTH_MAX_ITEMS = 1 << 27
MESH_SMOOTH_MAX_SLOTS = 1 << 30
MESH_SMOOTH_MAX_ITERATIONS = 1000
MESH_SMOOTH_VERTEX_WORDS = 4
MESH_SMOOTH_SCALAR_WORDS = 5
MESH_SMOOTH_RECORD_FIELDS = ("vertices_in", "faces_in", "invalid_vertices", "invalid_faces", "edges", "boundary_edges",
                             "nonmanifold_edges", "pinned_vertices", "isolated_vertices", "max_degree", "table_overflow",
                             "nonfinite_out", "zero_normals")
MESH_SMOOTH_RECORD_WORDS = len(MESH_SMOOTH_RECORD_FIELDS)
MESH_SMOOTH_BOUNDARIES = {"fixed": 1, "free": 0}


class MeshSmoothParams(ctypes.Structure):
    """lsf_mesh_smooth_params: Taubin smoothing and vertex normals of a mesh (lsf_mesh_smooth_prepare, _run,
    lsf_mesh_vertex_normals)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("vertex_count", "face_count", "table_slots", "boundary_fixed",
                                              "fresh_record", "iterations", "max_blocks", "reserved")] + \
        [("lam", ctypes.c_double), ("mu", ctypes.c_double)]


ESDF_UNKNOWN = {"free": 0, "occupied": 1}
ESDF_PASS_X, ESDF_PASS_Y, ESDF_PASS_Z, ESDF_PASSES_ALL = 1, 2, 4, 7
ESDF_MAX_DISTANCE = 4096
ESDF_FAR = 0x7fffffff
ESDF_MAX_BLOCKS = 2048
ESDF_BLOCK_ROWS = 4
ESDF_BLOCK_VOXELS = 256
ESDF_RECORD_FIELDS = ("sites", "finite", "max_distance2")
ESDF_RECORD_WORDS = len(ESDF_RECORD_FIELDS)


class EsdfParams(ctypes.Structure):
    """lsf_esdf_params: the Euclidean distance field of the model (lsf_esdf_compute)"""
    _fields_ = [("voxel_size", ctypes.c_double), ("iso", ctypes.c_float), ("min_weight", ctypes.c_float)] + \
               [(n, ctypes.c_int32) for n in ("depth", "height", "width", "max_distance_voxels", "unknown", "passes")]


class VolumeShiftParams(ctypes.Structure):
    """lsf_volume_shift_params: the model shifted by whole voxels (lsf_volume_shift)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("depth", "height", "width", "shift_x", "shift_y", "shift_z")]


VOLUME_SHIFT_MAX_BLOCKS = 2048
VOLUME_SHIFT_BLOCK_ROWS = 4


class VolumeBricksParams(ctypes.Structure):
    """lsf_volume_bricks_params: the window on the brick lattice (lsf_volume_bricks_count / _gather / _scatter)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("depth", "height", "width", "origin_x", "origin_y", "origin_z",
                                              "shift_x", "shift_y", "shift_z")]


VOLUME_BRICK = 8
VOLUME_BRICKS_MAX_BLOCKS = 2048
VOLUME_BRICKS_BLOCK_BRICKS = 4


class RgbdParams(ctypes.Structure):
    """lsf_rgbd_params: the source lens, the ideal output camera and the transform between them (lsf_rgbd_ray_table /
    _register_depth / _rectify_colour)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy")] + [("k", ctypes.c_double * 8)] + \
               [(n, ctypes.c_double) for n in ("out_fx", "out_fy", "out_cx", "out_cy")] + \
               [("rotation", ctypes.c_double * 9), ("translation", ctypes.c_double * 3),
                ("depth_unit_ratio", ctypes.c_double)] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "out_height", "out_width", "max_footprint",
                                              "reserved")]


RGBD_UNDISTORT_ITERATIONS = 10
RGBD_MAX_FOOTPRINT = 16
RGBD_DEFAULT_FOOTPRINT = 8
RGBD_MAX_BLOCKS = 512
RGBD_RECORD_WORDS = 8
RGBD_ZBUFFER_EMPTY = 0x7f800000

class RelocParams(ctypes.Structure):
    """lsf_reloc_params: the frame, the coarse image, the fern table's extents and the database (lsf_reloc_encode /
    lsf_reloc_query)"""
    _fields_ = [(n, ctypes.c_double) for n in ("depth_unit_ratio", "depth_near", "depth_far")] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "coarse_height", "coarse_width", "channels", "ferns",
                                              "decisions", "capacity", "candidates", "harvest", "harvest_differing",
                                              "reserved")]


RELOC_MAX_BLOCKS = 1024
RELOC_MAX_FERNS = 4096
RELOC_MAX_DECISIONS = 8
RELOC_MAX_CANDIDATES = 4
RELOC_MAX_DEPTH = 64.0
RELOC_ENCODE_RECORD_WORDS = 2
RELOC_QUERY_RECORD_WORDS = 12

ICP_MAX_LEVELS = 4
ICP_RECORD_DOUBLES = 64
ICP_MAX_BLOCKS = 256
ICP_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 29 * 8


class IcpParams(ctypes.Structure):
    """lsf_icp_params: projective point-to-plane ICP against the ray-cast prediction (lsf_icp_run)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "depth_unit_ratio", "max_distance")] + \
               [("twist_p", ctypes.c_double * 6)] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "depth_dtype", "levels")] + \
               [("iterations", ctypes.c_int32 * ICP_MAX_LEVELS), ("strides", ctypes.c_int32 * ICP_MAX_LEVELS)]


PYRAMID_MAX_RADIUS = 8
ICP_PYRAMID_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 30 * 8


class DepthPyramidParams(ctypes.Structure):
    """lsf_depth_pyramid_params: the live depth pyramid (lsf_depth_pyramid)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "depth_unit_ratio", "sigma_space",
                                               "sigma_range", "depth_gate")] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "depth_dtype", "levels", "radius")]


class IcpPyramidParams(ctypes.Structure):
    """lsf_icp_pyramid_params: point-to-plane ICP over a live depth pyramid (lsf_icp_run_pyramid)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "max_distance", "cos_max_angle")] + \
               [("twist_p", ctypes.c_double * 6)] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "pyramid_levels", "levels", "angle_gate")] + \
               [("iterations", ctypes.c_int32 * ICP_MAX_LEVELS)]


ICP_PHOTOMETRIC_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 31 * 8


class IcpPhotometricParams(ctypes.Structure):
    """lsf_icp_photometric_params: joint geometric and photometric ICP on the strided path (lsf_icp_run_photometric)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "depth_unit_ratio", "max_distance",
                                               "photometric_weight", "max_intensity_difference")] + \
               [("twist_p", ctypes.c_double * 6)] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "depth_dtype", "levels")] + \
               [("iterations", ctypes.c_int32 * ICP_MAX_LEVELS), ("strides", ctypes.c_int32 * ICP_MAX_LEVELS)]


INTENSITY_SOURCE_COLOUR, INTENSITY_SOURCE_PREDICTION = 0, 1


class IntensityPyramidParams(ctypes.Structure):
    """lsf_intensity_pyramid_params: an intensity pyramid of a colour image or a ray-cast colour image
    (lsf_intensity_pyramid)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("height", "width", "levels", "source")]


ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 32 * 8


class IcpPyramidPhotometricParams(ctypes.Structure):
    """lsf_icp_pyramid_photometric_params: joint geometric and photometric ICP over a live depth pyramid and two
    intensity pyramids (lsf_icp_run_pyramid_photometric)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "max_distance", "cos_max_angle",
                                               "photometric_weight", "max_intensity_difference")] + \
               [("twist_p", ctypes.c_double * 6)] + \
               [(n, ctypes.c_int32) for n in ("height", "width", "pyramid_levels", "levels", "angle_gate",
                                              "reserved")] + \
               [("iterations", ctypes.c_int32 * ICP_MAX_LEVELS)]


ICP_LOSS_HUBER, ICP_LOSS_TUKEY = 1, 2
ICP_ROBUST_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 34 * 8
ICP_PYRAMID_ROBUST_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 35 * 8
_ROBUST_FIELDS = [("loss", ctypes.c_int32), ("scale", ctypes.c_double), ("intensity_scale", ctypes.c_double)]


class IcpRobustParams(ctypes.Structure):
    """lsf_icp_robust_params: lsf_icp_photometric_params' members, then the loss and its two scales (lsf_icp_run_robust)"""
    _fields_ = IcpPhotometricParams._fields_ + _ROBUST_FIELDS


class IcpPyramidRobustParams(ctypes.Structure):
    """lsf_icp_pyramid_robust_params: lsf_icp_pyramid_photometric_params' members, then the loss and its two scales
    (lsf_icp_run_pyramid_robust)"""
    _fields_ = IcpPyramidPhotometricParams._fields_ + _ROBUST_FIELDS


POINT_SDF_LOSS_NONE = 0
POINT_SDF_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 33 * 8


class PointSdfParams(ctypes.Structure):
    """lsf_point_sdf_params: point-to-SDF tracking of a live depth frame against the canonical TSDF (lsf_point_sdf_run)"""
    _fields_ = [(n, ctypes.c_double) for n in ("fx", "fy", "cx", "cy", "depth_unit_ratio", "max_distance", "voxel_size",
                                               "offset_x", "offset_y", "offset_z", "narrow_band_width_voxels",
                                               "scale")] + \
               [(n, ctypes.c_int32) for n in ("depth", "height", "width", "image_height", "image_width", "depth_dtype",
                                              "levels")] + \
               [("iterations", ctypes.c_int32 * ICP_MAX_LEVELS), ("strides", ctypes.c_int32 * ICP_MAX_LEVELS),
                ("loss", ctypes.c_int32)]


POINT_SDF_COLOUR_SCRATCH_BYTES = 2 * ICP_MAX_BLOCKS * 35 * 8
_POINT_SDF_COLOUR_FIELDS = [(n, ctypes.c_double) for n in ("photometric_weight", "max_intensity_difference",
                                                           "intensity_scale")]


class PointSdfPhotometricParams(ctypes.Structure):
    """lsf_point_sdf_photometric_params: lsf_point_sdf_params' members, then the colour term's
    (lsf_point_sdf_run_photometric)"""
    _fields_ = PointSdfParams._fields_ + _POINT_SDF_COLOUR_FIELDS


class PointSdfPyramidParams(ctypes.Structure):
    """lsf_point_sdf_pyramid_params: lsf_point_sdf_photometric_params' members, then the levels the pyramids hold
    (lsf_point_sdf_run_pyramid)"""
    _fields_ = PointSdfPhotometricParams._fields_ + [("pyramid_levels", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class EwaParams(ctypes.Structure):
    _fields_ = [("covariance_camera_space", ctypes.c_double * 9), ("squared_radius_threshold", ctypes.c_double),
                ("intrinsic_matrix", ctypes.c_float * 9), ("method", ctypes.c_int32)]


_P = ctypes.POINTER
_vp, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

# name -> (restype, argtypes); every symbol include/lsf_hip.h declares
PROTOTYPES = {
    "lsf_abi_version": (ctypes.c_int, []),
    "lsf_target_arch": (ctypes.c_char_p, []),
    "lsf_build_id": (ctypes.c_char_p, []),
    "lsf_abi_hash": (ctypes.c_char_p, []),
    "lsf_deinterleave": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lsf_interleave": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lsf_halo_copy": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _i32, _i32, _i32, _i32, _i32, _vp]),
    "lsf_warp_field": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _f32, _vp]),
    "lsf_warp_field_advanced": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Grid), _i32, _vp]),
    "lsf_pack_live_gradient": (ctypes.c_int, [_vp, _vp, _P(Grid), _vp]),
    "lsf_restrict_mean": (ctypes.c_int, [_vp, _vp, _P(Grid), _i32, _vp]),
    "lsf_prolong_repeat": (ctypes.c_int, [_vp, _vp, _P(Grid), _vp]),
    "lsf_upsample2x_linear": (ctypes.c_int, [_vp, _vp, _P(Grid), _i32, _vp]),
    "lsf_downsample2x_linear": (ctypes.c_int, [_vp, _vp, _P(Grid), _i32, _vp]),
    "lsf_convolve_axis": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _i32, _i32, _P(ctypes.c_double), _i32,
                                         _P(Gate), _vp]),
    "lsf_convolve_xy": (ctypes.c_int, [_vp, _vp, _P(Grid), _i32, _P(ctypes.c_double), _i32, _P(Gate), _vp]),
    "lsf_convolve_axis_update": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _P(Grid), _i32, _i32, _P(ctypes.c_double),
                                                _i32, _P(Gate), _vp]),
    "lsf_convolve_xyz": (ctypes.c_int, [_vp, _vp, _vp, _f32, _P(Grid), _i32, _P(ctypes.c_double), _i32, _P(Gate),
                                        _vp]),
    "lsf_hier_iteration": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Grid), _P(HierParams), _P(Gate), _vp, _vp]),
    "lsf_hier_update": (ctypes.c_int, [_vp, _vp, _P(Grid), _f32, _P(Gate), _vp, _vp]),
    "lsf_hier_level_run_2d": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(Grid), _P(HierParams), _P(ctypes.c_double),
                                            _i32, _vp, _i32, _i32, ctypes.c_float, _vp]),
    "lsf_slavcheva_gradient": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _P(SlavchevaParams), _P(Gate), _vp,
                                              _vp, _i64, _vp]),
    "lsf_convolve_axis_listed": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _i32, _i32, _P(ctypes.c_double), _i32,
                                                _P(Gate), _vp, _i64, _vp]),
    "lsf_state_prepare_scratch_elements": (ctypes.c_int64, [_P(Grid)]),
    "lsf_band_list_fill_prepared": (ctypes.c_int, [_P(Grid), _i32, _vp, _vp, _vp]),
    "lsf_state_prepare": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _vp, _vp, _vp]),
    "lsf_state_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _vp]),
    "lsf_state_pack_needed": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _vp, _i32, _i32, _vp]),
    "lsf_state_unpack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _vp]),
    "lsf_state_finalize_scratch_elements": (ctypes.c_int64, [_P(Grid)]),
    "lsf_state_finalize": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Grid), _f32, _vp, _vp, _vp]),
    "lsf_planar_finalize": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Grid), _f32, _vp, _vp, _vp]),
    "lsf_state_finalize_listed": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _P(ctypes.c_void_p), _P(_i64), _i32,
                                                 _i64, _i64, _f32, _vp, _vp, _vp, _vp, _i32, _f32, _vp]),
    "lsf_slavcheva_state_iteration": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _P(SlavchevaParams), _P(Gate), _vp,
                                                     _vp, _i64, _i32, _vp]),
    "lsf_cumulative_warp_compose": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _P(Gate), _vp, _i64, _vp]),
    "lsf_band_boxes_scratch_elements": (ctypes.c_int64, [_P(Grid)]),
    "lsf_band_boxes_count": (ctypes.c_int, [_P(Grid), ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsf_band_boxes_fill": (ctypes.c_int, [_P(Grid), ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsf_band_boxes_canonical": (ctypes.c_int, [_vp, _P(Grid), _vp, ctypes.c_int64, _vp, _vp]),
    "lsf_slavcheva_state_iteration_boxes": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _P(SlavchevaParams), _P(Gate), _vp, _vp,
                                                           _i64, _vp]),
    "lsf_state_run_begin": (ctypes.c_int, [_P(StateRun), _vp]),
    "lsf_state_run_finish_rows": (ctypes.c_int, [_P(StateRun), _P(SlavchevaParams), _vp, _vp, _vp, _vp, _vp, _i32, _P(RunLoop),
                                                 _vp, _f32, _vp, _vp, _vp, _vp, _P(StateRunResult), _vp, ctypes.c_int64,
                                                 _P(ctypes.c_int32), _vp]),
    "lsf_state_run_rows_elements": (ctypes.c_int64, [_P(Grid), _i32, _i32]),
    "lsf_state_run_finish": (ctypes.c_int, [_P(StateRun), _P(SlavchevaParams), _vp, _vp, _vp, _vp, _vp, _i32, _P(RunLoop), _vp,
                                            _f32, _vp, _vp, _vp, _vp, _P(StateRunResult), _vp]),
    "lsf_sobolev_run_finish": (ctypes.c_int, [_P(StateRun), _P(SlavchevaParams), _P(ctypes.c_double), _i32, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _i32, _P(RunLoop), _vp, _f32, _vp, _vp, _vp, _vp,
                                              _P(StateRunResult), _vp]),
    "lsf_slab_run_begin": (ctypes.c_int, [_P(SlabRun), _vp]),
    "lsf_slab_run_finish": (ctypes.c_int, [_P(SlabRun), _vp, _P(SlavchevaParams), _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                           _P(StateRunResult), _vp]),
    "lsf_band_scratch_elements": (ctypes.c_int64, [_P(Grid)]),
    "lsf_band_count": (ctypes.c_int, [_vp, _vp, _P(Grid), _i32, _vp, _vp, _vp]),
    "lsf_band_list_fill": (ctypes.c_int, [_vp, _vp, _P(Grid), _i32, _vp, _vp, _vp]),
    "lsf_records_decode": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "lsf_merge_sorted_runs": (ctypes.c_int, [_P(_vp), _P(_i64), _P(_vp), _P(_i64), _P(_vp), _i32, _vp]),
    "lsf_slab_unique_id": (ctypes.c_int, [ctypes.c_char_p, _vp]),
    "lsf_slab_comm_create": (ctypes.c_int, [ctypes.c_char_p, _vp, _i32, _i32, _P(_vp)]),
    "lsf_slab_comm_destroy": (ctypes.c_int, [_vp]),
    "lsf_slab_comm_info": (ctypes.c_int, [_vp, _P(_i32), _P(_i32)]),
    "lsf_slab_face_counts_begin": (ctypes.c_int, [_vp, _P(_i64)]),
    "lsf_slab_face_counts_end": (ctypes.c_int, [_vp, _P(_i64)]),
    "lsf_slab_state_iteration": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(SlabLayoutC), _P(SlabPart), _i32, _P(SlabPart),
                                                _i32, _P(SlavchevaParams), _P(Gate), _vp, _i32, _P(SlabFaces), _vp]),
    "lsf_slavcheva_filter_update_rewarp": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(Grid), _P(SlavchevaParams),
                                                          _i32, _P(ctypes.c_double), _i32, _P(Gate), _vp, _vp, _i64,
                                                          _vp]),
    "lsf_sobolev_state_gradient": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _P(SlavchevaParams), _P(Gate), _vp, _vp, _i64,
                                                  _vp]),
    "lsf_band_list_strip_major": (ctypes.c_int, [_vp, _i64, _P(Grid), _i32, _vp, _vp, _vp]),
    "lsf_sobolev_state_gradient_x": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _P(SlavchevaParams), _P(ctypes.c_double), _i32,
                                                    _P(Gate), _vp, _vp, _i64, _i32, _vp]),
    "lsf_zero_listed4": (ctypes.c_int, [_vp, _P(Grid), _vp, _i64, _i32, _vp]),
    "lsf_convolve_axis_listed4": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _i32, _P(ctypes.c_double), _i32, _P(Gate), _vp,
                                                 _i64, _vp]),
    "lsf_sobolev_state_update": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Grid), _P(SlavchevaParams), _i32,
                                                _P(ctypes.c_double), _i32, _P(Gate), _vp, _vp, _i64, _i32, _vp]),
    "lsf_sobolev_state_update_boxes": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Grid), _P(SlavchevaParams),
                                                      _P(ctypes.c_double), _i32, _P(Gate), _vp, _vp, _i64, _vp]),
    "lsf_slavcheva_update_rewarp": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Grid), _P(SlavchevaParams),
                                                   _P(Gate), _vp, _vp, _i64, _vp]),
    "lsf_term_gradient": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(Grid), _P(TermParams), _i32, _i32,
                                         _vp, _i64, _vp]),
    "lsf_warp_statistics": (ctypes.c_int, [_vp, _vp, _vp, _P(Grid), _f32, _vp, _vp]),
    "lsf_tsdf_difference_statistics": (ctypes.c_int, [_vp, _vp, _P(Grid), _vp, _vp]),
    "lsf_tsdf_generate_nearest": (ctypes.c_int, [_vp, _vp, _P(Grid), _P(TsdfParams), _vp]),
    "lsf_tsdf_generate_bilinear": (ctypes.c_int, [_vp, _vp, _P(Grid), _P(TsdfParams), _i32, _vp]),
    "lsf_tsdf_generate_ewa": (ctypes.c_int, [_vp, _vp, _P(Grid), _P(TsdfParams), _P(EwaParams), _vp]),
    "lsf_tsdf_generate_nearest_typed": (ctypes.c_int, [_vp, _i32, _vp, _P(Grid), _P(TsdfParams), _P(ctypes.c_double),
                                                       _P(ctypes.c_double), _vp]),
    "lsf_rigid_gradient": (ctypes.c_int, [_vp, _vp, _P(RigidParams), _vp]),
    "lsf_rigid_run": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(RigidParams), _vp]),
    "lsf_rigid3d_gradient": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(Rigid3dParams), _vp]),
    "lsf_rigid3d_run": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(Rigid3dParams), _vp]),
    "lsf_fusion_integrate_volume": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(FusionParams), _vp]),
    "lsf_fusion_integrate_depth": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _P(FusionParams), _vp]),
    "lsf_fusion_integrate_depth_weighted": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(FusionWeightedParams),
                                                           _vp]),
    "lsf_fusion_integrate_depth_colour": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                         _P(FusionColourParams), _vp]),
    "lsf_fusion_integrate_depth_warped": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                         _P(FusionWarpedParams), _vp]),
    "lsf_depth_confidence": (ctypes.c_int, [_vp, _vp, _vp, _P(DepthConfidenceParams), _vp]),
    "lsf_raycast": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(RaycastParams), _vp]),
    "lsf_raycast_colour": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(RaycastParams), _vp]),
    "lsf_mesh_count": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(MeshParams), _vp]),
    "lsf_mesh_emit": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _P(MeshParams), _vp]),
    "lsf_mesh_vertex_colours": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int32, _P(MeshParams), _vp]),
    "lsf_mesh_simplify_count": (ctypes.c_int, [_vp] * 11 + [_P(MeshSimplifyParams), _vp]),
    "lsf_mesh_simplify_emit": (ctypes.c_int, [_vp] * 11 + [_i64, _i64, _i64, _P(MeshSimplifyParams), _vp]),
    "lsf_mesh_components_label": (ctypes.c_int, [_vp] * 5 + [_P(MeshComponentsParams), _vp]),
    "lsf_mesh_components_table": (ctypes.c_int, [_vp] * 7 + [_i64, _P(MeshComponentsParams), _vp]),
    "lsf_mesh_components_select": (ctypes.c_int, [_vp] * 5 + [_i64, _P(MeshComponentsParams), _vp]),
    "lsf_mesh_components_emit": (ctypes.c_int, [_vp] * 11 + [_i64, _i64, _i64, _P(MeshComponentsParams), _vp]),
    "lsf_mesh_smooth_prepare": (ctypes.c_int, [_vp] * 9 + [_P(MeshSmoothParams), _vp]),
    "lsf_mesh_smooth_run": (ctypes.c_int, [_vp] * 7 + [_P(MeshSmoothParams), _vp]),
    "lsf_mesh_vertex_normals": (ctypes.c_int, [_vp] * 6 + [_P(MeshSmoothParams), _vp]),
    "lsf_esdf_compute": (ctypes.c_int, [_vp] * 8 + [_P(EsdfParams), _vp]),
    "lsf_volume_shift": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(VolumeShiftParams), _vp]),
    "lsf_volume_bricks_count": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(VolumeBricksParams), _vp]),
    "lsf_volume_bricks_gather": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                                _P(VolumeBricksParams), _vp]),
    "lsf_volume_bricks_scatter": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                                 _P(VolumeBricksParams), _vp]),
    "lsf_rgbd_ray_table": (ctypes.c_int, [_vp, _vp, _P(RgbdParams), _vp]),
    "lsf_rgbd_register_depth": (ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _P(RgbdParams), _vp]),
    "lsf_rgbd_rectify_colour": (ctypes.c_int, [_vp, _vp, _vp, _P(RgbdParams), _vp]),
    "lsf_reloc_encode": (ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _P(RelocParams), _vp]),
    "lsf_reloc_query": (ctypes.c_int, [_vp] * 9 + [_P(RelocParams), _vp]),
    "lsf_icp_run": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(IcpParams), _vp]),
    "lsf_depth_pyramid": (ctypes.c_int, [_vp, _vp, _vp, _P(DepthPyramidParams), _vp]),
    "lsf_icp_run_pyramid": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(IcpPyramidParams), _vp]),
    "lsf_icp_run_photometric": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _P(IcpPhotometricParams), _vp]),
    "lsf_intensity_pyramid": (ctypes.c_int, [_vp, _vp, _P(IntensityPyramidParams), _vp]),
    "lsf_icp_run_pyramid_photometric": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                       _P(IcpPyramidPhotometricParams), _vp]),
    "lsf_icp_run_robust": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(IcpRobustParams),
                                          _vp]),
    "lsf_icp_run_pyramid_robust": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _P(IcpPyramidRobustParams), _vp]),
    "lsf_point_sdf_run": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(PointSdfParams), _vp]),
    "lsf_point_sdf_run_photometric": (ctypes.c_int, [_vp] * 11 + [_P(PointSdfPhotometricParams), _vp]),
    "lsf_point_sdf_run_pyramid": (ctypes.c_int, [_vp] * 11 + [_P(PointSdfPyramidParams), _vp]),
}


class LsfHipError(RuntimeError):
    pass


def _load():
    # LSF_HIP_LIBRARY: another build of the SAME HIP library (A/B measurements of kernel variants, tools/ab_state_kernel.py)
    path = os.environ.get("LSF_HIP_LIBRARY") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            "liblsf_hip.so is missing (%s).  This package has no CPU fallback: build the HIP library first with\n"
            "    python -c 'import __graft_entry__ as g; g.build()'      (needs hipcc, cross-compiles gfx950)"
            % path)
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if argtypes is None:
            continue
        fn = getattr(lib, name)  # AttributeError here = the .so is stale against the header
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.lsf_abi_version() != ABI_VERSION:
        raise ImportError("liblsf_hip.so ABI version %d != binding version %d: rebuild" %
                          (lib.lsf_abi_version(), ABI_VERSION))
    built_against = lib.lsf_abi_hash().decode()
    if built_against != HEADER_ABI_HASH:
        raise ImportError("%s was compiled from an include/lsf_hip.h whose structures / prototypes hash to %s; this binding "
                          "was written against %s: rebuild the library (or update the binding to the header)"
                          % (path, built_against, HEADER_ABI_HASH))
    return lib


lib = _load()

def check(status, what):
    if status == 0:
        return
    if status in ERRORS:
        raise LsfHipError("%s: %s" % (what, ERRORS[status]))
    raise LsfHipError("%s: HIP error %d" % (what, status))
