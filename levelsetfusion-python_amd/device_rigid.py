"""Torch-facing wrapper of the SDF-2-SDF rigid tracker's entry points (include/lsf_hip.h: lsf_rigid_gradient,
lsf_rigid_run, lsf_rigid3d_gradient, lsf_rigid3d_run).  The public drop-ins are rigid_opt/sdf_gradient_field.py,
rigid_opt/sdf_2_sdf_optimizer2d.py and rigid_opt/sdf_2_sdf_optimizer3d.py."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import RigidParams, check, lib
from .device_core import require_gpu, stream_ptr
from .tsdf.generation import offsets_of, tsdf_params

RECORD = _lib.RIGID_RECORD_DOUBLES


def _field(x, name):
    if isinstance(x, torch.Tensor):
        t = (x if x.is_cuda else x.to("cuda")).to(torch.float32).contiguous()
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "fiub":
            raise ValueError("%s must be numeric, got %s" % (name, a.dtype))
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")
    if t.dim() != 2 or t.shape[0] < 2 or t.shape[1] < 2:
        raise ValueError("%s must be a 2-D field of at least 2 x 2, got shape %s" % (name, tuple(t.shape)))
    return t


def twist3(twist):
    t = np.asarray(twist, dtype=np.float64).reshape(-1)
    if t.size != 3:
        raise ValueError("twist must have 3 entries (t_x, t_z, theta), got %d" % t.size)
    return t


def gradient_wrt_twist(live_field, twist, array_offset, voxel_size=0.004):
    """(H, W, 3) float32 device tensor: calculate_gradient_wrt_twist of live_field (H, W) in one launch"""
    require_gpu()
    live = _field(live_field, "live_field")
    p = RigidParams()
    p.array_offset[:] = list(offsets_of(array_offset))
    p.voxel_size = float(voxel_size)
    if not p.voxel_size > 0.0:
        raise ValueError("voxel_size must be positive")
    p.twist[:] = list(twist3(twist))
    p.height, p.width = int(live.shape[0]), int(live.shape[1])
    out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    check(lib.lsf_rigid_gradient(ctypes.c_void_p(live.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.byref(p),
                                 stream_ptr()), "lsf_rigid_gradient")
    return out


def rigid_run(canonical, live_depth, depth_code, camera, image_y_coordinate, array_offset, iterations, rate, eta,
              voxel_size, generator_voxel_size, narrow_band_width_voxels, default_value=1, twist=None):
    """the whole optimize() enqueued: iterations + 1 launches and one copy back.  canonical: float32 device field
    (H, W); live_depth: device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*).  Returns (final twist
    float64 (3,), records float64 (iterations, RIGID_RECORD_DOUBLES))."""
    require_gpu()
    canonical = _field(canonical, "canonical_field")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iteration must be >= 0")
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p = RigidParams()
    p.tsdf = tsdf_params(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, image_y_coordinate,
                         default_value)
    p.array_offset[:] = list(offsets_of(array_offset))
    p.voxel_size = float(voxel_size)
    p.rate = float(rate)
    p.eta = float(np.float32(eta))
    p.depth_dtype = int(depth_code)
    p.height, p.width = int(canonical.shape[0]), int(canonical.shape[1])
    p.iterations = iterations
    # one buffer: [twist (3)][records (iterations x RECORD)] -- one copy back
    out = torch.zeros(3 + iterations * RECORD, dtype=torch.float64, device="cuda")
    if twist is not None:
        out[:3] = torch.from_numpy(twist3(twist))
    scratch = torch.empty(_lib.RIGID_SCRATCH_BYTES // 8, dtype=torch.float64, device="cuda")
    base = out.data_ptr()
    check(lib.lsf_rigid_run(ctypes.c_void_p(canonical.data_ptr()), ctypes.c_void_p(live_depth.data_ptr()),
                            ctypes.c_void_p(base), ctypes.c_void_p(base + 3 * 8), ctypes.c_void_p(scratch.data_ptr()),
                            ctypes.byref(p), stream_ptr()), "lsf_rigid_run")
    host = out.cpu().numpy()
    return host[:3].copy(), host[3:].reshape(iterations, RECORD).copy()


# ---- the 6-DoF 3-D tracker (lsf_rigid3d_gradient, lsf_rigid3d_run) ----------------------------------------------------

RECORD3D = _lib.RIGID3D_RECORD_DOUBLES


def _volume(x, name):
    if isinstance(x, torch.Tensor):
        t = (x if x.is_cuda else x.to("cuda")).to(torch.float32).contiguous()
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "fiub":
            raise ValueError("%s must be numeric, got %s" % (name, a.dtype))
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")
    if t.dim() != 3 or min(t.shape) < 2:
        raise ValueError("%s must be a 3-D volume of at least 2 x 2 x 2, got shape %s" % (name, tuple(t.shape)))
    return t


def twist6(twist):
    t = np.asarray(twist, dtype=np.float64).reshape(-1)
    if t.size != 6:
        raise ValueError("twist must have 6 entries (t_x, t_y, t_z, r_x, r_y, r_z), got %d" % t.size)
    return t


def volume_shape(shape):
    """(Z, Y, X) ints >= 2, from an int (a cube) or a 3-sequence"""
    s = (int(shape),) * 3 if np.ndim(shape) == 0 else tuple(int(v) for v in shape)
    if len(s) != 3 or min(s) < 2:
        raise ValueError("a 3-D volume needs three extents >= 2, got %s" % (s,))
    return s


def _params3d(shape, array_offset, voxel_size):
    p = _lib.Rigid3dParams()
    p.array_offset[:] = list(offsets_of(array_offset))
    p.voxel_size = float(voxel_size)
    if not p.voxel_size > 0.0:
        raise ValueError("voxel_size must be positive")
    p.depth, p.height, p.width = volume_shape(shape)
    return p


def gradient_wrt_twist_3d(live, twist, array_offset, voxel_size=0.004):
    """(Z, Y, X, 6) float32 device tensor: the 6-DoF twist gradient of the live volume (Z, Y, X) in one launch"""
    require_gpu()
    live = _volume(live, "live_field")
    p = _params3d(live.shape, array_offset, voxel_size)
    p.twist[:] = list(twist6(twist))
    out = torch.empty(tuple(live.shape) + (6,), dtype=torch.float32, device="cuda")
    check(lib.lsf_rigid3d_gradient(ctypes.c_void_p(live.data_ptr()), None, None, ctypes.c_void_p(out.data_ptr()),
                                   ctypes.byref(p), stream_ptr()), "lsf_rigid3d_gradient")
    return out


def _tsdf3d(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, default_value):
    if not narrow_band_width_voxels > 0:
        raise ValueError("narrow_band_width_voxels must be positive")
    return tsdf_params(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, None, default_value)


def live_and_gradient_3d(live_depth, depth_code, camera, shape, array_offset, twist, voxel_size=0.004,
                         generator_voxel_size=0.004, narrow_band_width_voxels=20., default_value=1):
    """(live (Z, Y, X), gradient (Z, Y, X, 6)) float32 device tensors: the live volume an iteration of rigid_run_3d
    generates under twist, and its twist gradient -- one launch of the run's own generation and gradient code"""
    require_gpu()
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p = _params3d(shape, array_offset, voxel_size)
    p.tsdf = _tsdf3d(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, default_value)
    p.twist[:] = list(twist6(twist))
    p.depth_dtype = int(depth_code)
    s = (p.depth, p.height, p.width)
    live = torch.empty(s, dtype=torch.float32, device="cuda")
    grad = torch.empty(s + (6,), dtype=torch.float32, device="cuda")
    check(lib.lsf_rigid3d_gradient(None, ctypes.c_void_p(live_depth.data_ptr()), ctypes.c_void_p(live.data_ptr()),
                                   ctypes.c_void_p(grad.data_ptr()), ctypes.byref(p), stream_ptr()),
          "lsf_rigid3d_gradient")
    return live, grad


def live_volume_3d(live_depth, depth_code, camera, shape, array_offset, twist, voxel_size=0.004,
                   narrow_band_width_voxels=20., default_value=1):
    """(Z, Y, X) float32 device tensor: the live volume of live_and_gradient_3d alone (one launch, no gradient)"""
    require_gpu()
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p = _params3d(shape, array_offset, voxel_size)
    p.tsdf = _tsdf3d(P, camera, live_depth, voxel_size, narrow_band_width_voxels, default_value)
    p.twist[:] = list(twist6(twist))
    p.depth_dtype = int(depth_code)
    live = torch.empty((p.depth, p.height, p.width), dtype=torch.float32, device="cuda")
    check(lib.lsf_rigid3d_gradient(None, ctypes.c_void_p(live_depth.data_ptr()), ctypes.c_void_p(live.data_ptr()),
                                   None, ctypes.byref(p), stream_ptr()), "lsf_rigid3d_gradient")
    return live


def rigid_run_3d(canonical, live_depth, depth_code, camera, array_offset, iterations, rate, eta, voxel_size,
                 generator_voxel_size, narrow_band_width_voxels, default_value=1, twist=None):
    """the whole 6-DoF optimize() enqueued: iterations + 1 launches and one copy back.  canonical: float32 volume
    (Z, Y, X), any extents >= 2; live_depth: device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*);
    twist: the starting 6-vector (zero by default).  Returns (final twist float64 (6,), records float64
    (iterations, RIGID3D_RECORD_DOUBLES))."""
    require_gpu()
    canonical = _volume(canonical, "canonical_field")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iteration must be >= 0")
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p = _params3d(canonical.shape, array_offset, voxel_size)
    p.tsdf = _tsdf3d(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, default_value)
    p.rate = float(rate)
    p.eta = float(np.float32(eta))
    p.depth_dtype = int(depth_code)
    p.iterations = iterations
    # one buffer: [twist (6)][pad (2)][records (iterations x RECORD3D)] -- one copy back
    out = torch.zeros(8 + iterations * RECORD3D, dtype=torch.float64, device="cuda")
    if twist is not None:
        out[:6] = torch.from_numpy(twist6(twist))
    scratch = torch.empty(_lib.RIGID3D_SCRATCH_BYTES // 8, dtype=torch.float64, device="cuda")
    base = out.data_ptr()
    check(lib.lsf_rigid3d_run(ctypes.c_void_p(canonical.data_ptr()), ctypes.c_void_p(live_depth.data_ptr()),
                              ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * 8),
                              ctypes.c_void_p(scratch.data_ptr()), ctypes.byref(p), stream_ptr()), "lsf_rigid3d_run")
    host = out.cpu().numpy()
    return host[:6].copy(), host[8:].reshape(iterations, RECORD3D).copy()
