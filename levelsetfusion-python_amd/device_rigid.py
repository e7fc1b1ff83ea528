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


TWIST_NAMES = {3: "t_x, t_z, theta", 6: "t_x, t_y, t_z, r_x, r_y, r_z"}


def _device_f32(x, name, rank):
    """x as a contiguous float32 device tensor of `rank` extents >= 2: a 2-D field or a 3-D volume"""
    if isinstance(x, torch.Tensor):
        t = (x if x.is_cuda else x.to("cuda")).to(torch.float32).contiguous()
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "fiub":
            raise ValueError("%s must be numeric, got %s" % (name, a.dtype))
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")
    if t.dim() != rank or min(t.shape) < 2:
        raise ValueError("%s must be a %d-D %s of at least %s, got shape %s" % (
            name, rank, "field" if rank == 2 else "volume", " x ".join(["2"] * rank), tuple(t.shape)))
    return t


def twist_n(twist, n):
    """the twist as a flat float64 n-vector: n = 3 (2-D tracker) or 6 (6-DoF)"""
    t = np.asarray(twist, dtype=np.float64).reshape(-1)
    if t.size != n:
        raise ValueError("twist must have %d entries (%s), got %d" % (n, TWIST_NAMES[n], t.size))
    return t


def twist3(twist):
    return twist_n(twist, 3)


def twist6(twist):
    return twist_n(twist, 6)


def enqueue_run(entry, name, inputs, p, twist, n, head, record, scratch_bytes, iterations, outputs=()):
    """a whole tracker run enqueued by `entry` (lsf_rigid_run / lsf_rigid3d_run / lsf_icp_run / lsf_icp_run_pyramid):
    iterations + 1 launches into one buffer [twist (n)][pad to head][records (iterations x record)], and one copy back.
    inputs: the device tensors the entry point reads, in its order (None after the first for an optional one); outputs: what it takes after the scratch buffer
    (device tensors, or None for a NULL).  Returns (final twist float64 (n,), records float64 (iterations, record))."""
    device = inputs[0].device
    out = torch.zeros(head + iterations * record, dtype=torch.float64, device=device)
    if twist is not None:
        out[:n] = torch.from_numpy(twist_n(twist, n).copy())
    scratch = torch.empty(scratch_bytes // 8, dtype=torch.float64, device=device)
    base = out.data_ptr()
    ptr = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in inputs]
    ptr += [ctypes.c_void_p(base), ctypes.c_void_p(base + head * 8), ctypes.c_void_p(scratch.data_ptr())]
    ptr += [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in outputs]
    check(entry(*ptr, ctypes.byref(p), stream_ptr()), name)
    host = out.cpu().numpy()
    return host[:n].copy(), host[head:].reshape(iterations, record).copy()


def gradient_wrt_twist(live_field, twist, array_offset, voxel_size=0.004):
    """(H, W, 3) float32 device tensor: calculate_gradient_wrt_twist of live_field (H, W) in one launch"""
    require_gpu()
    live = _device_f32(live_field, "live_field", 2)
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
    canonical = _device_f32(canonical, "canonical_field", 2)
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
    return enqueue_run(lib.lsf_rigid_run, "lsf_rigid_run", (canonical, live_depth), p, twist, 3, 3, RECORD,
                       _lib.RIGID_SCRATCH_BYTES, iterations)


# ---- the 6-DoF 3-D tracker (lsf_rigid3d_gradient, lsf_rigid3d_run) ----------------------------------------------------

RECORD3D = _lib.RIGID3D_RECORD_DOUBLES


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
    live = _device_f32(live, "live_field", 3)
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
                         generator_voxel_size=0.004, narrow_band_width_voxels=20., default_value=1, gradient=True):
    """(live (Z, Y, X), gradient (Z, Y, X, 6)) float32 device tensors: the live volume an iteration of rigid_run_3d
    generates under twist, and its twist gradient -- one launch of the run's own generation and gradient code.
    gradient=False: the live volume alone, and None"""
    require_gpu()
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p = _params3d(shape, array_offset, voxel_size)
    p.tsdf = _tsdf3d(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, default_value)
    p.twist[:] = list(twist6(twist))
    p.depth_dtype = int(depth_code)
    s = (p.depth, p.height, p.width)
    live = torch.empty(s, dtype=torch.float32, device="cuda")
    grad = torch.empty(s + (6,), dtype=torch.float32, device="cuda") if gradient else None
    check(lib.lsf_rigid3d_gradient(None, ctypes.c_void_p(live_depth.data_ptr()), ctypes.c_void_p(live.data_ptr()),
                                   ctypes.c_void_p(grad.data_ptr()) if gradient else None, ctypes.byref(p),
                                   stream_ptr()), "lsf_rigid3d_gradient")
    return live, grad


def live_volume_3d(live_depth, depth_code, camera, shape, array_offset, twist, voxel_size=0.004,
                   narrow_band_width_voxels=20., default_value=1):
    """(Z, Y, X) float32 device tensor: the live volume of live_and_gradient_3d alone (one launch, no gradient),
    generated at voxel_size"""
    return live_and_gradient_3d(live_depth, depth_code, camera, shape, array_offset, twist, voxel_size, voxel_size,
                                narrow_band_width_voxels, default_value, gradient=False)[0]


def rigid_run_3d(canonical, live_depth, depth_code, camera, array_offset, iterations, rate, eta, voxel_size,
                 generator_voxel_size, narrow_band_width_voxels, default_value=1, twist=None):
    """the whole 6-DoF optimize() enqueued: iterations + 1 launches and one copy back.  canonical: float32 volume
    (Z, Y, X), any extents >= 2; live_depth: device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*);
    twist: the starting 6-vector (zero by default).  Returns (final twist float64 (6,), records float64
    (iterations, RIGID3D_RECORD_DOUBLES))."""
    require_gpu()
    canonical = _device_f32(canonical, "canonical_field", 3)
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
    return enqueue_run(lib.lsf_rigid3d_run, "lsf_rigid3d_run", (canonical, live_depth), p, twist, 6, 8, RECORD3D,
                       _lib.RIGID3D_SCRATCH_BYTES, iterations)
