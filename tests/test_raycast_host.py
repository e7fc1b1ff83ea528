"""CPU checks of ray-casting the canonical TSDF: the numpy restatement (tests/raycast_restatement.py) against the analytic
scene (tests/fusion_scene.py), the restated "raycast" tracking sequence against the scene's true twists, the ctypes
layout of lsf_raycast_params, the header's macros, the exports, the refusal of bad arguments and the no-CPU-path
error."""
import ctypes
import math
import os

import numpy as np
import pytest

import fusion_restatement as F
import fusion_scene as S
import raycast_restatement as RC
from conftest import ROOT

# the restated "raycast" sequence, 48^3, five frames, 60 rigid iterations, measured: the largest translation error of a
# frame 1.5, 3.6, 4.9 and 7.1 mm, the largest rotation error 3.0e-3, 7.1e-3, 9.6e-3 and 1.4e-2 rad (frames 1-4).  The
# bounds are twice the worst frame.  Tracking against the model itself misses by up to 0.21 m and 0.49 rad
# (tests/test_fusion_host.py::test_restated_sequence).
SEQUENCE_ATOL_T, SEQUENCE_ATOL_R = 0.015, 0.03


def _model(n, frames=1):
    off = S.offset(n)
    t, w = F.empty_model((n,) * 3)
    for k, depth in enumerate(S.frames(frames)):
        t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k))
    return t, w, off


def test_the_restated_prediction_matches_the_scene():
    """frame 0 fused at the identity and ray-cast at the identity: within 0.2 mm of the analytic depth on average; the
    pixels above 2 mm are silhouette pixels, where a ray grazes a sphere"""
    t, w, off = _model(48)
    depth, normals, hits = RC.raycast(t, w, S.K, np.zeros(6), off, normals=True)
    truth = S.render(np.zeros(6))
    hit = depth > 0
    assert hits == int(hit.sum()) == 44413
    err = np.abs(depth - truth)[hit]
    assert err.mean() < 2.0e-4, err.mean()  # a voxel is 4 mm
    assert int((err > 0.002).sum()) == 445
    # the back plane faces the camera: its normal is (0, 0, -1); every normal is a unit vector or zero.  8282 hits have
    # none: within a voxel of the box's sides a difference sample leaves the box, and at silhouettes it meets an
    # unobserved voxel
    assert depth[240, 235] == pytest.approx(S.PLANE_Z, abs=5e-4)
    assert np.allclose(normals[240, 235], [0, 0, -1], atol=1e-3)
    length = np.linalg.norm(normals[hit], axis=1)
    assert np.all((np.abs(length - 1) < 1e-6) | (length == 0)) and int((length == 0).sum()) == 8282
    assert not normals[~hit].any()


def test_the_restated_normals_face_the_camera():
    t, w, off = _model(48)
    depth, normals, _ = RC.raycast(t, w, S.K, np.zeros(6), off, normals=True)
    lit = np.linalg.norm(normals, axis=-1) > 0
    assert np.mean(normals[lit][:, 2] < 0) > 0.99  # the gradient of the TSDF points out of the surface, to the camera
    centre = S.SPHERES[0]
    v, u = 240, 320  # the ray through the principal point meets the first sphere head on
    assert depth[v, u] == pytest.approx(centre[0][2] - centre[1], abs=5e-4)
    assert np.allclose(normals[v, u], [0, 0, -1], atol=2e-2)


def test_rays_that_miss_and_the_fallback():
    t, w, off = _model(32)
    small = np.array([[70.0, 0, 32], [0, 70.0, 24], [0, 0, 1]], np.float32)  # a 64 x 48 camera of the same view
    depth, _, hits = RC.raycast(t, w, small, np.zeros(6), off, image_shape=(48, 64))
    fb16 = np.arange(48 * 64, dtype=np.uint16).reshape(48, 64)
    filled, _, hits2 = RC.raycast(t, w, small, np.zeros(6), off, image_shape=(48, 64), fallback=fb16, ratio=0.001)
    assert hits == hits2 and 0 < hits < 48 * 64
    hit = depth > 0
    assert np.array_equal(filled[hit], depth[hit])
    assert np.array_equal(filled[~hit], (fb16[~hit].astype(np.float64) * 0.001).astype(np.float32))
    empty = F.empty_model((16, 16, 16))
    d, n, h = RC.raycast(*empty, S.K, np.zeros(6), S.offset(16), image_shape=(20, 30), normals=True)
    assert h == 0 and not d.any() and not n.any()


def test_restated_raycast_sequence():
    """48^3, five frames, 60 rigid iterations: SequenceFusion3d(tracking_reference="raycast") restated.  Every frame
    stays within (SEQUENCE_ATOL_T, SEQUENCE_ATOL_R) of the true twist; the same sequence tracked against the model
    (tests/test_fusion_host.py::test_restated_sequence) is more than 10x outside those bounds."""
    n, count = 48, 5
    off = S.offset(n)
    tsdf, weight, twists, records, hits = RC.sequence(S.frames(count), S.K, 1.0, (n,) * 3, off, 60)
    assert hits == [None, 44413, 44201, 44086, 44107]
    assert [r["fused"] for r in records] == [32916, 32873, 32842, 32834, 32873]
    assert [r["first_seen"] for r in records] == [32916, 234, 144, 102, 134]
    err = np.abs(np.array(twists) - np.array([S.true_twist(k) for k in range(count)]))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err
    np.testing.assert_allclose(err[1:, :3].max(axis=1), [1.48e-3, 3.61e-3, 4.87e-3, 7.10e-3], rtol=0.02)
    np.testing.assert_allclose(err[1:, 3:].max(axis=1), [2.98e-3, 7.11e-3, 9.58e-3, 1.394e-2], rtol=0.02)


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p = lib.RaycastParams
    assert [f[0] for f in p._fields_] == ["fx", "fy", "cx", "cy", "depth_unit_ratio", "voxel_size", "offset_x",
                                          "offset_y", "offset_z", "t_x", "t_y", "t_z", "r_x", "r_y", "r_z", "depth",
                                          "height", "width", "image_height", "image_width", "fallback_dtype"]
    assert ctypes.sizeof(p) == 15 * 8 + 6 * 4 and p.depth.offset == 120 and p.fallback_dtype.offset == 140
    assert lib.RAYCAST_STEPS_PER_VOXEL == RC.STEPS_PER_VOXEL == 2 and lib.RAYCAST_TILE == 16
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for macro, value in (("LSF_RAYCAST_STEPS_PER_VOXEL", "2"), ("LSF_RAYCAST_TILE", "16")):
        assert "#define %s %s" % (macro, value) in header
    assert "lsf_raycast" in lib.PROTOTYPES and lib.lib.lsf_raycast is not None


def _good_params():
    import levelsetfusion_python_amd._lib as lib
    p = lib.RaycastParams()
    p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.voxel_size = 700.0, 700.0, 320.0, 240.0, 0.001, 0.004
    p.offset_z = 100.0
    p.depth, p.height, p.width, p.image_height, p.image_width = 8, 8, 8, 48, 64
    return p


def test_the_c_abi_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    f = lib.lib.lsf_raycast
    p = _good_params()
    # never dereferenced: every call below is refused on the host.  The fake buffers are far apart (1 MiB), so only
    # the cases built to alias do.
    t, w, fb, d, n, h = (ctypes.c_void_p((1 << 20) * k) for k in (1, 2, 3, 4, 5, 6))
    for field, value in (("depth", 1), ("width", 0), ("height", -3), ("image_height", 0), ("image_width", -1),
                         ("voxel_size", 0.0), ("voxel_size", -0.004), ("voxel_size", math.nan), ("fx", 0.0),
                         ("fy", math.inf), ("cx", math.nan), ("offset_y", math.inf), ("r_z", math.nan),
                         ("t_x", -math.inf), ("image_height", 1 << 16)):
        q = lib.RaycastParams.from_buffer_copy(p)
        setattr(q, field, value)
        if field == "image_height" and value == 1 << 16:
            q.image_width = 1 << 16  # 2^32 pixels
        assert f(t, w, None, d, None, None, ctypes.byref(q), None) == -1, (field, value)
    for field, value in (("fallback_dtype", 3), ("fallback_dtype", -1), ("depth_unit_ratio", math.nan)):
        q = lib.RaycastParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert f(t, w, fb, d, None, None, ctypes.byref(q), None) == -1, (field, value)
    P = ctypes.byref(p)
    assert f(None, w, None, d, None, None, P, None) == -1
    assert f(t, None, None, d, None, None, P, None) == -1
    assert f(t, w, None, None, None, None, P, None) == -1
    assert f(t, t, None, d, None, None, P, None) == -1           # tsdf is weight
    assert f(t, w, None, t, None, None, P, None) == -1           # depth_out aliases tsdf
    assert f(t, w, fb, fb, None, None, P, None) == -1            # depth_out aliases the fallback
    assert f(t, w, None, d, d, None, P, None) == -1              # normals_out aliases depth_out
    assert f(t, w, None, d, None, w, P, None) == -1              # hit_count aliases weight
    assert f(t, w, None, d, None, h, None, None) == -1           # no params
    near = ctypes.c_void_p((1 << 20) * 4 + 4 * 48 * 64 - 4)      # the last float of depth_out
    assert f(t, w, None, d, near, None, P, None) == -1
    assert f(t, w, None, d, None, near, P, None) == -1


def test_host_argument_checks():
    from levelsetfusion_python_amd import device_raycast
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    p = device_raycast.params((8, 9, 10), cam, np.arange(6) * 0.01, [1, 2, 3.5], 0.004, (48, 64))
    assert (p.depth, p.height, p.width, p.image_height, p.image_width) == (8, 9, 10, 48, 64)
    assert (p.fx, p.fy, p.cx, p.cy) == (700.0, 700.0, 320.0, 240.0) and p.offset_z == 3.5 and p.r_z == 0.05
    for bad in (dict(shape=(8, 8)), dict(shape=(1, 8, 8)), dict(image_shape=(0, 4)), dict(image_shape=(4,)),
                dict(voxel_size=0.0), dict(voxel_size=math.nan), dict(twist=np.zeros(3)),
                dict(twist=[0, 0, 0, 0, 0, math.nan]), dict(array_offset=[0, 0]), dict(array_offset=[0, math.inf, 0])):
        kw = dict(shape=(8, 8, 8), camera=cam, twist=np.zeros(6), array_offset=[0, 0, 0], voxel_size=0.004,
                  image_shape=(4, 4))
        kw.update(bad)
        with pytest.raises(ValueError):
            device_raycast.params(**kw)
    flat = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=np.diag([0.0, 1.0, 1.0])))
    with pytest.raises(ValueError, match="intrinsics"):
        device_raycast.params((8, 8, 8), flat, np.zeros(6), [0, 0, 0], 0.004, (4, 4))


def test_package_exports_raycast():
    from levelsetfusion_python_amd import device_raycast, fusion
    assert callable(fusion.CanonicalVolume.raycast) and callable(device_raycast.raycast)
    assert fusion.TRACKING_REFERENCES == ("model", "raycast")
    assert "raycast" in fusion.__doc__ and "prediction" in fusion.__doc__


def test_no_cpu_path():
    import torch
    from levelsetfusion_python_amd import device_raycast, fusion
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    z = torch.zeros((4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        device_raycast.raycast(z, z.clone(), cam, np.zeros(6), [0, 0, 0])
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        fusion.SequenceFusion3d(cam, 8, [0, 0, 100], tracking_reference="raycast")
