"""GPU check that every configuration of the two frame trackers reaches its own C entry point and computes what the
direct device call computes.  rigid_opt.ProjectiveIcp3d and rigid_opt.PointToSdf3d choose the entry point from their
settings ({strided, pyramid} x {no colour, colour} x {no loss, Tukey}); ENTRY_POINTS writes the choice out.  In each
configuration `track` must call exactly that symbol of the library, once, and its twist, records and residual image
must equal those of the direct device_icp / device_point_sdf call on the same inputs bit for bit.

The scene is tests/colour_scene.py's three spheres and plane seen by a 32 x 24 camera (fusion_scene's, scaled by 20, so
the 16 x 16 tiles are ragged) that stands 0.25 m nearer than fusion_scene's, three pyramid levels down to 8 x 6, and a
32^3 model of 8 mm voxels holding frame 0, fused by the restatement; frame 1 is tracked from frame 0's twist with
iterations (1, 1, 2).  Every record of the direct call has pairs (count > 0); test_scene_has_pairs_on_the_cpu asserts
it of the restated runs without a GPU.  From fusion_scene's own distance the largest sphere is six pixels wide and the
8 x 6 level sees the plane alone: its solve is singular, or with weights nearly so, and a Tukey run then leaves the
scene after its first step (count 0 from the second record on)."""
import functools

import numpy as np
import pytest

import colour_restatement as C
import colour_scene as CS
import fusion_restatement as F
import fusion_scene as S

IMAGE = (24, 32)
N, VOXEL = 32, 0.008
# fusion_scene.K for an image 20 times smaller: pixel centres map as u' = (u + 0.5) / 20 - 0.5
K = np.array([[35.0, 0, 15.525], [0, 35.0, 11.525], [0, 0, 1]], np.float32)
OFFSET = S.offset(64) / 2.0  # fusion_scene's 64^3 placement in voxels of twice the size
ITERATIONS, STRIDES, LEVELS = (1, 1, 2), (4, 2, 1), 3
MAX_DISTANCE = 0.05  # metres: a pixel of the coarsest level is 34 mm wide at the spheres
LAMBDA = 0.1
TUKEY = ("tukey", 0.03, 0.5)
NEARER = np.array([0.0, 0.0, -0.25, 0.0, 0.0, 0.0])  # the camera: the spheres at 0.3 m, twelve pixels wide
TWIST_P, TWIST_LIVE = NEARER + S.true_twist(0), NEARER + S.true_twist(1)

# (tracker, pyramid, colour, loss) -> the symbol `track` calls: the dispatch of the two trackers, written out.  The
# robust ICP entry points take the colour term as an option; point-to-SDF has the loss in every struct and no entry
# point of its own for it, and its pyramid entry point takes the colour term as an option
ENTRY_POINTS = {
    ("icp", False, False, False): "lsf_icp_run",
    ("icp", False, True, False): "lsf_icp_run_photometric",
    ("icp", False, False, True): "lsf_icp_run_robust",
    ("icp", False, True, True): "lsf_icp_run_robust",
    ("icp", True, False, False): "lsf_icp_run_pyramid",
    ("icp", True, True, False): "lsf_icp_run_pyramid_photometric",
    ("icp", True, False, True): "lsf_icp_run_pyramid_robust",
    ("icp", True, True, True): "lsf_icp_run_pyramid_robust",
    ("sdf", False, False, False): "lsf_point_sdf_run",
    ("sdf", False, False, True): "lsf_point_sdf_run",
    ("sdf", False, True, False): "lsf_point_sdf_run_photometric",
    ("sdf", False, True, True): "lsf_point_sdf_run_photometric",
    ("sdf", True, False, False): "lsf_point_sdf_run_pyramid",
    ("sdf", True, False, True): "lsf_point_sdf_run_pyramid",
    ("sdf", True, True, False): "lsf_point_sdf_run_pyramid",
    ("sdf", True, True, True): "lsf_point_sdf_run_pyramid",
}
SYMBOLS = sorted(set(ENTRY_POINTS.values()))


@functools.lru_cache(maxsize=None)
def scene():
    """(tsdf, weight, colour) of frame 0 fused into the empty model, and frame 1's (depth, colour image); read-only"""
    depth0, image0, _ = CS.render(TWIST_P, IMAGE[1], IMAGE[0], K)
    depth1, image1, _ = CS.render(TWIST_LIVE, IMAGE[1], IMAGE[0], K)
    t, w = F.empty_model((N,) * 3)
    c = np.zeros((N,) * 3 + (4,), np.float32)
    t, w, c, _ = C.fuse_depth_colour(t, w, c, depth0, image0, K, 1.0, OFFSET, TWIST_P, voxel_size=VOXEL)
    out = (t, w, c, depth1, image1)
    for a in out:
        a.setflags(write=False)
    return out


def test_scene_has_pairs_on_the_cpu():
    """every record of the restated strided runs -- ICP against the model's restated ray-cast and point-to-SDF against
    the model, least squares and Tukey -- has pairs and a solve that is not skipped.  A pyramid level of the device
    runs has the extents of the stride's grid"""
    import icp_restatement as I
    import point_sdf_restatement as P
    import raycast_restatement as RC
    import robust_icp_restatement as RR
    t, w, _, depth, _ = scene()
    pd, pn, hits = RC.raycast(t, w, K, TWIST_P, OFFSET, VOXEL, IMAGE, normals=True)
    assert hits > 300
    loss = RR.Loss(*TUKEY)
    runs = [I.icp(depth, pd, pn, K, 1.0, TWIST_P, None, ITERATIONS, STRIDES, MAX_DISTANCE)[0],
            RR.icp(loss, depth, pd, pn, K, 1.0, TWIST_P, None, ITERATIONS, STRIDES, MAX_DISTANCE)[0]]
    runs += [P.track(t, w, depth, K, 1.0, TWIST_P, OFFSET, ITERATIONS, STRIDES, MAX_DISTANCE, voxel_size=VOXEL,
                     loss=which)[0] for which in (None, loss)]
    for records in runs:
        assert len(records) == sum(ITERATIONS)
        assert min(r["count"] for r in records) >= 15 and not any(r["skipped"] for r in records)


@pytest.fixture(scope="module")
def device():
    """the scene on the device, the model's prediction at TWIST_P, and the frame's two pyramids; nothing modifies them"""
    import torch

    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_raycast
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera, device_depth
    t, w, c, depth, image = (torch.from_numpy(np.array(a)).cuda() for a in scene())
    camera = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K), depth_unit_ratio=1.0)
    depth, code = device_depth(depth)
    pd, pn, _, pc = device_raycast.raycast(t, w, camera, TWIST_P, OFFSET, VOXEL, IMAGE, normals=True, colour=c)
    pyramid = lsf.rigid_opt.DepthPyramid(levels=LEVELS)
    intensity = lsf.rigid_opt.IntensityPyramid(LEVELS)
    return dict(lsf=lsf, camera=camera, tsdf=t, weight=w, colour=c, depth=depth, code=code, image=image, pd=pd, pn=pn,
                pc=pc, pyramid=pyramid, intensity=intensity, levels=pyramid.build_device(depth, code, camera),
                live_intensity=intensity.build_device(image), pred_intensity=intensity.build_prediction(pc))


def _direct(d, tracker, pyramid, colour, robust):
    """the direct device call of a configuration: (twist, records, residual image)"""
    from levelsetfusion_python_amd import device_icp as DI
    from levelsetfusion_python_amd import device_point_sdf as DS
    lam = LAMBDA if colour else None
    if tracker == "sdf":
        model = (d["tsdf"], d["weight"])
        common = dict(voxel_size=VOXEL, iterations=ITERATIONS, max_distance=MAX_DISTANCE, robust=robust,
                      colour=d["colour"] if colour else None, photometric_weight=lam, residuals=True)
        if pyramid:
            out = DS.point_sdf_run_pyramid(*model, d["levels"].buffers[0], LEVELS, IMAGE, d["camera"], OFFSET, TWIST_P,
                                           pyramid_intensity=d["live_intensity"].buffer if colour else None, **common)
        elif colour:
            out = DS.point_sdf_run_photometric(*model, d["depth"], d["code"], d["camera"], OFFSET, TWIST_P,
                                               strides=STRIDES, live_colour=d["image"], **common)
        else:
            del common["colour"], common["photometric_weight"]
            out = DS.point_sdf_run(*model, d["depth"], d["code"], d["camera"], OFFSET, TWIST_P, strides=STRIDES,
                                   **common)
        return out[:3]
    common = dict(twist=TWIST_P, iterations=ITERATIONS, max_distance=MAX_DISTANCE, residuals=True)
    pred = (d["pd"], d["pn"])
    if pyramid:
        live, term = d["levels"].buffers, (d["live_intensity"].buffer, d["pred_intensity"].buffer)
        if robust is not None:
            joint = dict(pyramid_intensity=term[0], pred_intensity=term[1], photometric_weight=lam) if colour else {}
            out = DI.icp_run_pyramid_robust(*live, LEVELS, *pred, d["camera"], TWIST_P, robust, **common, **joint)
        elif colour:
            out = DI.icp_run_pyramid_photometric(*live, term[0], LEVELS, *pred, term[1], d["camera"], TWIST_P, lam,
                                                 **common)
        else:
            out = DI.icp_run_pyramid(*live, LEVELS, *pred, d["camera"], TWIST_P, **common)
        return out[:3]
    common["strides"] = STRIDES
    if robust is not None:
        joint = dict(live_colour=d["image"], pred_colour=d["pc"], photometric_weight=lam) if colour else {}
        out = DI.icp_run_robust(d["depth"], d["code"], *pred, d["camera"], TWIST_P, robust, **common, **joint)
    elif colour:
        out = DI.icp_run_photometric(d["depth"], d["code"], d["image"], *pred, d["pc"], d["camera"], TWIST_P, lam,
                                     **common)
    else:
        out = DI.icp_run(d["depth"], d["code"], *pred, d["camera"], TWIST_P, **common)
    return out[:3]


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy()).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("tracker,pyramid,colour,loss", sorted(ENTRY_POINTS))
def test_track_reaches_its_entry_point_bit_for_bit(device, monkeypatch, tracker, pyramid, colour, loss):
    from levelsetfusion_python_amd import _lib, device_icp
    d, R = device, device["lsf"].rigid_opt
    robust = R.RobustLoss(*TUKEY) if loss else None
    settings = dict(iterations=ITERATIONS, max_distance=MAX_DISTANCE, robust=robust,
                    pyramid=d["pyramid"] if pyramid else None, photometric_weight=LAMBDA if colour else None,
                    intensity_pyramid=d["intensity"] if pyramid and colour else None)
    if not pyramid:
        settings["strides"] = STRIDES
    want_twist, want_records, want_res = _direct(d, tracker, pyramid, colour, robust)
    assert len(want_records) == sum(ITERATIONS)
    for r in want_records:
        assert device_icp.unpack_record(r)["count"] > 0

    calls = []
    for name in SYMBOLS:
        def recorded(*args, _name=name, _entry=getattr(_lib.lib, name)):
            calls.append(_name)
            return _entry(*args)
        monkeypatch.setattr(_lib.lib, name, recorded)
    if tracker == "icp":
        joint = dict(colour_image=d["image"], prediction_colour=d["pc"]) if colour else {}
        twist, records, res = R.ProjectiveIcp3d(d["camera"], **settings).track(
            d["depth"], d["code"], d["pd"], d["pn"], TWIST_P, TWIST_P, residuals=True, **joint)
    else:
        joint = dict(colour=d["colour"], colour_image=d["image"]) if colour else {}
        twist, records, res = R.PointToSdf3d(d["camera"], **settings).track(
            d["depth"], d["code"], d["tsdf"], d["weight"], OFFSET, TWIST_P, voxel_size=VOXEL, residuals=True, **joint)
    monkeypatch.undo()
    assert calls == [ENTRY_POINTS[tracker, pyramid, colour, loss]]

    assert np.array_equal(twist.view(np.uint64), want_twist.view(np.uint64))
    assert len(records) == len(want_records)
    for got, raw in zip(records, want_records):
        want = device_icp.unpack_record(raw)
        assert got.keys() == want.keys()
        for field in want:
            a, b = np.asarray(got[field], np.float64), np.asarray(want[field], np.float64)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), field
    assert res.shape == want_res.shape and np.array_equal(_bits(res), _bits(want_res))
