"""GPU check of what SequenceFusion3d.integrate asks of the library, frame by frame: in every configuration below the
names of the lsf_* symbols called while a frame is integrated, in order, equal a table of literals.  The table was
recorded with this file's recorder on the commit before the fusion package was split into one module per class
(fusion/__init__.py held every class then, and integrate was one method), so it pins the number and the order of the
launches and, with the record keys, the stages a frame passes.  Where the suite restates the same sequence the results
are held against the restatement as the modes' own tests hold them: the "icp" and "sdf" sequences, the fusion and the
prediction's hits of all four modes without a non-rigid step, and the sensor's registration records.

The scene is tests/test_gpu_tracker_entry_points.py's: three painted spheres and a plane seen by a 32 x 24 camera that
stands 0.25 m nearer than fusion_scene's, a 32^3 model of 8 mm voxels, ICP and point-to-SDF iterations (1, 1, 2); the
SDF-2-SDF modes run 3 rigid iterations and every non-rigid optimizer 3 iterations.  Frame 0 is fused at the first true
twist; the calls of frame 1 are recorded, and of frames 1 and 2 where a configuration has three frames.  The sensor
configuration runs tests/rgbd_rig_scene.py's rig, which has one size, into colour_scene's 64^3 volume."""
import functools

import numpy as np
import pytest

import colour_scene as CS
import fusion_restatement as F
import fusion_scene as S
import icp_restatement as I
import point_sdf_restatement as P
import raycast_restatement as RC
import rgbd_rig_scene as RS
import test_gpu_tracker_entry_points as E

pytestmark = pytest.mark.gpu

RIGID_ITERATIONS, NONRIGID_ITERATIONS = 3, 3
TWIST_ATOL = 1e-9  # tests/test_gpu_icp.py's and test_gpu_point_sdf.py's bound on a restated sequence's twists
PLAIN_KEYS = {"frame", "twist", "rigid_records", "nonrigid", "fusion", "prediction_hits"}
JUDGED_KEYS = PLAIN_KEYS | {"tracking_state", "tracking_quality"}
# the window of the moving volume keeps this camera point within 1.2 voxels of its centre: it is 0.875 voxels above the
# centre in y at frame 0 and 1.81 at frame 1's true twist, so frame 1 shifts by one voxel in y once the tracker has
# covered 35 % of the motion, and the row of the plane that leaves holds data
ANCHOR, THRESHOLD_VOXELS = (0.0, 0.003, 0.3), 1.2


@functools.lru_cache(maxsize=None)
def frames():
    """three (depth, colour image) pairs of the scene at the true twists 0, 1, 2; read-only"""
    out = []
    for k in range(3):
        depth, image, _ = CS.render(E.NEARER + S.true_twist(k), E.IMAGE[1], E.IMAGE[0], E.K)
        depth.setflags(write=False)
        image.setflags(write=False)
        out.append((depth, image))
    return tuple(out)


def _camera():
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=E.K), depth_unit_ratio=1.0)


def _sequence(fusion, mode, **kw):
    """a SequenceFusion3d of `fusion` (the package, or another that has its classes) on the scene"""
    from levelsetfusion_python_amd import rigid_opt
    levels = dict(iterations=E.ITERATIONS, max_distance=E.MAX_DISTANCE)
    settings = dict(voxel_size=E.VOXEL, initial_twist=E.TWIST_P, tracking_reference=mode,
                    rigid_iterations=RIGID_ITERATIONS)
    if mode == "icp":
        settings.update(icp_iterations=E.ITERATIONS, icp_strides=E.STRIDES, icp_max_distance=E.MAX_DISTANCE)
    if mode == "sdf":
        settings["sdf_tracker"] = rigid_opt.PointToSdf3d(_camera(), strides=E.STRIDES, **levels)
    settings.update(kw)
    return fusion.SequenceFusion3d(_camera(), E.N, E.OFFSET, **settings)


def _hierarchical(lsf):
    return lsf.HierarchicalOptimizer3d(tikhonov_term_enabled=True, gradient_kernel_enabled=False, maximum_chunk_size=8,
                                       rate=0.3, maximum_iteration_count=NONRIGID_ITERATIONS,
                                       maximum_warp_update_threshold=0.0, tikhonov_strength=0.05)


def _slavcheva(lsf, **kw):
    return lsf.SlavchevaOptimizer3d(field_size=E.N, compute_method=lsf.ComputeMethod.DIRECT,
                                    smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                                    maximum_warp_length_lower_threshold=0.0, max_iterations=NONRIGID_ITERATIONS,
                                    min_iterations=NONRIGID_ITERATIONS, **kw)


def _depth_only(count=2):
    return [(depth,) for depth, _ in frames()[:count]]


def _plain(mode):
    return lambda lsf, fusion: (_sequence(fusion, mode), _depth_only())


def _nonrigid(make, **kw):
    return lambda lsf, fusion: (_sequence(fusion, "model", nonrigid_optimizer=make(lsf, **kw)), _depth_only())


def _icp_colour(lsf, fusion):
    R = lsf.rigid_opt
    seq = _sequence(fusion, "icp", colour=True, carve=True, confidence=fusion.DepthConfidence(),
                    icp_pyramid=R.DepthPyramid(levels=E.LEVELS), icp_intensity_pyramid=R.IntensityPyramid(E.LEVELS),
                    photometric_weight=E.LAMBDA)
    return seq, list(frames()[:2])


def _sdf_lost(lsf, fusion):
    return _sequence(fusion, "sdf", tracking_quality=fusion.TrackingQuality(max_rms=0.0)), _depth_only()


def _icp_relocalised(lsf, fusion):
    """three frames, the second blank: it is lost, and the third is tracked again from the one keyframe's twist"""
    reloc = fusion.Relocaliser(ferns=64, decisions=4, coarse_shape=(6, 8), depth_range=(0.1, 2.0), max_keyframes=8)
    gate = fusion.TrackingQuality(min_pair_fraction=0.05)
    depth = _depth_only(3)
    return _sequence(fusion, "icp", relocaliser=reloc, tracking_quality=gate), [depth[0], (np.zeros_like(depth[1][0]),),
                                                                                 depth[2]]


def _sdf_moving(lsf, fusion):
    window = fusion.MovingVolume(THRESHOLD_VOXELS, ANCHOR, stream_mesh=False, keep_tsdf=True)
    return _sequence(fusion, "sdf", moving_volume=window), _depth_only()


def _sensor(lsf, fusion):
    sensor = fusion.RgbdSensor(*RS.cameras(), RS.DEPTH_TO_COLOUR, max_footprint=RS.MAX_FOOTPRINT)
    seq = fusion.SequenceFusion3d(None, CS.N, CS.offset(), sensor=sensor, colour=True, colour_band=CS.COLOUR_BAND,
                                  tracking_reference="icp", icp_iterations=E.ITERATIONS)
    return seq, [(depth.copy(), image.copy()) for depth, image in RS.raw_frames()[:2]]


# name -> a function of (the package, the namespace with the fusion classes) that gives a fresh sequence and its frames,
# each the arguments of one integrate call
CONFIGURATIONS = {
    "model": _plain("model"),
    "raycast": _plain("raycast"),
    "icp": _plain("icp"),
    "sdf": _plain("sdf"),
    "model, hierarchical": _nonrigid(_hierarchical),
    "model, cumulative warp": _nonrigid(_slavcheva, cumulative_warp=True, level_set_term_enabled=False),
    "model, volume mode": _nonrigid(_slavcheva),
    "icp, colour, carving, confidence, pyramids": _icp_colour,
    "sdf, lost": _sdf_lost,
    "icp, relocalised": _icp_relocalised,
    "sdf, moving volume with bricks": _sdf_moving,
    "sensor": _sensor,
}

_ITERATION = ["lsf_slavcheva_state_iteration"] * 2 + ["lsf_cumulative_warp_compose"] * 2
_LEVEL = ["lsf_hier_iteration"] * NONRIGID_ITERATIONS + ["lsf_records_decode"]
_ATTEMPT = ["lsf_raycast", "lsf_icp_run"]
# name -> the symbols called while integrate runs frame 1 (and frame 2 of a configuration with three frames), in order
CALLS = {
    "model": ["lsf_rigid3d_run", "lsf_fusion_integrate_depth"],
    "raycast": ["lsf_raycast", "lsf_rigid3d_gradient", "lsf_rigid3d_run", "lsf_fusion_integrate_depth"],
    "icp": _ATTEMPT + ["lsf_fusion_integrate_depth"],
    "sdf": ["lsf_point_sdf_run", "lsf_fusion_integrate_depth"],
    "model, hierarchical": (
        ["lsf_rigid3d_run", "lsf_rigid3d_gradient", "lsf_pack_live_gradient"] + ["lsf_restrict_mean"] * 6 + _LEVEL
        + (["lsf_prolong_repeat"] + _LEVEL) * 3 + ["lsf_interleave", "lsf_fusion_integrate_depth_warped"]),
    "model, cumulative warp": (
        ["lsf_rigid3d_run", "lsf_rigid3d_gradient", "lsf_state_prepare_scratch_elements", "lsf_state_prepare",
         "lsf_state_pack", "lsf_band_list_fill_prepared", "lsf_band_list_fill_prepared"]
        + _ITERATION * NONRIGID_ITERATIONS
        + ["lsf_state_finalize_scratch_elements", "lsf_state_finalize_listed", "lsf_records_decode",
           "lsf_state_unpack", "lsf_fusion_integrate_depth_warped"]),
    "model, volume mode": ["lsf_rigid3d_run", "lsf_rigid3d_gradient", "lsf_state_prepare_scratch_elements",
                           "lsf_state_run_begin", "lsf_state_run_rows_elements",
                           "lsf_state_finalize_scratch_elements", "lsf_state_run_finish_rows",
                           "lsf_fusion_integrate_volume"],
    "icp, colour, carving, confidence, pyramids": [
        "lsf_raycast_colour", "lsf_depth_pyramid", "lsf_intensity_pyramid", "lsf_intensity_pyramid",
        "lsf_icp_run_pyramid_photometric", "lsf_depth_confidence", "lsf_fusion_integrate_depth_colour"],
    "sdf, lost": ["lsf_point_sdf_run"],
    # the blank frame: tracked from the last good twist, then from the keyframe's; the next frame: not again from the
    # last good twist, from the keyframe's, fused, and offered as a keyframe
    "icp, relocalised": (["lsf_reloc_encode"] + _ATTEMPT + ["lsf_reloc_query"] + _ATTEMPT
                         + ["lsf_reloc_encode", "lsf_reloc_query"] + _ATTEMPT
                         + ["lsf_fusion_integrate_depth", "lsf_reloc_query"]),
    "sdf, moving volume with bricks": ["lsf_point_sdf_run", "lsf_fusion_integrate_depth", "lsf_volume_bricks_count",
                                       "lsf_volume_bricks_gather", "lsf_volume_shift"],
    "sensor": ["lsf_rgbd_rectify_colour", "lsf_rgbd_register_depth"] + _ATTEMPT
              + ["lsf_fusion_integrate_depth_colour"],
}


def recorded_frames(patch, seq, calls_of):
    """integrate every frame of calls_of's configuration; the names of the lsf_* symbols called from frame 1 on.  patch
    is a pytest MonkeyPatch: it is undone before this returns"""
    from levelsetfusion_python_amd import _lib
    calls = []
    for k, arguments in enumerate(calls_of):
        if k == 1:
            for name, (_, argtypes) in _lib.PROTOTYPES.items():
                if argtypes is None:
                    continue

                def recorded(*args, _name=name, _entry=getattr(_lib.lib, name)):
                    calls.append(_name)
                    return _entry(*args)
                patch.setattr(_lib.lib, name, recorded)
        seq.integrate(*arguments)
    patch.undo()
    return calls


def _bits_equal(t, want):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@functools.lru_cache(maxsize=None)
def restated(mode):
    """(twists, fusion records) of the restated two-frame "icp" or "sdf" sequence"""
    depths = [depth for depth, _ in frames()[:2]]
    sequence = I.sequence if mode == "icp" else P.sequence
    out = sequence(depths, E.K, 1.0, (E.N,) * 3, E.OFFSET, E.ITERATIONS, E.STRIDES, E.MAX_DISTANCE, voxel_size=E.VOXEL,
                   initial_twist=E.TWIST_P)
    return out[2], out[3]


def _check_plain(seq, mode):
    """the model of the restated fusion at the device's twists bit for bit and its fused counts; in "icp" and "sdf" mode
    the restated sequence's twists to TWIST_ATOL and its fused counts, and in "raycast" and "icp" mode the hits of the
    restated ray-cast of frame 0's model at the first twist.  The restated SDF-2-SDF tracker generates its live volumes
    with 4 mm voxels alone, so the suite restates no "model" or "raycast" sequence of this scene's 8 mm"""
    t, w = F.empty_model((E.N,) * 3)
    for k, (depth, _) in enumerate(frames()[:2]):
        frame = seq.frame_records[k]
        assert set(frame) == PLAIN_KEYS and frame["nonrigid"] is None
        if mode in ("icp", "sdf"):
            twists, records = restated(mode)
            np.testing.assert_allclose(seq.twists[k], twists[k], rtol=0, atol=TWIST_ATOL)
            assert frame["fusion"]["fused"] == records[k]["fused"]
        hits = None
        if k == 1 and mode == "icp":
            hits = RC.raycast(t, w, E.K, E.TWIST_P, E.OFFSET, E.VOXEL, E.IMAGE, normals=True)[2]
        if k == 1 and mode == "raycast":  # holes filled from frame 0
            hits = RC.raycast(t, w, E.K, E.TWIST_P, E.OFFSET, E.VOXEL, E.IMAGE, fallback=frames()[0][0], ratio=1.0)[2]
        assert frame["prediction_hits"] == hits
        t, w, want = F.fuse_depth(t, w, depth, E.K, 1.0, E.OFFSET, seq.twists[k], voxel_size=E.VOXEL)
        assert frame["fusion"]["fused"] == want["fused"]
    tracked = RIGID_ITERATIONS if mode in ("model", "raycast") else sum(E.ITERATIONS)
    assert len(seq.frame_records[1]["rigid_records"]) == tracked and not np.array_equal(seq.twists[1], seq.twists[0])
    assert _bits_equal(seq.canonical.tsdf, t) and _bits_equal(seq.canonical.weight, w)


def _check(lsf, name, seq):
    """the frame records' keys and what the configuration is there to show"""
    first, last = seq.frame_records[1], seq.frame_records[-1]
    if name in ("model", "raycast", "icp", "sdf"):
        _check_plain(seq, name)
    elif name.startswith("model, "):
        assert set(last) == PLAIN_KEYS and last["nonrigid"] is seq.nonrigid_optimizer.engine.last_call is not None
        warped = name != "model, volume mode"
        assert seq.warped == warped and (seq.warp is not None) == warped
        assert tuple(last["fusion"]) == (lsf.fusion.WARPED_RECORD_FIELDS if warped else lsf.fusion.RECORD_FIELDS)
    elif name == "icp, colour, carving, confidence, pyramids":
        assert set(last) == PLAIN_KEYS and tuple(last["fusion"]) == lsf.fusion.COLOUR_RECORD_FIELDS
        assert len(last["rigid_records"]) == sum(E.ITERATIONS) and "photometric_count" in last["rigid_records"][-1]
        assert seq.prediction_colour is not None and last["fusion"]["carved"] > 0 and last["fusion"]["coloured"] > 0
    elif name == "sdf, lost":
        assert set(last) == JUDGED_KEYS and last["tracking_state"] == seq.tracking_state == "lost"
        assert last["fusion"] is None and np.array_equal(seq.twists[1], seq.twists[0])
        assert len(last["rigid_records"]) == sum(E.ITERATIONS) and last["tracking_quality"]["rms"] > 0
    elif name == "icp, relocalised":
        assert all(set(r) == JUDGED_KEYS | {"relocalisation", "keyframe"} for r in seq.frame_records)
        assert [r["tracking_state"] for r in seq.frame_records] == ["tracking", "lost", "relocalised"]
        assert first["fusion"] is None and first["keyframe"] is None and first["relocalisation"]["chosen"] is None
        assert last["relocalisation"]["chosen"] == 0 and last["fusion"]["fused"] > 0
        assert seq.frame_records[0]["keyframe"] == 0
    elif name == "sdf, moving volume with bricks":
        assert set(last) == PLAIN_KEYS | {"shift", "streamed_faces", "bricks_out", "bricks_in"}
        assert seq.frame_records[0]["shift"] == (0, 0, 0) and last["shift"] != (0, 0, 0) and last["bricks_out"] > 0
        assert last["streamed_faces"] == 0 and len(seq.brick_store) > 0
        assert np.array_equal(seq.array_offset, seq.initial_array_offset + np.array(last["shift"], np.float64))
    else:
        assert name == "sensor" and set(last) == PLAIN_KEYS | {"registration"}
        for k, frame in enumerate(seq.frame_records):
            assert frame["registration"] == RS.restated_registration()[k][3]
        assert len(last["rigid_records"]) == sum(E.ITERATIONS) and last["fusion"]["coloured"] > 0


@pytest.mark.parametrize("name", sorted(CONFIGURATIONS))
def test_integrate_calls_the_library_as_tabled(monkeypatch, name):
    import levelsetfusion_python_amd as lsf
    seq, calls_of = CONFIGURATIONS[name](lsf, lsf.fusion)
    calls = recorded_frames(monkeypatch, seq, calls_of)
    print(name, calls)
    assert len(seq.frame_records) == len(calls_of) == (3 if name == "icp, relocalised" else 2)
    _check(lsf, name, seq)
    assert calls == CALLS[name]
    if name == "sdf, lost":  # a frame that is not fused calls no fusion symbol
        assert not any("fusion" in c for c in calls)
