"""CPU checks of the weighted fusion rule with free-space carving on its numpy restatement
(tests/fusion_weighted_restatement.py): it is the unweighted rule when nothing is asked of it, carving removes a
surface that a later frame looks through after one frame, and the host refuses bad settings before touching the GPU."""
import numpy as np
import pytest

import fusion_restatement as F
import fusion_scene as S
import fusion_weighted_restatement as FW
import ghost_scene as G

BAND, VOXEL = 20, 0.004
ZERO = np.zeros(6)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def ghost():
    """frames A (with the ghost) and B (without), and the model after A, shared and never written"""
    off = S.offset(G.N)
    a, b = G.with_ghost(), G.plain()
    t, w, rec = FW.fuse_depth_weighted(*F.empty_model((G.N,) * 3), a, G.K, 1.0, off, ZERO)
    for x in (a, b, t, w):
        x.setflags(write=False)
    return {"A": a, "B": b, "off": off, "tsdf": t, "weight": w, "record": rec}


@pytest.mark.parametrize("ones", [False, True])
def test_restatement_without_weights_or_carving_is_the_unweighted_rule(ghost, ones):
    rng = np.random.default_rng(3)
    shape = (G.N,) * 3
    t = rng.uniform(-1, 1, shape).astype(np.float32)
    t.reshape(-1)[::13] = 1.0
    w = rng.choice(np.array([0, 0, 1, 2.5, 5, 8], np.float32), shape)
    twist = np.array([0.003, -0.002, 0.002, 0.01, -0.012, 0.008])
    pw = np.ones(ghost["A"].shape, np.float32) if ones else None
    got = FW.fuse_depth_weighted(t, w, ghost["A"], G.K, 1.0, ghost["off"], twist, BAND, VOXEL, 0.5, 8.0, pw, False)
    want = F.fuse_depth(t, w, ghost["A"], G.K, 1.0, ghost["off"], twist, BAND, VOXEL, 0.5, 8.0)
    assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
    assert {k: got[2][k] for k in want[2]} == want[2] and want[2]["fused"] > 1000
    assert got[2]["carved"] == 0 and got[2]["weight_rejected"] == 0


def test_the_ghost_is_placed_as_the_scenario_needs(ghost):
    """inside the volume, clear of the other spheres' silhouettes, its far side in front of the back plane's band"""
    half = BAND / 2 * VOXEL
    lo = S.offset(G.N) * VOXEL
    hi = (S.offset(G.N) + G.N - 1) * VOXEL
    assert np.all(G.GHOST_CENTRE - G.GHOST_RADIUS > lo) and np.all(G.GHOST_CENTRE + G.GHOST_RADIUS < hi)
    assert G.GHOST_CENTRE[2] + G.GHOST_RADIUS < S.PLANE_Z - half
    silhouette = np.isfinite(G.sphere_depth(G.GHOST_CENTRE, G.GHOST_RADIUS))
    assert silhouette.sum() > 100 and np.array_equal(silhouette, ghost["A"] != ghost["B"])
    others = np.zeros_like(silhouette)
    for c, r in S.SPHERES:
        others |= np.isfinite(G.sphere_depth(c, r))
    assert not np.any(silhouette & others)
    assert G.in_ghost().sum() > 500


def test_a_ghost_stays_without_carving_and_goes_after_one_carving_frame(ghost):
    ball = G.in_ghost()
    assert np.any(ghost["tsdf"][ball] < 0)  # frame A put a surface there
    model = (ghost["tsdf"], ghost["weight"])
    kept_t, kept_w, kept = FW.fuse_depth_weighted(*model, ghost["B"], G.K, 1.0, ghost["off"], ZERO, carve=False)
    assert np.any(kept_t[ball] < 0) and kept["carved"] == 0
    t, w, rec = FW.fuse_depth_weighted(*model, ghost["B"], G.K, 1.0, ghost["off"], ZERO, carve=True)
    # a fused value t0 is > -1, and one frame of +1 at equal weight gives (t0 + 1) / 2 > 0
    assert np.all(t[ball] > 0)
    assert rec["carved"] > 0 and rec["fused"] == kept["fused"] and rec["weight_rejected"] == 0
    assert rec["first_seen"] > kept["first_seen"]
    # in-band voxels do not depend on carving
    carved = w != kept_w
    assert np.count_nonzero(carved) == rec["carved"] and _bits_equal(t[~carved], kept_t[~carved])
    # voxels without a valid pixel -- here behind a patch of holes -- are untouched
    holes = ghost["B"].copy()
    holes[10:40, 30:90] = 0
    t, w, rec = FW.fuse_depth_weighted(*model, holes, G.K, 1.0, ghost["off"], ZERO, carve=True)
    _, _, valid = FW.pixel_of_voxels(holes, G.K, 1.0, t.shape, ghost["off"], ZERO)
    assert np.count_nonzero(~valid) > 1000 and rec["carved"] > 0
    assert _bits_equal(t[~valid], ghost["tsdf"][~valid]) and _bits_equal(w[~valid], ghost["weight"][~valid])


def test_weights_that_are_not_finite_and_positive_reject_their_voxels(ghost):
    pw = np.ones(ghost["B"].shape, np.float32)
    pw[::2, ::3] = 0.0
    pw[1::4, 1::3] = np.nan
    pw[3::4, 2::3] = np.inf
    pw[2::4, ::5] = -1.0
    model = (ghost["tsdf"], ghost["weight"])
    t, w, rec = FW.fuse_depth_weighted(*model, ghost["B"], G.K, 1.0, ghost["off"], ZERO, pixel_weight=pw, carve=True)
    _, _, full = FW.fuse_depth_weighted(*model, ghost["B"], G.K, 1.0, ghost["off"], ZERO, carve=True)
    assert rec["weight_rejected"] > 0
    assert rec["fused"] + rec["carved"] + rec["weight_rejected"] == full["fused"] + full["carved"]
    assert np.all(np.isfinite(t)) and np.all(np.isfinite(w))
    iy, ix, _ = FW.pixel_of_voxels(ghost["B"], G.K, 1.0, t.shape, ghost["off"], ZERO)
    bad = ~(pw[iy, ix] > 0) | ~np.isfinite(pw[iy, ix])
    assert _bits_equal(t[bad], ghost["tsdf"][bad]) and _bits_equal(w[bad], ghost["weight"][bad])


def test_restated_confidence():
    """frontal at the reference depth counts 1; beyond it (z_ref / z)^2; grazing less; holes and no-normal pixels 0"""
    K = np.array([[100.0, 0, 1], [0, 100.0, 1], [0, 0, 1]])
    depth = np.array([[0.5, 1.0, 0.0], [0.25, np.nan, 0.5], [0.5, 0.5, 0.5]], np.float32)
    normals = np.zeros((3, 3, 3), np.float32)
    normals[..., 2] = -1.0
    normals[2, 0] = 0.0
    normals[2, 1] = (np.sqrt(0.5), 0.0, -np.sqrt(0.5))
    c = FW.confidence(depth, normals, K, 0.5)
    assert c.dtype == np.float32 and c[1, 1] == 0 and c[0, 2] == 0 and c[2, 0] == 0
    assert c[1, 1 - 1] == np.float32(1.0 / np.sqrt(1.0 + 1e-4))  # nearer than the reference: the cosine alone
    assert c[0, 1] == np.float32(0.25 / np.sqrt(1.0 + 1e-4))
    # two float32 roundings (the normal's components, the result): 2^-23 relative at the most
    np.testing.assert_allclose(c[2, 1], np.sqrt(0.5) / np.sqrt(1.0 + 1e-4), rtol=2.0 ** -23)


def test_host_refuses_bad_settings_before_the_gpu():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="reference_depth"):
            lsf.fusion.DepthConfidence(reference_depth=bad)
    with pytest.raises(ValueError, match="DepthPyramid"):
        lsf.fusion.DepthConfidence(pyramid=3)
    c = lsf.fusion.DepthConfidence(0.75, lsf.rigid_opt.DepthPyramid(levels=2, radius=2))
    assert c.reference_depth == 0.75 and c.pyramid.radius == 2
    assert c.shares(lsf.rigid_opt.DepthPyramid(levels=3, radius=2)) and not c.shares(lsf.rigid_opt.DepthPyramid())
    assert not c.shares(None)
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    for kw in (dict(carve=True), dict(confidence=lsf.fusion.DepthConfidence())):
        with pytest.raises(ValueError, match="nonrigid_optimizer"):
            lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=object(), **kw)
    with pytest.raises(ValueError, match="DepthConfidence"):
        lsf.SequenceFusion3d(cam, 32, S.offset(32), confidence=0.5)
    rec = lsf.fusion.unpack_weighted_record(np.array([5, 2, 1.5, 0.75, 7, 3, 0, 0], np.float64))
    assert rec == {"fused": 5, "first_seen": 2, "sum_abs_change": 1.5, "max_abs_change": 0.75, "carved": 7,
                   "weight_rejected": 3}
    assert lsf.fusion.RECORD_FIELDS == ("fused", "first_seen", "sum_abs_change", "max_abs_change")
