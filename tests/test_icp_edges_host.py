"""CPU checks of the ragged, adversarial ICP pair (tests/icp_edge_scene.py): with the numpy restatement
(tests/icp_restatement.py) alone, the pair has the extents, the pairs, the solvable iterations and the rejection classes
that tests/test_gpu_icp_edges.py relies on.  The classes are counted by icp_edge_scene.rejection_classes, which does not
call icp_restatement.associate.  The pyramid and the photometric sources of lsf_icp.hip are out of scope here: they
have their own images and their tests are tests/test_gpu_depth_pyramid.py and tests/test_gpu_photometric.py."""
import numpy as np
import pytest

import icp_edge_scene as IS
import icp_restatement as I


def test_the_image_is_ragged():
    h, w = IS.IMAGE
    for s in IS.STRIDES[1:] + (16,):
        assert h % s and w % s
    # cells the residual store must clip: at the right edge, at the bottom edge, or at both
    assert any((w - 1) % s == 0 and s > 1 for s in IS.STRIDES) and any((w - 1) % s for s in IS.STRIDES)
    assert any((h - 1) % s == 0 and s > 1 for s in IS.STRIDES) and any((h - 1) % s for s in IS.STRIDES)


def test_the_prediction_carries_depth_with_a_zero_normal():
    pd, pn = IS.prediction()
    zero = ~pn.any(axis=2)
    filled = pd == np.float32(IS.FALLBACK)
    assert (pd > 0).all()  # every miss was filled
    assert int((zero & filled).sum()) >= 5 and int((zero & ~filled).sum()) >= 5  # from the fallback, and next to holes
    assert int((~zero).sum()) >= 200 and not (filled & ~zero).any()
    assert int((~filled).sum()) == IS.prediction_hits()


@pytest.mark.parametrize("kind", IS.LIVE_TYPES)
def test_the_live_frame_is_adversarial(kind):
    image, ratio = IS.live(kind)
    assert image.shape == IS.IMAGE and image.dtype == np.dtype(kind)
    assert ratio == {"float32": 0.5, "float64": 1.0, "uint16": 0.001}[kind]
    clean = IS.clean_live()
    assert int(((image == 0) & (clean > 0)).sum()) >= 40
    if kind != "uint16":
        assert int((image < 0).sum()) >= 40 and int(np.isnan(image).sum()) >= 40 and int(np.isposinf(image).sum()) >= 40
        assert not np.isfinite(image[-1, -1]) and not image[-2, -1] > 0 and not image[0, -1] > 0


@pytest.mark.parametrize("kind", IS.LIVE_TYPES)
def test_every_stride_has_pairs_and_a_solvable_iteration(kind):
    for stride in IS.STRIDES:
        rec, residuals, _ = IS.restated_iteration(kind, stride)
        assert rec["count"] >= (200 if stride == 1 else 5), (stride, rec["count"])
        assert rec["skipped"] == 0 and np.abs(rec["A"]).min() > 0
        # well-posed: sums in another order (1e-12 of A) move the step by far less than the twist tolerance of 1e-9
        assert np.linalg.cond(rec["A"]) < 1e6 and np.abs(rec["delta"]).max() < 0.05
        assert int((~np.isnan(residuals)).sum()) == rec["count"]
        off = np.ones(IS.IMAGE, bool)
        off[::stride, ::stride] = False
        assert np.isnan(residuals[off]).all()


@pytest.mark.parametrize("kind", IS.LIVE_TYPES)
def test_every_rejection_class_occurs(kind):
    image, ratio = IS.live(kind)
    classes = IS.rejection_classes(image, ratio, IS.start_twist(), 1)
    for name in ("not_positive", "outside", "zero_normal", "far"):
        assert classes[name] >= 5, classes
    assert sum(classes.values()) == image.size
    assert classes["paired"] == IS.restated_iteration(kind, 1)[0]["count"]  # the census and the restatement agree
    if kind != "uint16":
        assert int((~(I.scaled_depth(image, ratio) > 0)).sum()) == classes["not_positive"]
        assert classes["behind"] >= 5  # an infinite depth: q_z is inf or NaN, and NaN is not > 0


def test_the_whole_pass_keeps_pairs_at_every_level():
    records, twist = IS.restated_pass("float64")
    assert [r["level"] for r in records] == [0, 0, 1, 1, 2, 2, 2]
    assert all(r["count"] >= 5 and r["skipped"] == 0 for r in records)
    assert np.abs(twist - IS.twist_p() - IS.DELTA).max() < 0.01  # it stays near the live twist
