"""CPU checks of the SDF-2-SDF rigid tracker's host half: transformation known answers, the EXR reader, the numpy
restatement (tests/rigid_restatement.py) against the reference's answers and per-iteration records
(tests/golden/ref_rigid.npz, written by tests/golden/make_golden_rigid.py), host argument checks and the exports."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import rigid_restatement as R
from conftest import GOLDEN, ROOT, load_golden

PKG = os.path.join(ROOT, "levelsetfusion-python_amd")
FRAMES = [os.path.join(GOLDEN, n) for n in ("depth_000000.exr", "depth_000003.exr")]


def _load(name, rel):  # host modules of the package, without loading the HIP library
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("_t_transformation", os.path.join("math_utils", "transformation.py"))
IO = _load("_t_image_io", "image_io.py")


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_rigid.npz")


@pytest.mark.parametrize("k", range(1, 7))
def test_twist_vector_to_matrix2d_answers(ref, k):
    m = T.twist_vector_to_matrix2d(ref["twist2d.%02d.vector" % k] if k != 6 else -ref["twist2d.06.vector"])
    assert m.dtype == np.float64 and m.shape == (3, 3)
    assert np.allclose(ref["twist2d.%02d.expected" % k], m)


def test_twist_vector_to_matrix3d_answer(ref):
    v = ref["twist3d.01.vector"]
    m = T.twist_vector_to_matrix3d(v)
    assert m.dtype == np.float64 and m.shape == (4, 4)
    assert np.allclose(ref["twist3d.01.expected"], m)
    assert np.array_equal(m, ref["twist3d.01.reference_out"])
    assert np.array_equal(m, R.matrix3d(v))


def test_rodrigues_rounds_like_its_input():
    r32 = np.array([0.0, 0.3, 0.0], dtype=np.float32)
    assert T.rodrigues(r32).dtype == np.float32
    assert np.array_equal(T.rodrigues(r32), T.rodrigues(r32.astype(np.float64)).astype(np.float32))
    assert np.array_equal(T.rodrigues(np.zeros(3)), np.eye(3))
    m = T.twist_vector_to_matrix3d(np.array([1, 2, 3, 0, 0.5, 0], dtype=np.float32))
    assert m.dtype == np.float64 and m[0, 3] == 1 and np.float32(m[0, 0]) == m[0, 0]


def test_exr_reader_gives_the_fixture_frames(ref):
    for path in FRAMES:
        planes = IO.read_exr(path)
        assert sorted(planes) == ["B", "G", "R"] and planes["B"].shape == (480, 640)
        d = IO.read_depth_image(path)
        assert d.dtype == np.uint16
        assert np.array_equal(d, ref["frame.%s" % os.path.basename(path)])


def _exr(compression, pixel_type=1, flags=2, rows=2):
    def attr(name, kind, value):
        return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value
    ch = b"Y\0" + struct.pack("<iB3xii", pixel_type, 0, 1, 1) + b"\0"
    header = attr("channels", "chlist", ch) + attr("compression", "compression", bytes([compression])) + \
        attr("dataWindow", "box2i", struct.pack("<iiii", 0, 0, 3, rows - 1)) + b"\0"
    return struct.pack("<iI", IO.EXR_MAGIC, flags) + header


def _write_exr(tmp_path, compression, values):
    raw_rows = [np.asarray(r, dtype="<f2").tobytes() for r in values]
    head = _exr(compression, rows=len(values))
    chunks, rows_per = [], 1 if compression in (0, 2) else 16
    for y in range(0, len(raw_rows), rows_per):
        raw = b"".join(raw_rows[y:y + rows_per])
        if compression:
            t = bytearray(len(raw))
            half = (len(raw) + 1) // 2
            t[:half], t[half:] = raw[0::2], raw[1::2]
            p = bytearray(t)
            for i in range(len(t) - 1, 0, -1):
                p[i] = (t[i] - t[i - 1] + 128) & 0xFF
            packed = zlib.compress(bytes(p))
            raw = packed if len(packed) < len(raw) else raw  # OpenEXR stores a chunk raw when zlib does not shrink it
        chunks.append(struct.pack("<ii", y, len(raw)) + raw)
    table_len = 8 * len(chunks)
    offsets, pos = [], len(head) + table_len
    for c in chunks:
        offsets.append(pos)
        pos += len(c)
    path = tmp_path / ("c%d.exr" % compression)
    path.write_bytes(head + struct.pack("<%dQ" % len(offsets), *offsets) + b"".join(chunks))
    return str(path)


@pytest.mark.parametrize("compression", [0, 2, 3])
def test_exr_reader_none_zips_zip(tmp_path, compression):
    values = np.zeros((20, 4), dtype=np.float32)
    values[:2] = [[0, 1.5, 1000, 65504], [2, 3, 4, -1]]
    planes = IO.read_exr(_write_exr(tmp_path, compression, values))
    assert list(planes) == ["Y"] and np.array_equal(planes["Y"], values)


@pytest.mark.parametrize("compression,flags,pixel_type,what", [(4, 2, 1, "PIZ"), (0, 0x202, 1, "tiled"),
                                                               (0, 0x1002, 1, "multi-part"), (0, 2, 0, "pixel type")])
def test_exr_reader_refuses_what_it_does_not_cover(tmp_path, compression, flags, pixel_type, what):
    path = tmp_path / "bad.exr"
    path.write_bytes(_exr(compression, pixel_type, flags) + b"\0" * 64)
    with pytest.raises(ValueError, match=what):
        IO.read_exr(str(path))
    (tmp_path / "not.exr").write_bytes(b"garbage!")
    with pytest.raises(ValueError, match="not an OpenEXR"):
        IO.read_exr(str(tmp_path / "not.exr"))


def test_gray_refuses_colour_and_maps_zero():
    img = np.zeros((2, 2, 3), np.uint16)
    img[..., 2] = 7
    with pytest.raises(ValueError, match="colour"):
        IO.to_gray(img)
    same = np.full((2, 2, 3), 5, np.uint16)
    assert np.array_equal(IO.to_gray(same), np.full((2, 2), 5))


@pytest.mark.parametrize("k", range(1, 12))
def test_generation_restatement_equals_reference(ref, k):
    p = "gen.%02d." % k
    depth = ref[p + "depth"]
    n = int(ref[p + "field_size"])
    out = R.tsdf_nearest(depth, ref[p + "K"], float(ref[p + "ratio"]), (n, n), ref[p + "offset"], ref[p + "E"],
                         float(ref[p + "band"]), float(ref[p + "voxel"]), int(ref[p + "row"]), float(ref[p + "default"]))
    assert np.array_equal(out, ref[p + "out"])
    assert np.allclose(out, ref[p + "expected"])


@pytest.mark.parametrize("k", range(6))
def test_gradient_restatement_equals_reference(ref, k):
    p = "grad.%d." % k
    g = R.gradient_wrt_twist(ref[p + "live"], ref[p + "twist"], ref[p + "offset"], float(ref[p + "voxel_size"]))
    assert g.dtype == np.float32 and np.array_equal(g, ref[p + "out"])


# measured tolerances of the restatement (pairwise np.sum) against the reference's sequential loop
A_RTOL, TWIST_ATOL = 1e-12, 1e-9


@pytest.mark.parametrize("tag", ["test01", "same_cpp", "large", "singular", "flat"])
def test_optimizer_restatement_against_reference_records(ref, tag):
    p = "opt.%s." % tag
    K = ref[p + "K"]
    off = ref[p + "offset"]
    row, n = int(ref[p + "row"]), int(ref[p + "field_size"])
    d0 = ref["frame.depth_000000.exr"]
    d1 = ref["frame.depth_000003.exr"] if tag != "singular" else np.full((480, 640), np.inf)
    if tag == "flat":
        d0 = d1 = np.full((480, 640), 600, dtype=np.uint16)
    canonical = R.tsdf_nearest(d0, K, 0.001, (n, n), off, None, float(ref[p + "band"]), 0.004, row)
    records, twist = R.optimize(canonical, d1, K, 0.001, row, off, int(ref[p + "iterations"]), float(ref[p + "band"]),
                                float(ref[p + "eta"]))
    for i, rec in enumerate(records):
        assert rec["skipped"] == ref[p + "skipped"][i]
        np.testing.assert_allclose(rec["A"], ref[p + "A"][i], rtol=A_RTOL, atol=0)
        if not rec["skipped"]:
            np.testing.assert_allclose(rec["b"], ref[p + "b"][i], rtol=A_RTOL, atol=1e-300)
        np.testing.assert_allclose(rec["energy"], ref[p + "energy"][i], rtol=A_RTOL)
        np.testing.assert_allclose(rec["twist"], ref[p + "twist"][i], rtol=0, atol=TWIST_ATOL)
    np.testing.assert_allclose(twist.reshape(3, 1), ref[p + "final_twist"], rtol=0, atol=TWIST_ATOL)
    if tag == "test01":
        assert np.allclose(ref[p + "expected_twist"], twist.reshape(3, 1), atol=1e-6)


def test_singular_rule():
    """skip exactly where the reference's cond(A) is inf for the A a field pair can produce: zero, a zero row and
    column, non-finite; invert a nearly singular A, as the reference does"""
    assert R.singular_class(np.array([[1, 0, 0], [0, 9, 9], [0, 9, 15]])) == 0  # test_matrix_a_not_singular01
    assert np.isfinite(np.linalg.cond(np.array([[1, 0, 0], [0, 9, 9], [0, 9, 15]])))
    for a in (np.zeros((3, 3)), np.diag([1.0, 0, 1]), [[0, 0, 0], [0, 2, 1], [0, 1, 3]], [[5, 0, 1], [0, 0, 0], [1, 0, 3]]):
        a = np.array(a, dtype=np.float64)
        assert not np.isfinite(np.linalg.cond(a)) and R.singular_class(a) == 1
    assert R.singular_class(np.array([[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]])) == 1
    assert R.singular_class(np.array([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]])) == 1
    assert R.singular_class(np.diag([1e-300, 1.0, 1.0])) == 0
    # the documented difference: exactly singular, no zero row, cond ~1e16 (finite) -- the reference's np.linalg.inv
    # raises LinAlgError on it; the device skips the update
    a = np.array([[1.0, 2, 0], [2, 4, 0], [0, 0, 1]])
    assert np.isfinite(np.linalg.cond(a)) and R.singular_class(a) == 1
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv(a)


def test_package_exports_rigid_modules():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd.rigid_opt import sdf_2_sdf_optimizer2d, sdf_generation, sdf_gradient_field
    from levelsetfusion_python_amd.rigid_opt.sdf_2_sdf_visualizer import Sdf2SdfVisualizer
    assert lsf.transformation.twist_vector_to_matrix2d is not None and lsf.rigid_opt is not None
    assert lsf.Sdf2SdfOptimizer2d is sdf_2_sdf_optimizer2d.Sdf2SdfOptimizer2d
    assert callable(sdf_gradient_field.calculate_gradient_wrt_twist)
    assert sdf_generation.ImageBasedSingleFrameDataset and sdf_generation.ArrayBasedSingleFrameDataset
    v = Sdf2SdfVisualizer(Sdf2SdfVisualizer.Parameters(out_path="nowhere", save_initial_fields=True,
                                                       save_final_fields=True, save_live_progression=True))
    v.generate_pre_optimization_visualizations(None, None)
    v.generate_per_iteration_visualizations(None)
    assert not os.path.exists("nowhere")
    p = sdf_2_sdf_optimizer2d.Sdf2SdfOptimizer2d.VerbosityParameters(True, False)
    assert p.print_per_iteration_info and sdf_2_sdf_optimizer2d.Sdf2SdfOptimizer2d().rate == 0.5


def test_host_argument_checks():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd.tsdf.generation import offsets_of
    from levelsetfusion_python_amd import device_rigid
    with pytest.raises(ValueError, match="3 entries"):
        offsets_of([1, 2])
    assert np.array_equal(offsets_of(np.array([[-16], [-16], [93.4375]])), [-16, -16, 93.4375])
    with pytest.raises(ValueError, match="3 entries"):
        device_rigid.twist3(np.zeros(6))
    with pytest.raises(ValueError, match="6 entries"):
        lsf.transformation.twist_vector_to_matrix3d(np.zeros(3))
    with pytest.raises(ValueError, match="3 entries"):
        lsf.transformation.rodrigues(np.zeros(4))


def test_report_text_of_both_optimizers(capsys):
    """the verbosity prints of Sdf2SdfOptimizer2d and Sdf2SdfOptimizer3d, from host-built records: the reference's 2-D
    text, and the 6-DoF text with the same format, which at three components is the 2-D text byte for byte"""
    from levelsetfusion_python_amd.rigid_opt import sdf_2_sdf_optimizer2d as O2, sdf_2_sdf_optimizer3d as O3

    def records(n, size):
        out = []
        for k, skipped in enumerate((0, 1, 0)):
            r = np.zeros(size)
            r[:2 * n] = 0.125 * (np.arange(2 * n) + 1) * (-1) ** k
            r[2 * n] = 1234.5 / (k + 1)
            r[2 * n + 1 + n * n + n] = skipped
            out.append(r)
        return out

    def report(cls, recs):
        verbose = cls.VerbosityParameters(print_max_warp_update=True, print_iteration_energy=True)
        cls(verbosity_parameters=verbose)._report(recs)
        return capsys.readouterr().out

    text2 = report(O2.Sdf2SdfOptimizer2d, [O2.unpack_record(r) for r in records(3, 24)])
    c, y, z = "\033[36;1;m", "\033[33;1;m", "\033[0m"
    assert text2 == (
        c + "[ITERATION 0 COMPLETED]" + z + " energy: 1234.500000\n"
        "optimal twist: 0.125000, 0.250000, 0.375000, twist: 0.500000, 0.625000, 0.750000\n" +
        c + "[ITERATION 1 COMPLETED]" + z + " energy: 617.250000\n" + y + "SINGULAR MATRIX!" + z + "\n" +
        c + "[ITERATION 2 COMPLETED]" + z + " energy: 411.500000\n"
        "optimal twist: 0.125000, 0.250000, 0.375000, twist: 0.500000, 0.625000, 0.750000\n")
    assert report(O3.Sdf2SdfOptimizer3d, [O2.unpack_record(r) for r in records(3, 24)]) == text2
    text3 = report(O3.Sdf2SdfOptimizer3d, [O3.unpack_record(r) for r in records(6, 64)])
    assert text3.splitlines()[1] == ("optimal twist: 0.125000, 0.250000, 0.375000, 0.500000, 0.625000, 0.750000, "
                                     "twist: 0.875000, 1.000000, 1.125000, 1.250000, 1.375000, 1.500000")
    assert text3.splitlines()[2:4] == text2.splitlines()[2:4]
