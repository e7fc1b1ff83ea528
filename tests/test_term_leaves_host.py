"""Term-level drop-ins (data_term / smoothing_term / level_set_term), host side (no GPU needed): the reference's function
names are exported with its signatures, lsf_term_gradient refuses bad arguments before any launch, and without a GPU
every function raises the package's no-CPU-path error instead of computing on the CPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DATA_TERM = ["compute_data_term_gradient_vectorized", "compute_data_term_energy_contribution",
             "compute_data_term_gradient_direct", "compute_local_data_term_gradient_basic",
             "compute_local_data_term_gradient_thresholded_fdm", "data_term_at_location", "compute_local_data_term"]
SMOOTHING_TERM = ["compute_smoothing_term_gradient_vectorized", "compute_smoothing_term_energy",
                  "compute_smoothing_term_gradient_direct", "compute_local_smoothing_term_gradient_tikhonov",
                  "compute_local_smoothing_term_gradient_killing", "compute_local_smoothing_term_gradient"]


@pytest.fixture(scope="module")
def pkg():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_lsf_build_terms", os.path.join(ROOT, "levelsetfusion-python_amd",
                                                                                   "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(force=False, verbose=False)
    import levelsetfusion_python_amd as lsf
    return lsf


def test_term_modules_are_exported(pkg):
    for name in ("data_term", "smoothing_term", "level_set_term"):
        assert name in pkg.__all__ and inspect.ismodule(getattr(pkg, name))
    for name in DATA_TERM:
        assert callable(getattr(pkg.data_term, name)), name
    for name in SMOOTHING_TERM:
        assert callable(getattr(pkg.smoothing_term, name)), name
    assert callable(pkg.level_set_term.level_set_term_at_location)
    assert pkg.data_term.DataTermMethod.THRESHOLDED_FDM.value == 2
    assert pkg.smoothing_term.SmoothingTermMethod.KILLING.value == 1


def test_reference_signatures_and_defaults(pkg):
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    st, dt, lt = pkg.smoothing_term, pkg.data_term, pkg.level_set_term
    assert params(st.compute_local_smoothing_term_gradient_killing) == [
        ("warp_field", inspect.Parameter.empty), ("x", inspect.Parameter.empty), ("y", inspect.Parameter.empty),
        ("ignore_if_zero", False), ("copy_if_zero", True), ("isomorphic_enforcement_factor", 0.1)]
    assert params(st.compute_local_smoothing_term_gradient_tikhonov)[3:] == [
        ("ignore_if_zero", False), ("copy_if_zero", True), ("isomorphic_enforcement_factor", 0.1)]
    assert params(st.compute_smoothing_term_energy)[1:] == [("warped_live_field", None), ("canonical_field", None),
                                                            ("band_union_only", True)]
    assert params(dt.compute_data_term_gradient_vectorized)[4] == ("scaling_factor", 10.0)
    assert params(dt.compute_data_term_energy_contribution)[2] == ("band_union_only", True)
    assert params(dt.compute_data_term_gradient_direct)[4] == ("band_union_only", True)
    assert params(dt.compute_local_data_term)[-1] == ("method", dt.DataTermMethod.BASIC)
    assert params(lt.level_set_term_at_location) == [("warped_live_field", inspect.Parameter.empty),
                                                     ("x", inspect.Parameter.empty), ("y", inspect.Parameter.empty),
                                                     ("epsilon", 1e-5)]


def test_term_entry_point_validates_on_the_host(pkg):
    """lsf_term_gradient returns LSF_ERR_* before anything touches a device (the pointers below are never read)"""
    L = pkg._lib
    g2, g3 = L.Grid(2, 1, 8, 8, 0, 1, 0, 0), L.Grid(3, 4, 8, 8, 0, 4, 0, 0)

    def call(grid, term, flags=0, selection=L.SELECT_ALL, energy_form=L.TERM_ENERGY_LOCAL, live=1, canonical=1,
             warp=1, gradients=(1, 1, 1), indices=None, count=0):
        p = L.TermParams(0.1, 0.1, 1e-5, 10.0, term, flags, 0)
        return L.lib.lsf_term_gradient(live, canonical, *gradients, warp, 1, None, None, ctypes.byref(grid),
                                       ctypes.byref(p), selection, energy_form, indices, count, None)

    assert call(g3, L.TERM_KILLING, L.TERM_COPY_IF_ZERO) == -1          # copy_if_zero has 2-D semantics only
    assert call(g3, L.TERM_TIKHONOV_LOCAL, L.TERM_IGNORE_IF_ZERO) == -1
    assert call(g2, L.TERM_TIKHONOV, L.TERM_COPY_IF_ZERO) == -1         # the vectorised Tikhonov has no such flag
    assert call(g2, L.TERM_DATA_BASIC, 8) == -1                         # unknown flag
    assert call(g2, 6) == -1                                            # unknown term
    assert call(g2, L.TERM_KILLING, energy_form=L.TERM_ENERGY_NP_GRADIENT) == -1
    assert call(g2, L.TERM_KILLING, warp=None) == -1
    assert call(g2, L.TERM_DATA_BASIC, canonical=None) == -1
    assert call(g3, L.TERM_DATA_BASIC, gradients=(1, 1, None)) == -1    # 3-D data term: three gradient planes
    assert call(g2, L.TERM_TIKHONOV, selection=L.SELECT_BAND, live=None) == -1
    assert call(g2, L.TERM_LEVEL_SET, selection=L.SELECT_LIST, count=3) == -1  # a list without indices
    assert call(g2, L.TERM_LEVEL_SET, selection=3) == -1
    assert call(L.Grid(3, 4, 8, 8, 1, 4, 0, 0), L.TERM_LEVEL_SET) == -1  # not a whole array
    assert call(L.Grid(4, 1, 8, 8, 0, 1, 0, 0), L.TERM_LEVEL_SET) == -2


def test_no_cpu_execution_path(pkg, monkeypatch):
    import torch
    from levelsetfusion_python_amd import device_core
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(device_core, "_gpu_seen", False)
    f = np.zeros((6, 5), np.float32)
    w = np.zeros((6, 5, 2), np.float32)
    calls = [lambda: pkg.data_term.compute_data_term_gradient_vectorized(f, f, f, f),
             lambda: pkg.data_term.compute_data_term_energy_contribution(f, f),
             lambda: pkg.data_term.compute_data_term_gradient_direct(f, f, f, f),
             lambda: pkg.data_term.compute_local_data_term(f, f, 1, 1, f, f),
             lambda: pkg.data_term.compute_local_data_term_gradient_thresholded_fdm(f, f, 1, 1, f, f),
             lambda: pkg.data_term.data_term_at_location(f, f, 1, 1, f, f),
             lambda: pkg.smoothing_term.compute_smoothing_term_gradient_vectorized(w),
             lambda: pkg.smoothing_term.compute_smoothing_term_energy(w, f, f),
             lambda: pkg.smoothing_term.compute_smoothing_term_gradient_direct(w, f, f),
             lambda: pkg.smoothing_term.compute_local_smoothing_term_gradient(w, 1, 1),
             lambda: pkg.smoothing_term.compute_local_smoothing_term_gradient_killing(w, 1, 1),
             lambda: pkg.level_set_term.level_set_term_at_location(f, 1, 1)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            call()


def test_band_union_only_needs_the_fields(pkg):
    """the reference's ValueError comes before anything else, GPU or not"""
    with pytest.raises(ValueError, match="narrow band union"):
        pkg.smoothing_term.compute_smoothing_term_energy(np.zeros((4, 4, 2), np.float32))
