"""Term-level drop-ins (nonrigid_opt/slavcheva/{data_term,smoothing_term,level_set_term}.py) on the GPU: the reference's
known answers, the reference's own outputs on a 12x12 case, the oracle bit for bit in 2-D and 3-D, the reference's
copy_if_zero / ignore_if_zero behaviour against a per-voxel numpy restatement, tensors in / tensors out, and errors.
Run with  pytest -m gpu.  Tolerances as in test_gpu_parity.py: EXACT against the oracle, 1e-5 against the reference,
relative 1e-9 for float64 sums."""
import os

import numpy as np
import pytest
import torch

from oracle import lsf_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERALS = np.load(os.path.join(ROOT, "tests", "golden", "ref_test_literals.npz"))
PREFIXES = ("data_term.", "smoothing_term.")
CASES = sorted({k.rsplit(".", 1)[0] for k in LITERALS.files if k.startswith(PREFIXES)})
# the reference tests that zero the vectorised gradient outside the narrow-band union before comparing
MASKED = {"data_term.test_data_term02", "data_term.test_data_term03", "smoothing_term.test_smoothing_term02",
          "smoothing_term.test_smoothing_term03", "smoothing_term.test_smoothing_term04"}
ATOL = 1e-5


@pytest.fixture(scope="module")
def lsf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import levelsetfusion_python_amd as pkg
    return pkg


def maxdiff(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


class Case(dict):
    """the arrays of one reference test; records every key it hands out"""
    used = set()

    def __init__(self, name):
        super().__init__((k[len(name) + 1:], LITERALS[k]) for k in LITERALS.files if k.startswith(name + "."))
        self.name = name

    def __getitem__(self, key):
        Case.used.add(self.name + "." + key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default


def band_mask(live, canonical):
    return ~(O.is_truncated(live) & O.is_truncated(canonical))


def case_fields(c):
    """the fields every case of the reference test file names, and its expected gradient"""
    live = c.get("warped_live_field", c.get("live_field"))
    canonical = c.get("canonical_field")
    if live is not None:
        live, canonical = live.astype(np.float32), canonical.astype(np.float32)
    return live, canonical, c["expected_gradient_out"].reshape(-1, *c["expected_gradient_out"].shape[-3:])[0]


# ---------------------------------------------------------------------------------- 1. reference known answers
@pytest.mark.parametrize("name", CASES)
def test_reference_known_answers(lsf, name):
    c = Case(name)
    live, canonical, expected = case_fields(c)
    if name.startswith("data_term."):
        dt = lsf.data_term
        gy, gx = np.gradient(live)
        unmasked_only = "expected_gradient_out_band_union_only" in c
        out, energy = dt.compute_data_term_gradient_direct(live, canonical, gx, gy, band_union_only=not unmasked_only)
        assert maxdiff(out, expected) <= ATOL
        diff = (live - canonical).astype(np.float64)
        band = band_mask(live, canonical)
        expected_energy = 0.5 * float((diff[band] ** 2).sum()) if not unmasked_only else 0.5 * float((diff ** 2).sum())
        assert abs(energy - expected_energy) < 1e-6
        vec = dt.compute_data_term_gradient_vectorized(live, canonical, gx, gy)
        if name in MASKED:
            vec[~band] = 0.0
        assert maxdiff(vec, expected) <= ATOL
        assert abs(dt.compute_data_term_energy_contribution(live, canonical, band_union_only=not unmasked_only)
                   - expected_energy) < 1e-6
        if unmasked_only:
            expected_band = c["expected_gradient_out_band_union_only"]
            out, energy = dt.compute_data_term_gradient_direct(live, canonical, gx, gy, band_union_only=True)
            assert maxdiff(out, expected_band) <= ATOL
            assert abs(energy - 0.5 * float((diff[band] ** 2).sum())) < 1e-6
            vec[~band] = 0.0
            assert maxdiff(vec, expected_band) <= ATOL
    else:
        st = lsf.smoothing_term
        warp = c["warp_field"] if "warp_field" in c else (c["grad"] * np.float32(0.1)).astype(np.float32)
        with_band = live is not None
        out, energy = st.compute_smoothing_term_gradient_direct(warp, live, canonical, band_union_only=with_band)
        assert maxdiff(out, expected) <= ATOL
        vec = st.compute_smoothing_term_gradient_vectorized(warp)
        if name in MASKED:
            vec[~band_mask(live, canonical)] = 0.0
        assert maxdiff(vec, expected) <= ATOL
        band = band_mask(live, canonical) if with_band else np.ones(warp.shape[:-1], bool)
        e_vec = st.compute_smoothing_term_energy(warp, live, canonical, band_union_only=with_band)
        assert rel(e_vec, O.smoothing_energy_vectorized(warp, band)) < 1e-9
        assert rel(energy, float(O.tikhonov_energy_direct(warp)[band].astype(np.float64).sum())) < 1e-9


def test_every_reference_literal_is_used(lsf):
    for name in CASES:
        c = Case(name)
        case_fields(c)
        for key in list(c):
            if key in ("warp_field", "grad", "expected_gradient_out_band_union_only"):
                c[key]
    assert len(CASES) == 9
    assert Case.used == {k for k in LITERALS.files if k.startswith(PREFIXES)}


# ------------------------------------------------------------------------ 2. the reference's outputs on 12 x 12
def whole(lsf, term, **kw):
    """(gradient, per-voxel energy, energy total) of one term over a whole field, numpy out"""
    from levelsetfusion_python_amd import _lib, device_core, device_terms
    live, canonical, warp = (device_terms._device(kw.pop(k, None)) for k in ("live", "canonical", "warp"))
    gradients = [device_terms._device(g) for g in kw.pop("gradients", ())]
    shape = tuple(live.shape) if live is not None else tuple(warp.shape[:-1])
    dev = (live if live is not None else warp).device
    # NaN, not torch.empty: a recycled block may hold a same-shaped earlier call's right answer, and a location the
    # kernel never wrote would then pass
    g = torch.full(shape + (len(shape),), float("nan"), dtype=torch.float32, device=dev)
    e = torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    band = kw.pop("band", False)
    device_terms.term_gradient(term, device_core.make_grid(shape), live, canonical, gradients, warp, g, e, total,
                               selection=_lib.SELECT_BAND if band else _lib.SELECT_ALL, **kw)
    return g.cpu().numpy(), e.cpu().numpy(), float(total.item())


def at_every_location(f, shape):
    g = np.zeros(shape + (2,), np.float32)
    e = np.zeros(shape)
    for y in range(shape[0]):
        for x in range(shape[1]):
            g[y, x], e[y, x] = f(x, y)
    return g, e


def test_reference_outputs_12x12(lsf, ref_leaf):
    L = lsf._lib
    dt, st, lt = lsf.data_term, lsf.smoothing_term, lsf.level_set_term
    R = ref_leaf
    live, canonical, warp, steep = R["terms.live"], R["terms.canonical"], R["terms.warp"], R["terms.steep_live"]
    shape = live.shape
    gy, gx = np.gradient(live)
    sgy, sgx = np.gradient(steep)
    assert maxdiff(dt.compute_data_term_gradient_vectorized(live, canonical, gx, gy), R["terms.data_vectorized"]) == 0.0
    g, _ = at_every_location(lambda x, y: dt.compute_local_data_term_gradient_basic(live, canonical, x, y, gx, gy), shape)
    assert maxdiff(g, R["terms.data_basic"]) == 0.0
    g, _ = at_every_location(lambda x, y: dt.data_term_at_location(live, canonical, x, y, gx, gy), shape)
    assert maxdiff(g, R["terms.data_basic"]) == 0.0
    assert maxdiff(st.compute_smoothing_term_gradient_vectorized(warp), R["terms.tikhonov_vectorized"]) == 0.0
    assert rel(dt.compute_data_term_energy_contribution(live, canonical), float(R["terms.data_energy"])) < 1e-6
    assert rel(st.compute_smoothing_term_energy(warp, live, canonical),
               float(R["terms.smoothing_energy_vectorized"])) < 1e-6

    g, _ = at_every_location(lambda x, y: dt.compute_local_data_term(steep, canonical, x, y, sgx, sgy,
                                                                     method=dt.DataTermMethod.THRESHOLDED_FDM), shape)
    assert maxdiff(g, R["terms.data_fdm"]) <= ATOL
    assert maxdiff(whole(lsf, L.TERM_DATA_THRESHOLDED_FDM, live=steep, canonical=canonical, gradients=(sgx, sgy))[0],
                   R["terms.data_fdm"]) <= ATOL

    local = {"tikhonov_direct": (lambda x, y: st.compute_local_smoothing_term_gradient_tikhonov(
                 warp, x, y, copy_if_zero=False), lambda: whole(lsf, L.TERM_TIKHONOV_LOCAL, warp=warp)),
             "killing": (lambda x, y: st.compute_local_smoothing_term_gradient(
                 warp, x, y, copy_if_zero=False, method=st.SmoothingTermMethod.KILLING,
                 isomorphic_enforcement_factor=0.1), lambda: whole(lsf, L.TERM_KILLING, warp=warp)),
             "level_set": (lambda x, y: lt.level_set_term_at_location(live, x, y),
                           lambda: whole(lsf, L.TERM_LEVEL_SET, live=live))}
    for key, (per_location, whole_field) in local.items():
        g, e = at_every_location(per_location, shape)
        assert maxdiff(g, R["terms." + key]) <= ATOL, key
        assert maxdiff(e, R["terms.%s_energy" % key]) <= 1e-6, key
        g, e, total = whole_field()
        assert maxdiff(g, R["terms." + key]) <= ATOL, key
        assert maxdiff(e, R["terms.%s_energy" % key]) <= 1e-6, key
        assert rel(total, float(e.sum())) < 1e-9
    g, total = st.compute_smoothing_term_gradient_direct(warp, live, canonical, band_union_only=False)
    assert maxdiff(g, R["terms.tikhonov_direct"]) <= ATOL
    assert rel(total, float(R["terms.tikhonov_direct_energy"].sum())) < 1e-6


# ------------------------------------------------------------------------------- 3. the oracle, bit for bit
def rand_field(rng, shape, noise=0.05, slope=0.06):
    grids = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    f = slope * (grids[-2] - shape[-2] / 2) + 0.3 * np.sin(grids[-1] * 0.35) + noise * rng.standard_normal(shape)
    if len(shape) == 3:
        f = f + 0.2 * np.cos(grids[0] * 0.4)
    return np.clip(f, -1.0, 1.0).astype(np.float32)


TERM_CAP = 2048 * 256  # kTermMaxBlocks * kTermBlock, csrc/lsf_terms.hip: a lane of term_kernel loops past this count


def term_fields(shape, slope=0.06):
    """(live, canonical, warp) of the oracle comparisons; slope: of the fields along their second-to-last axis"""
    rng = np.random.default_rng(7)
    live = rand_field(rng, shape, slope=slope)
    canonical = rand_field(rng, shape, noise=0.08, slope=slope)
    warp = (0.4 * rng.standard_normal(shape + (len(shape),))).astype(np.float32)
    return live, canonical, warp


@pytest.mark.parametrize("shape", [(33, 70), (9, 20, 67)])
def test_terms_match_the_oracle(lsf, shape):
    assert_terms_match_the_oracle(lsf, shape)


def assert_terms_match_the_oracle(lsf, shape, slope=0.06):
    """every term over the whole field and over its band against the oracle, bit for bit; the oracle's terms are
    whole-array numpy (no per-location loop), so every location is compared at every shape.  Past TERM_CAP voxels the
    band and its complement must both reach into the second trip of the kernel's loop."""
    L = lsf._lib
    d = len(shape)
    live, canonical, warp = term_fields(shape, slope)
    grads = O.gradient(live)
    band = band_mask(live, canonical)
    assert 0 < band.sum() < band.size
    if band.size > TERM_CAP:
        past = band.reshape(-1)[TERM_CAP:]
        assert past.any() and not past.all()

    for method, term in ((O.BASIC, L.TERM_DATA_BASIC), (O.THRESHOLDED_FDM, L.TERM_DATA_THRESHOLDED_FDM)):
        expected, diff = O.data_term_gradient(live, canonical, method)
        g, e, total = whole(lsf, term, live=live, canonical=canonical, gradients=grads)
        assert maxdiff(g, expected) == 0.0
        e_ref = (np.float32(0.5) * (diff * diff)).astype(np.float32)
        assert maxdiff(e, e_ref) == 0.0
        assert rel(total, float(e_ref.astype(np.float64).sum())) < 1e-9
        g, _, total = whole(lsf, term, live=live, canonical=canonical, gradients=grads, band=True)
        assert maxdiff(g, np.where(band[..., None], expected, 0.0)) == 0.0
        assert rel(total, float(e_ref[band].astype(np.float64).sum())) < 1e-9
    dt = lsf.data_term
    extra = dict(live_gradient_z=grads[2]) if d == 3 else {}
    assert maxdiff(dt.compute_data_term_gradient_vectorized(live, canonical, grads[0], grads[1], **extra),
                   O.data_term_gradient(live, canonical)[0]) == 0.0
    out, energy = dt.compute_data_term_gradient_direct(live, canonical, grads[0], grads[1], **extra)
    diff = (live - canonical).astype(np.float32)
    e_band = (np.float32(0.5) * (diff * diff)).astype(np.float32)[band].astype(np.float64).sum()
    assert rel(energy, float(e_band)) < 1e-9
    assert rel(dt.compute_data_term_energy_contribution(live, canonical), float(e_band)) < 1e-9

    st = lsf.smoothing_term
    assert maxdiff(st.compute_smoothing_term_gradient_vectorized(warp), O.tikhonov_gradient(warp)) == 0.0
    g, e, total = whole(lsf, L.TERM_TIKHONOV, warp=warp)
    assert maxdiff(g, O.tikhonov_gradient(warp)) == 0.0
    assert maxdiff(e, O.tikhonov_energy_direct(warp)) == 0.0
    assert rel(total, float(O.tikhonov_energy_direct(warp).astype(np.float64).sum())) < 1e-9
    out, energy = st.compute_smoothing_term_gradient_direct(warp, live, canonical)
    assert maxdiff(out, np.where(band[..., None], O.tikhonov_gradient(warp), 0.0)) <= ATOL
    assert rel(energy, float(O.tikhonov_energy_direct(warp)[band].astype(np.float64).sum())) < 1e-9
    assert rel(st.compute_smoothing_term_energy(warp, live, canonical), O.smoothing_energy_vectorized(warp, band)) < 1e-9
    assert rel(st.compute_smoothing_term_energy(warp, band_union_only=False),
               O.smoothing_energy_vectorized(warp, np.ones(shape, bool))) < 1e-9

    kg, ke = O.killing_gradient(warp, 0.1)
    g, e, total = whole(lsf, L.TERM_KILLING, warp=warp, isomorphic_enforcement_factor=0.1)
    assert maxdiff(g, kg) == 0.0 and maxdiff(e, ke) == 0.0
    assert rel(total, float(ke.astype(np.float64).sum())) < 1e-9
    lg, le = O.level_set_gradient(live)
    g, e, total = whole(lsf, L.TERM_LEVEL_SET, live=live)
    assert maxdiff(g, lg) == 0.0 and maxdiff(e, le) == 0.0
    assert rel(total, float(le.astype(np.float64).sum())) < 1e-9


# ------------------------------------------------------------- 4. behaviour no fixture pins: a numpy restatement
F = np.float32


def restated_smoothing(warp, x, y, killing, copy_if_zero, ignore_if_zero, lam=0.1):
    """smoothing_term.py:50-139 at one voxel, float32, in the order the kernels use"""
    h, w = warp.shape[:2]
    centre = warp[y, x]

    def nb(xx, yy):
        if not (0 <= xx < w and 0 <= yy < h):
            return centre
        v = warp[yy, xx]
        return centre if copy_if_zero and F(v[0] * v[0] + v[1] * v[1]) == 0 else v

    if not killing and ignore_if_zero:
        for xx, yy in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
            if 0 <= xx < w and 0 <= yy < h and (warp[yy, xx] == 0).any():
                return np.zeros(2, F), 0.0
    xp, xm, yp, ym = nb(x + 1, y), nb(x - 1, y), nb(x, y + 1), nb(x, y - 1)
    gx, gy = F(0.5) * (xp - xm), F(0.5) * (yp - ym)
    if not killing:
        g = -((((xp + yp) - F(4) * centre) + xm) + ym)
        e = F(0.5) * F(F(F(gx[0] * gx[0] + gx[1] * gx[1]) + gy[0] * gy[0]) + gy[1] * gy[1])
        return g.astype(F), float(e)
    xx = (xp - F(2) * centre) + xm
    yy = (yp - F(2) * centre) + yp  # the reference's w_yy: the +1 neighbour twice
    xy = (((nb(x + 1, y + 1) - nb(x + 1, y - 1)) - nb(x - 1, y + 1)) + nb(x - 1, y - 1)) / F(4)
    c1, l32 = F(-2.0 * (1.0 + lam)), F(lam)
    g = np.array([(c1 * xx[0] + yy[0]) + l32 * xy[1], (c1 * xx[1] + yy[1]) + l32 * xy[0]], F)
    jac = np.array([gx[0], gx[1], gy[0], gy[1]], np.float64)
    e = jac.dot(jac) + lam * np.array([gx[0], gy[0], gx[1], gy[1]], np.float64).dot(jac)
    return g, float(e)


def zeroed_warp(rng, shape=(9, 11)):
    warp = (0.5 * rng.standard_normal(shape + (2,))).astype(F)
    warp[2, 3] = 0.0           # whole vectors
    warp[5, 5] = 0.0
    warp[0, 4] = 0.0           # on the border
    warp[4, 7, 0] = 0.0        # single components
    warp[6, 2, 1] = 0.0
    warp[8, 10, 0] = 0.0
    return warp


@pytest.mark.parametrize("killing, copy_if_zero, ignore_if_zero",
                         [(False, True, False), (False, False, True), (False, True, True), (True, True, False),
                          (True, True, True)])
def test_copy_and_ignore_if_zero(lsf, killing, copy_if_zero, ignore_if_zero):
    st = lsf.smoothing_term
    warp = zeroed_warp(np.random.default_rng(3))
    shape = warp.shape[:2]
    f = st.compute_local_smoothing_term_gradient_killing if killing else st.compute_local_smoothing_term_gradient_tikhonov
    g, e = at_every_location(lambda x, y: f(warp, x, y, ignore_if_zero=ignore_if_zero, copy_if_zero=copy_if_zero), shape)
    rg, re_ = at_every_location(lambda x, y: restated_smoothing(warp, x, y, killing, copy_if_zero, ignore_if_zero),
                                shape)
    assert maxdiff(g, rg) <= 1e-6
    assert maxdiff(e, re_) <= 1e-6
    L = lsf._lib
    wg, we, _ = whole(lsf, L.TERM_KILLING if killing else L.TERM_TIKHONOV_LOCAL, warp=warp,
                      copy_if_zero=copy_if_zero, ignore_if_zero=ignore_if_zero)
    assert maxdiff(wg, g) == 0.0 and maxdiff(we, e) == 0.0
    if copy_if_zero and not ignore_if_zero:  # the flag changes the result where a neighbour is zero
        plain, _ = at_every_location(lambda x, y: f(warp, x, y, copy_if_zero=False), shape)
        assert maxdiff(plain, g) > 1e-3


def test_data_terms_take_the_callers_gradients(lsf):
    dt = lsf.data_term
    rng = np.random.default_rng(11)
    shape = (10, 13)
    live = rand_field(rng, shape, noise=0.3)
    canonical = rand_field(rng, shape, noise=0.1)
    gx = (0.6 * rng.standard_normal(shape)).astype(F)  # not np.gradient(live): half of them above the 0.5 threshold
    gy = (0.6 * rng.standard_normal(shape)).astype(F)
    diff = (live - canonical).astype(F)

    def fdm(x, y, g, axis):
        if abs(g) <= 0.5:
            return g
        h, w = shape
        at = lambda xx, yy: live[yy, xx] if 0 <= xx < w and 0 <= yy < h else F(1)  # noqa: E731
        dx, dy = (1, 0) if axis == 0 else (0, 1)
        fwd, bwd = at(x + dx, y + dy) - live[y, x], live[y, x] - at(x - dx, y - dy)
        alt = fwd if abs(fwd) < abs(bwd) else bwd
        return F(0.0) if abs(alt) > 0.5 else alt

    for method in (dt.DataTermMethod.BASIC, dt.DataTermMethod.BASIC_CPP, dt.DataTermMethod.THRESHOLDED_FDM):
        for y in range(shape[0]):
            for x in range(shape[1]):
                g, e = dt.compute_local_data_term(live, canonical, x, y, gx, gy, method=method)
                lg = np.array([gx[y, x], gy[y, x]], F)
                if method == dt.DataTermMethod.THRESHOLDED_FDM:
                    lg = np.array([fdm(x, y, gx[y, x], 0), fdm(x, y, gy[y, x], 1)], F)
                assert np.array_equal(g, ((diff[y, x] * lg).astype(F) * F(10)).astype(F))
                assert e == float(F(0.5) * F(diff[y, x] * diff[y, x]))
    expected = np.stack([(diff * gx).astype(F) * F(3), (diff * gy).astype(F) * F(3)], axis=-1)
    assert maxdiff(dt.compute_data_term_gradient_vectorized(live, canonical, gx, gy, scaling_factor=3.0),
                   expected) == 0.0


# ----------------------------------------------------------------------------------- 5. devices and errors
def test_tensors_in_tensors_out(lsf):
    dt, st, lt = lsf.data_term, lsf.smoothing_term, lsf.level_set_term
    rng = np.random.default_rng(5)
    shape = (12, 15)
    live, canonical = rand_field(rng, shape), rand_field(rng, shape, noise=0.1)
    warp = zeroed_warp(rng, shape)
    gy, gx = np.gradient(live)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
    device = torch.device("cuda", torch.cuda.current_device())

    def same(t, a):
        assert isinstance(t, torch.Tensor) and t.device == device and t.dtype == torch.float32
        assert np.array_equal(t.cpu().numpy(), a)

    same(dt.compute_data_term_gradient_vectorized(T(live), T(canonical), T(gx), T(gy)),
         dt.compute_data_term_gradient_vectorized(live, canonical, gx, gy))
    (tg, te), (ng, ne) = (dt.compute_data_term_gradient_direct(T(live), T(canonical), T(gx), T(gy)),
                          dt.compute_data_term_gradient_direct(live, canonical, gx, gy))
    same(tg, ng)
    assert rel(te, ne) < 1e-9
    same(st.compute_smoothing_term_gradient_vectorized(T(warp)), st.compute_smoothing_term_gradient_vectorized(warp))
    tg, te = st.compute_smoothing_term_gradient_direct(T(warp), T(live), T(canonical))
    same(tg, st.compute_smoothing_term_gradient_direct(warp, live, canonical)[0])
    for (tg, te), (ng, ne) in (
            (st.compute_local_smoothing_term_gradient_killing(T(warp), 3, 4),
             st.compute_local_smoothing_term_gradient_killing(warp, 3, 4)),
            (dt.compute_local_data_term_gradient_basic(T(live), T(canonical), 5, 2, T(gx), T(gy)),
             dt.compute_local_data_term_gradient_basic(live, canonical, 5, 2, gx, gy)),
            (lt.level_set_term_at_location(T(live), 0, 7), lt.level_set_term_at_location(live, 0, 7))):
        same(tg, ng)
        assert te == ne and isinstance(ng, np.ndarray) and ng.dtype == np.float32 and ng.shape == (2,)


def test_errors(lsf):
    st, L = lsf.smoothing_term, lsf._lib
    from levelsetfusion_python_amd import device_core, device_terms
    w3 = np.zeros((4, 5, 6, 3), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        device_terms.term_field(L.TERM_KILLING, warp=w3, copy_if_zero=True)
    g = torch.empty((4, 5, 6, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(L.LsfHipError, match="LSF_ERR_BAD_ARGUMENT"):  # the library refuses it as well
        device_terms.term_gradient(L.TERM_KILLING, device_core.make_grid((4, 5, 6)), warp=torch.zeros_like(g),
                                   gradient_out=g, copy_if_zero=True)
    with pytest.raises(ValueError, match="narrow band union"):
        st.compute_smoothing_term_energy(np.zeros((4, 4, 2), np.float32))
    with pytest.raises(ValueError):
        st.compute_local_smoothing_term_gradient_killing(w3, 1, 1)  # the per-location functions are 2-D
    with pytest.raises(IndexError):
        st.compute_local_smoothing_term_gradient_tikhonov(np.zeros((4, 4, 2), np.float32), 4, 0)
    assert st.compute_smoothing_term_gradient_vectorized(w3).shape == (4, 5, 6, 3)  # whole fields take 3-D
