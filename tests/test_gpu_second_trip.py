"""GPU checks of the second trip of every capped-grid loop outside the KillingFusion hot path, against the restatements
the first trip is already compared with ("Capped grids and the tests that cross them").  A kernel that
launches at most a fixed number of workgroups lets a workgroup or a lane loop to a second item past that cap, and a
one-workgroup pass loops over more partials than it has lanes.  Every test here first asserts, from a restatement of the
kernel's work split, that its shape crosses the cap -- a later change of a cap fails that line instead of silently
emptying the test -- and that work with an effect lies past it, then compares as the first-trip tests do: bit for bit
per voxel, counts and maxima exactly, float64 sums to the existing relative bounds.  The shapes are the smallest that
cross.  Sections 7 to 15 (the relocaliser, the brick store) compare bits, codes, counts, ids and records exactly; their
inputs and crossing assertions live in tests/test_relocaliser_host.py and tests/test_volume_bricks_host.py, which check
them without a card."""
import functools

import numpy as np
import pytest
import torch

import fusion_restatement as F
import fusion_weighted_restatement as FW
import mesh_restatement as M
import relocaliser_restatement as R
import rigid3d_restatement as R3
import test_relocaliser_host as RH
import test_volume_bricks_host as BH
import volume_bricks_restatement as B
from test_gpu_fusion import SUM_RTOL
from test_gpu_fusion import _assert_record as _assert_fusion_record
from test_gpu_fusion import _host_record, _random_live, _random_model
from test_gpu_fusion_weighted import SUM_RTOL as WEIGHTED_SUM_RTOL
from test_gpu_fusion_weighted import _assert_record as _assert_weighted_record
from test_gpu_fusion_weighted import _random_weights, _unpack
from test_gpu_mesh import _check as _check_mesh
from test_gpu_relocaliser import _bits as _relocaliser_bits
from test_gpu_relocaliser import _cuda, _run_query, encode_twice_against, query_comparison
from test_gpu_rigid3d import A_RTOL, TWIST_ATOL, TWISTS, _bits_equal, _camera, _depth, _run, _teacher_forced
from test_gpu_term_leaves import TERM_CAP, assert_terms_match_the_oracle, maxdiff, rel, term_fields
from test_gpu_volume_bricks import count_and_gather_against_restatement, round_trip, scatter_against_restatement
from test_rigid3d_host import K_SYN, XI0

pytestmark = pytest.mark.gpu

assert SUM_RTOL == WEIGHTED_SUM_RTOL == 1e-12 and A_RTOL == 1e-12 and TWIST_ATOL == 1e-9


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _device(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


# ------------------------------------------------------------------------------------------ 1. rigid3d: the item loop
RIGID3D_MAX_BLOCKS, RIGID3D_TILE, RIGID3D_MIN_CHUNK = 256, 16, 4  # kMaxBlocks, kRT, kMinChunk of csrc/lsf_rigid3d.hip
# (Z, Y, X), the array offset that puts the synthetic depth image's surface (z = 250 voxels) through it, items, z-chunk
RIGID_VOLUMES = {"two-chunks": ((5, 160, 240), np.array([-120.5, -80.25, 247.75]), 300, 4),
                 "wide": ((8, 272, 272), np.array([-136.5, -200.25, 246.75]), 289, 8)}


def _rigid3d_items(shape):
    """convert() of csrc/lsf_rigid3d.hip: (items, z extent of an item); the loop is
    `for (item = blockIdx.x; item < p.items; item += gridDim.x)` on min(items, kMaxBlocks) workgroups"""
    nz, ny, nx = shape
    tiles = -(-nx // RIGID3D_TILE) * -(-ny // RIGID3D_TILE)
    zc = min(max(-(-nz * tiles // RIGID3D_MAX_BLOCKS), RIGID3D_MIN_CHUNK), nz)
    return tiles * -(-nz // zc), zc


def _rigid_volume(name):
    shape, off, items, zc = RIGID_VOLUMES[name]
    assert _rigid3d_items(shape) == (items, zc) and items > RIGID3D_MAX_BLOCKS  # some workgroups take a second item
    if name == "two-chunks":  # item = chunk * tiles + tile: workgroup b's second item b + 256 lies in the other z-chunk
        assert -(-shape[0] // zc) == 2 and items // 2 <= RIGID3D_MAX_BLOCKS
    return shape, off


def _second_items(shape):
    """the voxels of items >= kMaxBlocks, the ones a workgroup reaches on its second trip: item = chunk * tiles + tile,
    tile = (y / kRT) * tiles_x + x / kRT (the item loop's first lines)"""
    zc = _rigid3d_items(shape)[1]
    z, y, x = np.meshgrid(*(np.arange(v) for v in shape), indexing="ij")
    tiles_x = -(-shape[2] // RIGID3D_TILE)
    tile = (y // RIGID3D_TILE) * tiles_x + x // RIGID3D_TILE
    return (z // zc) * (tiles_x * -(-shape[1] // RIGID3D_TILE)) + tile >= RIGID3D_MAX_BLOCKS


def _assert_banded(live):
    """at least 1000 voxels strictly inside (-1, 1), and as many among the second items alone: a constant field there
    has no gradient and adds exactly 0 to A, b and the energy, so a skipped second item would change nothing; and the
    device allocates the live and gradient outputs itself, so only values that differ from item to item tell a written
    second item from a stale one"""
    banded = (live > -1) & (live < 1)
    assert np.count_nonzero(banded) >= 1000 and np.count_nonzero(banded & _second_items(live.shape)) >= 1000


@pytest.mark.parametrize("name,depth_dtype", [("two-chunks", np.uint16), ("wide", np.float32)])
def test_rigid3d_live_and_gradient_from_depth(lsf, name, depth_dtype):
    from levelsetfusion_python_amd import device_rigid
    from levelsetfusion_python_amd.tsdf import generation as gen
    shape, off = _rigid_volume(name)
    d = _depth(depth_dtype)
    dev, code = gen.device_depth(d)
    twist = TWISTS[1]
    want = R3.live_volume(d, K_SYN, 0.001, shape, off, twist)
    _assert_banded(want)
    live, grad = device_rigid.live_and_gradient_3d(dev, code, _camera(K_SYN), shape, off, twist)
    assert _bits_equal(live.cpu().numpy(), want)
    assert _bits_equal(grad.cpu().numpy(), R3.gradient_wrt_twist_3d(want, twist, off))


@pytest.mark.parametrize("name", list(RIGID_VOLUMES))
def test_rigid3d_gradient_of_a_given_volume(lsf, name):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist_3d
    shape, off = _rigid_volume(name)
    live = np.clip(np.random.default_rng(11).normal(0, 0.7, shape), -1, 1).astype(np.float32)
    _assert_banded(live)
    for twist in TWISTS[1:3]:
        g = calculate_gradient_wrt_twist_3d(live, twist.reshape(6, 1), off, 0.004)
        assert g.dtype == np.float32 and g.shape == shape + (6,)
        assert _bits_equal(g, R3.gradient_wrt_twist_3d(live, twist, off, 0.004))


@pytest.mark.parametrize("name,depth_dtype", [("two-chunks", np.float32), ("wide", np.uint16)])
def test_rigid3d_run_teacher_forced(lsf, name, depth_dtype):
    """three iterations from a non-zero start: every workgroup's partial holds the sums of both of its items"""
    shape, off = _rigid_volume(name)
    depth = _depth(depth_dtype)
    canonical = R3.live_volume(depth, K_SYN, 0.001, shape, off, XI0)
    _assert_banded(canonical)
    start = np.array([0.001, 0.0, -0.001, 0.0, 0.01, 0.0])
    _assert_banded(R3.live_volume(depth, K_SYN, 0.001, shape, off, start))
    twist, records = _run(canonical, depth, _camera(K_SYN), off, 3, twist=start)
    assert records.shape == (3, 64) and not np.any(records[:, 55])
    _teacher_forced(records, canonical, depth, K_SYN, off, start=start)
    _, want = R3.optimize(canonical, depth, K_SYN, 0.001, off, 3, 20., twist=start)
    np.testing.assert_allclose(twist, want, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1, 6:12])


# -------------------------------------------------------------------------- 2, 3. fusion: the finish pass, the grid-stride
FUSION_BLOCK, FUSION_MAX_BLOCKS = 256, 2048  # kBlock (csrc/lsf_device.h), LSF_FUSION_MAX_BLOCKS (include/lsf_hip.h)
FUSION_CAP = 4 * FUSION_BLOCK * FUSION_MAX_BLOCKS  # voxels of the first trip: 2^21
FUSION_BIG = (131, 133, 139)
# the surface (z = 250 voxels, +-16 of tilt and a 15-voxel bump towards the camera) lies at z index 131 of 131: its
# 20-voxel band takes the planes from 114 on (flat index >= 2^21) and leaves seen free space in front of it there
FUSION_BIG_OFF = np.array([-69.5, -66.25, 118.75])
FUSION_TWIST = np.array([0.013, -0.021, 0.008, 0.05, -0.17, 0.11])


def _fusion_split(shape):
    """convert() of csrc/lsf_fusion.hip: (4-voxel groups, tail voxels, workgroups = partials).  The one walk kernel,
    fusion_kernel<RULE>, loops `for (g = blockIdx.x * kBlock + threadIdx.x; g < p.groups; g += gridDim.x * kBlock)`
    under every rule, and fusion_finish_kernel
    `for (q = threadIdx.x; q < nblocks; q += kBlock)`"""
    n = int(np.prod(shape))
    groups = n // 4
    return groups, n % 4, min(max(-(-groups // FUSION_BLOCK), 1), FUSION_MAX_BLOCKS)


def _assert_second_trip_changes(before, after):
    """more than 1000 voxels of the second trip change, some of them among the first workgroup's 1024 voxels past the
    cap (a stride that is off by a block skips exactly those)"""
    changed = before.reshape(-1).view(np.uint32) != after.reshape(-1).view(np.uint32)
    assert np.count_nonzero(changed[FUSION_CAP:]) > 1000
    assert np.count_nonzero(changed[FUSION_CAP:FUSION_CAP + 4 * FUSION_BLOCK]) > 100


def _volume_mode(lsf, shape, w, cap, seed):
    rng = np.random.default_rng(seed)
    t, W = _random_model(shape, rng, cap)
    live = _random_live(shape, rng)
    vol = lsf.fusion.CanonicalVolume(shape, max_weight=cap)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(W))
    rec = vol.integrate_volume(live, weight=w)
    want_t, want_w, want_rec = F.fuse(t, W, live, w, cap)
    assert _bits_equal(vol.tsdf.cpu().numpy(), want_t) and _bits_equal(vol.weight.cpu().numpy(), want_w)
    _assert_fusion_record(_host_record(rec), want_rec)
    assert not np.any(rec.cpu().numpy()[4:])
    return t, want_t


def test_fusion_finish_pass_takes_a_second_trip(lsf):
    """335 partials on 256 lanes, and no grid-stride: the finish pass alone"""
    shape = (70, 70, 70)
    groups, _, blocks = _fusion_split(shape)
    assert FUSION_BLOCK < blocks == 335 and blocks < FUSION_MAX_BLOCKS and groups <= blocks * FUSION_BLOCK
    _volume_mode(lsf, shape, 0.75, 8.0, 3)


def _assert_fusion_big_crosses():
    groups, tail, blocks = _fusion_split(FUSION_BIG)
    assert blocks == FUSION_MAX_BLOCKS and tail != 0 and groups * 10 >= 11 * FUSION_BLOCK * FUSION_MAX_BLOCKS


def test_fusion_volume_mode_grid_stride(lsf):
    _assert_fusion_big_crosses()
    before, after = _volume_mode(lsf, FUSION_BIG, 0.75, 8.0, 4)
    _assert_second_trip_changes(before, after)


def test_fusion_depth_mode_grid_stride(lsf):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    _assert_fusion_big_crosses()
    d = _depth(np.float32)
    dev, code = gen.device_depth(d)
    t, W = _random_model(FUSION_BIG, np.random.default_rng(7))
    a_t, a_w = _device(t, W)
    rec = device_fusion.integrate_depth(a_t, a_w, dev, code, _camera(K_SYN), FUSION_BIG_OFF, FUSION_TWIST, w=0.5,
                                        max_weight=6.0)
    want_t, want_w, want_rec = F.fuse_depth(t, W, d, K_SYN, 0.001, FUSION_BIG_OFF, FUSION_TWIST, 20, 0.004, 0.5, 6.0)
    _assert_second_trip_changes(t, want_t)
    assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
    _assert_fusion_record(_host_record(rec), want_rec)


@functools.lru_cache(maxsize=None)
def _weighted_case():
    """the weighted call at FUSION_BIG, restated once: (depth, model tsdf, model weight, pixel weights, new tsdf, new
    weight, record); nothing modifies them"""
    d = _depth(np.uint16)
    rng = np.random.default_rng(11)
    pw = _random_weights(d.shape, rng)
    t, W = _random_model(FUSION_BIG, rng)
    args = (d, K_SYN, 0.001)
    want = FW.fuse_depth_weighted(t, W, *args, FUSION_BIG_OFF, FUSION_TWIST, 20, 0.004, 0.5, 6.0, pw, True)
    _assert_second_trip_changes(t, want[0])
    # the planes that lie wholly past the cap, restated on their own: carved and weight-rejected voxels are among them
    z = -(-FUSION_CAP // (FUSION_BIG[1] * FUSION_BIG[2]))
    assert z < FUSION_BIG[0]
    tail_t, _, tail = FW.fuse_depth_weighted(t[z:], W[z:], *args, FUSION_BIG_OFF + [0, 0, z], FUSION_TWIST, 20, 0.004,
                                             0.5, 6.0, pw, True)
    assert _bits_equal(tail_t, want[0][z:])
    assert tail["carved"] > 100 and tail["weight_rejected"] > 100 and tail["fused"] > 1000
    return (d, t, W, pw) + tuple(want)


def _weighted_call(tsdf, weight, d, pw):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    dev, code = gen.device_depth(d)
    return device_fusion.integrate_depth_weighted(tsdf, weight, dev, code, _camera(K_SYN), FUSION_BIG_OFF, FUSION_TWIST,
                                                  w=0.5, max_weight=6.0, pixel_weight=_device(pw)[0], carve=True)


def test_fusion_weighted_mode_grid_stride(lsf):
    _assert_fusion_big_crosses()
    d, t, W, pw, want_t, want_w, want = _weighted_case()
    a_t, a_w = _device(t, W)
    rec = _weighted_call(a_t, a_w, d, pw)
    assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
    _assert_weighted_record(_unpack(rec), want)
    assert not rec.cpu().numpy()[6:].any()


def test_fusion_weighted_mode_grid_stride_unaligned(lsf):
    """the scalar accesses of buffers off 16-byte alignment, over the same walk"""
    _assert_fusion_big_crosses()
    d, t, W, pw, want_t, want_w, want = _weighted_case()
    n = t.size
    big = torch.empty(2 * n + 8, dtype=torch.float32, device="cuda")
    o = n + 2 + ((n + 2) % 4 == 0)  # the second view starts past the first, on no multiple of 4 floats
    tv, wv = big[1:n + 1].view(FUSION_BIG), big[o:o + n].view(FUSION_BIG)
    assert tv.data_ptr() % 16 and wv.data_ptr() % 16
    tv.copy_(torch.from_numpy(t)), wv.copy_(torch.from_numpy(W))
    rec = _weighted_call(tv, wv, d, pw)
    assert _bits_equal(tv.cpu().numpy(), want_t) and _bits_equal(wv.cpu().numpy(), want_w)
    _assert_weighted_record(_unpack(rec), want)


# ----------------------------------------------------------------------------------------- 4. mesh: the scan's carry
MESH_TILE, MESH_SCAN_THREADS = 2048, 1024  # LSF_MESH_TILE (include/lsf_hip.h), kScanThreads (csrc/lsf_mesh.hip)


def _scan_passes(shape):
    """scan_kernel of csrc/lsf_mesh.hip: `for (base = 0; base < blocks; base += kScanThreads)` over one count per
    tile, with `running` carried from pass to pass"""
    tiles = -(-int(np.prod(shape)) // MESH_TILE)
    return -(-tiles // MESH_SCAN_THREADS)


def _owned_from_plane(t, w, z, min_weight=0.0):
    """(vertices, faces) of the cells from plane z on: a lower bound of what voxels of those planes own (they also own
    the vertices that only a cell of plane z - 1 draws)"""
    v, f, _ = M.extract(t[z:], w[z:], [0, 0, 0], 1.0, 0.0, min_weight)
    return len(v), len(f)


def test_mesh_scan_carries_into_a_second_pass(lsf):
    shape = (144, 128, 128)
    assert _scan_passes(shape) == 2
    z, y, x = np.meshgrid(*(np.arange(v, dtype=np.float64) for v in shape), indexing="ij")
    d = np.sqrt(((z - 71.3) / 1.1) ** 2 + (y - 63.6) ** 2 + (x - 64.2) ** 2) - 58.3
    t = np.clip(d / 3, -1, 1).astype(np.float32)
    w = np.ones_like(t)
    first = -(-MESH_SCAN_THREADS * MESH_TILE // (shape[1] * shape[2]))  # the first plane wholly in the second pass
    assert first == 128
    owned_v, owned_f = _owned_from_plane(t, w, first)
    assert owned_v >= 1000 and owned_f >= 1000
    verts, faces, _ = _check_mesh(lsf, t, w, [0, 0, 0], 1.0, min_faces=100000)
    assert M.is_closed_manifold(faces) and M.euler_characteristic(len(verts), faces) == 2


def test_mesh_scan_carries_into_a_third_pass(lsf):
    """a wavy sheet that climbs through the last planes, with unusable voxels"""
    shape = (132, 180, 180)
    assert _scan_passes(shape) == 3
    z, y, x = np.meshgrid(*(np.arange(v, dtype=np.float64) for v in shape), indexing="ij")
    d = z - (112.4 + 24.0 * np.sin(x * 0.05) * np.cos(y * 0.04))
    t = np.clip(d / 4, -1, 1).astype(np.float32)
    w = np.random.default_rng(7).uniform(0.0, 3.0, shape).astype(np.float32)
    w[w < 0.02] = 0.0
    w[120, 90, :] = np.nan
    t[125, 40:60, 100] = np.nan
    plane = shape[1] * shape[2]
    second, third = (-(-k * MESH_SCAN_THREADS * MESH_TILE // plane) for k in (1, 2))
    assert third < shape[0] - 1
    assert min(_owned_from_plane(t, w, second, 0.05)) >= 1000 and min(_owned_from_plane(t, w, third, 0.05)) >= 1000
    _check_mesh(lsf, t, w, [-90.0, -90.5, 100.25], 0.004, min_weight=0.05, min_faces=10000)


# ---------------------------------------------------------------------------------------------------- 5. term leaves
@pytest.mark.parametrize("shape,slope", [((726, 726), 0.0025), ((81, 81, 81), 0.02)])
def test_terms_match_the_oracle_past_the_cap(lsf, shape, slope):
    """LSF_SELECT_ALL and LSF_SELECT_BAND of test_gpu_term_leaves.test_terms_match_the_oracle, its assertions and
    tolerances, just past 2048 x 256 voxels; the slope keeps band voxels in the second trip"""
    assert TERM_CAP < int(np.prod(shape)) < 1.02 * TERM_CAP
    assert_terms_match_the_oracle(lsf, shape, slope)


@pytest.mark.parametrize("shape,slope", [((726, 726), 0.0025), ((81, 81, 81), 0.02)])
def test_listed_terms_match_the_oracle_past_the_cap(lsf, shape, slope):
    """LSF_SELECT_LIST with 600000 entries, repeats and out-of-range entries among them, on both sides of the cap: entry
    k of every output is the oracle's whole-field answer at voxel indices[k], bit for bit (the oracle's terms are
    whole-array numpy, so every entry is compared), and zero for an index outside the field"""
    from oracle import lsf_oracle as O
    from levelsetfusion_python_amd import _lib as L
    from levelsetfusion_python_amd import device_core, device_terms
    d, n, count = len(shape), int(np.prod(shape)), 600000
    assert count > TERM_CAP
    live, canonical, warp = term_fields(shape, slope)
    rng = np.random.default_rng(13)
    idx = rng.integers(0, n, count).astype(np.int32)
    idx[TERM_CAP - 1:TERM_CAP + 2] = [n - 1, 0, n // 2]
    outside = np.zeros(count, bool)
    outside[[5, TERM_CAP + 5, count - 1]] = True
    idx[outside] = [-1, n, 2 ** 31 - 1]
    at = np.where(outside, 0, idx)
    grads = O.gradient(live)
    kg, ke = O.killing_gradient(warp, 0.1)
    lg, le = O.level_set_gradient(live)
    dg, diff = O.data_term_gradient(live, canonical, O.BASIC)
    fg, fdiff = O.data_term_gradient(live, canonical, O.THRESHOLDED_FDM)
    cases = [(L.TERM_DATA_BASIC, dg, (np.float32(0.5) * (diff * diff)).astype(np.float32)),
             (L.TERM_DATA_THRESHOLDED_FDM, fg, (np.float32(0.5) * (fdiff * fdiff)).astype(np.float32)),
             (L.TERM_TIKHONOV, O.tikhonov_gradient(warp), O.tikhonov_energy_direct(warp)),
             (L.TERM_KILLING, kg, ke), (L.TERM_LEVEL_SET, lg, le)]
    live_t, canonical_t, warp_t = (device_terms._device(a) for a in (live, canonical, warp))
    grads_t = [device_terms._device(g) for g in grads]
    idx_t = torch.from_numpy(idx).cuda()
    for term, want_g, want_e in cases:
        g = torch.full((count, d), float("nan"), dtype=torch.float32, device="cuda")
        e = torch.full((count,), float("nan"), dtype=torch.float64, device="cuda")
        total = torch.zeros(1, dtype=torch.float64, device="cuda")
        device_terms.term_gradient(term, device_core.make_grid(shape), live_t, canonical_t, grads_t, warp_t, g, e, total,
                                   selection=L.SELECT_LIST, indices=idx_t, isomorphic_enforcement_factor=0.1)
        want_g = np.where(outside[:, None], np.float32(0), want_g.reshape(n, d)[at])
        want_e = np.where(outside, np.float32(0), want_e.reshape(n)[at])
        assert np.any(want_g[TERM_CAP:]) and np.any(want_e[TERM_CAP:])
        assert maxdiff(g, want_g) == 0.0 and maxdiff(e, want_e) == 0.0, term
        assert rel(float(total.item()), float(want_e.astype(np.float64).sum())) < 1e-9, term


# ------------------------------------------------------------------------------------------- 6. the halo copy kernel
HALO_CAP = 512 * 256  # the grid's x extent and kBlock, lsf_halo_copy in csrc/lsf_fields.hip


def test_halo_copy_past_its_grid(lsf):
    """pack and unpack of halo_copy_kernel, `i += gridDim.x * kBlock` over the halo * ny * nx floats of a channel,
    against tensor slicing, exactly"""
    from levelsetfusion_python_amd import device as dev
    nz, ny, nx, h = 9, 210, 211, 3
    assert HALO_CAP < h * ny * nx < 1.02 * HALO_CAP
    g = torch.Generator("cuda").manual_seed(7)
    live = torch.randn((nz, ny, nx), device="cuda", generator=g)
    warp = torch.randn((3, nz, ny, nx), device="cuda", generator=g)
    lo = torch.full((4, h, ny, nx), float("nan"), device="cuda")
    hi = torch.full_like(lo, float("nan"))
    z_lo, z_hi = 1, nz - 1 - h
    dev.halo_copy(live, warp, lo, hi, h, z_lo, z_hi, unpack=False)
    assert torch.equal(lo, torch.cat([live[z_lo:z_lo + h][None], warp[:, z_lo:z_lo + h]]))
    assert torch.equal(hi, torch.cat([live[z_hi:z_hi + h][None], warp[:, z_hi:z_hi + h]]))
    live2, warp2 = live.clone(), warp.clone()
    dev.halo_copy(live2, warp2, hi, lo, h, 0, nz - h, unpack=True)  # swapped messages into the end slices
    assert torch.equal(live2[:h], hi[0]) and torch.equal(warp2[:, :h], hi[1:])
    assert torch.equal(live2[nz - h:], lo[0]) and torch.equal(warp2[:, nz - h:], lo[1:])
    assert torch.equal(live2[h:nz - h], live[h:nz - h]) and torch.equal(warp2[:, h:nz - h], warp[:, h:nz - h])


# ------------------------------------------------------------------------------------- 7. relocaliser: the pixel loop
# The inputs of sections 7 to 12, the constants that mirror csrc/lsf_relocaliser.hip and the assertions that a shape
# crosses its cap with a visible effect past it are tests/test_relocaliser_host.py's, where they run without a card.

def _colour_image(shape, with_colour, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,)).astype(np.uint8) if with_colour else None


@pytest.mark.parametrize("with_colour", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.float64])
@pytest.mark.parametrize("shape, coarse_shape", RH.PIXEL_LOOP_IMAGES)
def test_reloc_encode_pixel_loop(lsf, shape, coarse_shape, dtype, with_colour):
    """`for (p = lane; p < pixels; p += kWave)` of reloc_encode_kernel: blocks of 306 to 342 pixels (five or six trips,
    the last one ragged; two workgroups, the second with two idle waves) and the header's 640 x 480 over 30 x 40 (four
    whole trips), with one block whose counting pixels all lie at p >= 64 and one that counts in its last trip only"""
    from levelsetfusion_python_amd import device_relocaliser as D
    depth, ratio = RH.pixel_loop_image(shape, coarse_shape, dtype)
    colour = _colour_image(shape, with_colour, 5)
    want, want_counts, want_record = R.encode(depth, ratio, coarse_shape, (0.5, 3.5), colour)
    RH.check_pixel_loop_image(shape, coarse_shape, depth, ratio, want, want_counts)
    if with_colour:
        assert want[-1, -1, 1:].all()  # the colour sums of the block that counts past the first trip only
    assert 0 < want_record["valid_blocks"] < want_counts.size
    encode_twice_against(D, depth, ratio, coarse_shape, colour, want, want_counts, want_record)


# ------------------------------------------------------------------------------------- 8. relocaliser: the block loop
@pytest.mark.parametrize("shape, dtype, with_colour", [(RH.BLOCK_LOOP_IMAGES[0], np.float32, True),
                                                       (RH.BLOCK_LOOP_IMAGES[1], np.uint16, False),
                                                       (RH.BLOCK_LOOP_IMAGES[1], np.float64, True)])
def test_reloc_encode_block_loop(lsf, shape, dtype, with_colour):
    """`b += waves` of reloc_encode_kernel, and the record kernel's sums over the blocks past it: 4160 coarse blocks on
    4096 waves, of one pixel each (`2 * count >= pixels` decided by a single pixel) and of 2 or 3 rows by 2 or 3 columns"""
    from levelsetfusion_python_amd import device_relocaliser as D
    depth, ratio = RH.depth_image(shape, RH.BLOCK_LOOP_COARSE, dtype, np.random.default_rng(shape[0]))
    colour = _colour_image(shape, with_colour, 6)
    want, want_counts, want_record = R.encode(depth, ratio, RH.BLOCK_LOOP_COARSE, (0.5, 3.5), colour)
    RH.check_block_loop_image(shape, want, want_counts, want_record)
    encode_twice_against(D, depth, ratio, RH.BLOCK_LOOP_COARSE, colour, want, want_counts, want_record)


# ---------------------------------------------------------------- 9. relocaliser: the distance word loop, the maximum F
@pytest.mark.parametrize("ferns, decisions", [(1030, 8), (RH.RELOC_MAX_FERNS, 1)])
def test_reloc_distance_word_loop(lsf, ferns, decisions):
    """`w += kWave` of reloc_distance_kernel under test_gpu_relocaliser's query comparison: F = 1030 (rows of 64.4 words
    off the alignment, a last word past the array) and F = 4096 (aligned rows of four whole trips, the LDS copy of the
    code full, 16 workgroups of the code kernel), with keyframes that differ from the frame only past the first trip"""
    from levelsetfusion_python_amd import device_relocaliser as D
    coarse, table, rows = RH.query_case(ferns, decisions, False, True)
    RH.check_word_loop_case(ferns, coarse, table, rows)
    query_comparison(D, ferns, decisions, coarse, table, rows)


# -------------------------------------------------------------- 10. relocaliser: the distance row loop, the select loop
@pytest.mark.parametrize("name", list(RH.ROW_LOOP_CASES))
def test_reloc_row_loop_and_selection(lsf, name):
    """`k += waves` of reloc_distance_kernel and `k += kBlock` of reloc_select_kernel over 4101 keyframes of 70 ferns:
    the four nearest spread over the first 256 keys, the later trips of the selection and the rows past 4096, a tie of
    equal codes across 4096 that goes to the lower id, the nearest of all in the last row; a database of `capacity`
    keyframes and of one fewer, harvest at the threshold (an append into row 4100), one below it, and into a full one"""
    from levelsetfusion_python_amd import device_relocaliser as D
    coarse, table, rows = RH.row_loop_case(name)
    capacity = len(rows)
    nearest = RH.check_row_loop_case(name, coarse, table, rows)
    code = R.frame_code(coarse, *table)
    want = _run_query(D, coarse, table, rows, capacity, capacity, candidates=4)
    assert want[2][5] == nearest and (want[1] >= 0).all() and want[2][9] == -1
    n = capacity - 1
    want = _run_query(D, coarse, table, rows, n, capacity, candidates=4)
    fewer = int(want[2][5])  # the nearest of the smaller database
    assert want[1][n] == -1 and (want[1][:n] >= 0).all() and fewer == (2 if name == "far-first" else nearest)
    at = _run_query(D, coarse, table, rows, n, capacity, candidates=4, harvest=True, harvest_differing=fewer)
    assert at[2][9] == n >= RH.RELOC_WAVES and at[4] == capacity and np.array_equal(at[3][n], code)
    below = _run_query(D, coarse, table, rows, n, capacity, candidates=4, harvest=True, harvest_differing=fewer + 1)
    assert below[2][9] == -1 and below[2][10] == 0 and below[4] == n
    full = _run_query(D, coarse, table, rows, capacity, capacity, candidates=4, harvest=True, harvest_differing=nearest)
    assert full[2][9] == -1 and full[2][10] == 1 and full[4] == capacity


# --------------------------------------------------------------------- 11. relocaliser: n_keyframes outside [0, capacity]
@pytest.mark.parametrize("harvest", [False, True])
@pytest.mark.parametrize("outside", [-5, 7])
def test_reloc_size_word_outside_the_database(lsf, outside, harvest):
    """*n_keyframes = -5 and capacity + 7: the kernels read min(max(n, 0), capacity), as R.query does, and write the
    word only when they append (include/lsf_hip.h, lsf_reloc_query) -- -5 with harvest becomes 1, -5 without stays -5,
    capacity + 7 stays and `full` is set for a wanted frame"""
    from levelsetfusion_python_amd import device_relocaliser as D
    coarse, table, rows = RH.query_case(70, 4, True)
    codes = rows[[k for k in range(131) if (k * 7) % 71 >= (23 * 7) % 71]]  # no keyframe equals the frame
    capacity = len(codes)
    n = outside if outside < 0 else capacity + outside
    kw = dict(candidates=4, harvest=harvest, harvest_differing=1)
    want = R.query(coarse, table, codes, n, 4, harvest, 1)
    assert want[2][0] == (0 if n < 0 else capacity) and (want[1] >= 0).all() == (n > 0) and want[1].min() != 0
    for _ in range(2):
        d_codes, d_n = _cuda(codes), torch.tensor([n], dtype=torch.int32, device="cuda")
        got = D.query(_cuda(coarse), *(_cuda(a) for a in table), d_codes, d_n, **kw)
        for a, b in zip(got, want[:3]):
            assert np.array_equal(a.cpu().numpy(), b)
        assert np.array_equal(d_codes.cpu().numpy(), want[3])
        appended = int(want[2][9]) >= 0
        assert appended == (harvest and n < 0) and int(want[2][10]) == (1 if harvest and n > 0 else 0)
        if appended:
            assert int(d_n.item()) == want[4] == 1 and np.array_equal(want[3][0], want[0])
        else:
            assert int(d_n.item()) == n  # not written


# ------------------------------------------------------------------ 12. fusion.Relocaliser with more than 256 keyframes
def test_relocaliser_object_with_many_keyframes(lsf):
    """test_gpu_relocaliser.test_relocaliser_object's comparison with R.Database over 280 synthetic frames that are all
    harvested, and four of them shown again: the select kernel's lanes take a second key, and nearest keyframes lie on
    both sides of key 256.  280 frames of 24 x 32 pixels take about a second, the restated database included."""
    coarse_want, found_want, db = RH.many_keyframes_restated()
    assert db.n == RH.MANY_FRAMES > RH.RELOC_BLOCK
    reloc = lsf.fusion.Relocaliser(**RH.MANY_KEYFRAMES)
    frames = RH.many_frames()
    queries = [(k, True) for k in range(RH.MANY_FRAMES)] + [(k, False) for k in RH.MANY_AGAIN]
    for (k, harvest), want in zip(queries, found_want):
        coarse = reloc.encode(frames[k])
        assert np.array_equal(_relocaliser_bits(coarse), coarse_want[k].view(np.uint32))
        got = reloc.query(coarse, harvest=harvest, twist=np.full(6, k, np.float64) if harvest else None)
        assert {name: got[name] for name in want} == want and not got["full"], k
    assert any(f["nearest"][0] >= RH.RELOC_BLOCK for f in found_want[RH.MANY_FRAMES:])
    codes, twists = reloc.keyframes()
    assert len(codes) == db.n > RH.RELOC_BLOCK and np.array_equal(codes, db.codes[:db.n])
    assert np.array_equal(twists, db.twists) and int(reloc.size.item()) == db.n
    assert all(np.array_equal(a, b) for a, b in zip(reloc.table, db.table))


# --------------------------------------------------------------------------- 13 to 15. the brick store past 8192 bricks
# The window, its shifts, the constants that mirror csrc/lsf_volume_bricks.hip and the assertions of the crossing are
# tests/test_volume_bricks_host.py's.

@pytest.mark.parametrize("with_colour", [False, True])
def test_bricks_count_and_gather_past_the_cap(lsf, with_colour):
    """`b += stride` of bricks_flag_kernel and bricks_gather_kernel and the second trip of bricks_scan_kernel (the carry;
    whole threads, a partial one and idle ones after a whole trip) on a 65 x 65 x 2 grid of 8450 bricks: flagged and
    touched-but-unflagged bricks past index 8192, and under the shift that makes everything leave more than 8192 rows"""
    want = BH.big_window_counts()
    assert want[BH.BIG_ALL_SHIFT][2] > BH.BRICKS_WAVES and want[BH.BIG_Y_SHIFT][0][BH.BRICKS_WAVES:].sum() >= 100
    rows, touched_unflagged = count_and_gather_against_restatement(BH.BIG_SHAPE, (BH.BIG_ORIGIN,), BH.BIG_SHIFTS,
                                                                   with_colour)
    assert rows == sum(v[2] for v in want.values()) and touched_unflagged > 0


@pytest.mark.parametrize("with_colour", [False, True])
def test_bricks_scatter_past_the_cap(lsf, with_colour):
    """`k += stride` of bricks_scatter_kernel over 8452 rows: every brick of the big window's grid and two outside it,
    shuffled, random validity bytes; tests/test_volume_bricks_host.py asserts that the rows from 8192 on change more
    than 1000 words under the last two shifts"""
    bricks = BH.big_window_bricks(with_colour)
    assert len(bricks[0]) > BH.BRICKS_WAVES
    dev_bricks = tuple(None if a is None else torch.from_numpy(np.array(a)).cuda() for a in bricks)
    scatter_against_restatement(bricks, dev_bricks, BH.BIG_SHAPE, BH.BIG_ORIGIN, BH.BIG_SHIFTS, with_colour)
    for dev, host in zip(dev_bricks[1:3], bricks[1:3]):
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), host.view(np.uint32))  # read only


@pytest.mark.parametrize("shift", [BH.BIG_SHIFTS[2], (0, BH.BIG_SHAPE[1] + 5, 0)])
def test_bricks_round_trip_past_the_cap(lsf, shift):
    """test_gpu_volume_bricks.test_round_trip's body on the big window at its lattice origin: a partial shift that takes
    the whole first z layer out, and one that empties the window (more than 8192 rows out, and scattered back)"""
    want = BH.big_window_counts()
    leaving = B.count(BH.inputs(BH.BIG_SHAPE)[1], BH.BIG_ORIGIN, shift)
    assert leaving[0].size > BH.BRICKS_WAVES and leaving[0][BH.BRICKS_WAVES:].sum() > 0
    if shift[1] > BH.BIG_SHAPE[1]:
        assert leaving[2] == want[BH.BIG_ALL_SHIFT][2] > BH.BRICKS_WAVES  # everything leaves either way
    vol, store, _ = round_trip(lsf, BH.BIG_SHAPE, shift, BH.BIG_ORIGIN)
    assert len(store) == 0 and store.last["bricks_in"] == leaving[2]
