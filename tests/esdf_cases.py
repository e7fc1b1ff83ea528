"""Models for the tests of the Euclidean distance field, shared by the CPU and the GPU suite: the random model, the
48^3 sphere model fused on the host from the restatements, its analytic distance, and the fixed inputs -- ties, the cap,
degenerate models, unknown="occupied", sites on the faces, min_weight and iso.  Host numpy only: no package import."""
import functools

import numpy as np

import fusion_scene as S
import fusion_weighted_restatement as FW

VOXEL = 0.004
SPHERE_N, SPHERE_BAND, SPHERE_FRAMES = 48, 20, 3


def random_model(shape, seed, observed=0.5):
    """weights zero with probability 1 - observed (else one), tsdf uniform in (-1, 1)"""
    rng = np.random.default_rng(seed)
    weight = (rng.random(shape) < observed).astype(np.float32)
    tsdf = rng.uniform(-1, 1, shape).astype(np.float32)
    return tsdf, weight


def flat(shape, z, y, x):
    return (z * shape[1] + y) * shape[2] + x


def empty(shape):
    return np.ones(shape, np.float32), np.zeros(shape, np.float32)


def with_pairs(shape, pairs):
    """an empty model with, per ((z, y, x), (z, y, x)) pair of neighbours, the first voxel observed inside (tsdf -1)
    and the second observed outside (tsdf +1): both are sites, and nothing else is"""
    tsdf, weight = empty(shape)
    for a, b in pairs:
        assert sum(abs(i - j) for i, j in zip(a, b)) == 1
        tsdf[a], weight[a] = -1.0, 1.0
        tsdf[b], weight[b] = 1.0, 1.0
    return tsdf, weight


# ties: (shape, pairs, the voxel asked about, its distance2, the sites that tie for it); the answer is the smallest flat
TIES = {
    "two along x": ((2, 3, 11), [((0, 0, 2), (1, 0, 2)), ((0, 0, 8), (1, 0, 8))], (0, 0, 5), 9,
                    [(0, 0, 2), (0, 0, 8)]),
    "two along y": ((2, 11, 3), [((0, 2, 0), (1, 2, 0)), ((0, 8, 0), (1, 8, 0))], (0, 5, 0), 9,
                    [(0, 2, 0), (0, 8, 0)]),
    "two along z": ((11, 2, 3), [((2, 0, 0), (2, 1, 0)), ((8, 0, 0), (8, 1, 0))], (5, 0, 0), 9,
                    [(2, 0, 0), (8, 0, 0)]),
    "four in a plane": ((2, 11, 11), [((0, 2, 5), (1, 2, 5)), ((0, 8, 5), (1, 8, 5)), ((0, 5, 2), (1, 5, 2)),
                                      ((0, 5, 8), (1, 5, 8))], (0, 5, 5), 9,
                        [(0, 2, 5), (0, 8, 5), (0, 5, 2), (0, 5, 8)]),
    "four in the plane above": ((2, 11, 11), [((0, 2, 5), (1, 2, 5)), ((0, 8, 5), (1, 8, 5)), ((0, 5, 2), (1, 5, 2)),
                                              ((0, 5, 8), (1, 5, 8))], (1, 5, 5), 9,
                                [(1, 2, 5), (1, 8, 5), (1, 5, 2), (1, 5, 8)]),
}

# the cap: one pair of sites at (0, 0, 0) (inside) and (1, 0, 0), R = 5.  Per voxel of the plane z = 0 the expected
# distance2, None for the sentinel: 25 = R^2 on an axis and as 3-4-5 is kept; 26 = R^2 + 1 is not, though each offset of
# the site is <= R; neither is 32 = 4^2 + 4^2.
CAP_SHAPE, CAP_PAIRS, CAP_R = (2, 8, 12), [((0, 0, 0), (1, 0, 0))], 5
CAP_EXPECTED = {(0, 0, 5): 25, (0, 0, 6): None, (0, 3, 4): 25, (0, 4, 3): 25, (0, 1, 5): None, (0, 5, 1): None,
                (0, 4, 4): None, (0, 5, 0): 25, (0, 6, 0): None, (1, 0, 5): 25, (1, 3, 4): 25, (1, 1, 5): None}


def one_unobserved():
    """a 4^3 model observed free everywhere but at (1, 1, 1)"""
    tsdf, weight = np.ones((4, 4, 4), np.float32), np.ones((4, 4, 4), np.float32)
    weight[1, 1, 1] = 0.0
    return tsdf, weight


def faces_model():
    """(5, 6, 7), observed everywhere, free but for one inside voxel at the centre of each of the six faces"""
    shape = (5, 6, 7)
    tsdf, weight = np.ones(shape, np.float32), np.ones(shape, np.float32)
    for v in ((0, 3, 3), (4, 3, 3), (2, 0, 3), (2, 5, 3), (2, 3, 0), (2, 3, 6)):
        tsdf[v] = -0.5
    return tsdf, weight


def fixed_cases():
    """{name: (tsdf, weight, keywords of the transform)}: what the CPU suite asserts properties of and the GPU suite
    compares exactly"""
    cases = {"tie " + name: with_pairs(shape, pairs) + (dict(max_distance_voxels=6),)
             for name, (shape, pairs, _, _, _) in TIES.items()}
    cases["cap"] = with_pairs(CAP_SHAPE, CAP_PAIRS) + (dict(max_distance_voxels=CAP_R),)
    cases["empty"] = empty((6, 5, 9)) + (dict(max_distance_voxels=7),)
    single = empty((6, 5, 9))
    single[0][2, 2, 4], single[1][2, 2, 4] = -1.0, 1.0
    cases["a single observed voxel"] = single + (dict(max_distance_voxels=7),)
    cases["occupied, one unobserved voxel"] = one_unobserved() + (dict(max_distance_voxels=3, unknown="occupied"),)
    cases["free, one unobserved voxel"] = one_unobserved() + (dict(max_distance_voxels=3),)
    cases["occupied, random"] = random_model((7, 9, 12), 21) + (dict(max_distance_voxels=4, unknown="occupied"),)
    cases["six faces"] = faces_model() + (dict(max_distance_voxels=4),)
    tsdf, weight = random_model((8, 9, 10), 22)
    cases["min_weight 1 over weights 1 and 2"] = (tsdf, weight + 1, dict(max_distance_voxels=5, min_weight=1.0))
    tsdf, weight = random_model((8, 9, 10), 23, observed=0.8)
    cases["iso 0.25"] = (tsdf, weight, dict(max_distance_voxels=5, iso=0.25))
    return cases


@functools.lru_cache(maxsize=None)
def sphere_model():
    """(tsdf, weight) of the 48^3 sphere scene: three frames fused at their true poses with carve=True, band 20, 4 mm
    voxels, by the host restatement of the weighted rule; read only"""
    shape = (SPHERE_N,) * 3
    tsdf, weight = empty(shape)
    off = S.offset(SPHERE_N)
    for k in range(SPHERE_FRAMES):
        tsdf, weight, _ = FW.fuse_depth_weighted(tsdf, weight, S.render(S.true_twist(k)), S.K, 1.0, off, S.true_twist(k),
                                                 SPHERE_BAND, VOXEL, carve=True)
    tsdf.setflags(write=False)
    weight.setflags(write=False)
    return tsdf, weight


def sphere_analytic_distance():
    """(48, 48, 48) float64, metres: the signed distance of each voxel centre to the nearest of the scene's three
    spheres and its back plane, positive in free space"""
    n, off = SPHERE_N, S.offset(SPHERE_N)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    px, py, pz = (x + off[0]) * VOXEL, (y + off[1]) * VOXEL, (z + off[2]) * VOXEL
    d = S.PLANE_Z - pz
    for c, r in S.SPHERES:
        d = np.minimum(d, np.sqrt((px - c[0]) ** 2 + (py - c[1]) ** 2 + (pz - c[2]) ** 2) - r)
    return d
