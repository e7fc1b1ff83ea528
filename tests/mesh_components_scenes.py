"""The meshes the mesh-components tests share (tests/test_mesh_components_host.py, tests/test_gpu_mesh_components.py):
the floaters scene, the padded-noise mesh, a mesh that strains a union-find, and a strip-and-fan mesh sized to cross
every capped loop.  Host numpy only."""
import functools

import numpy as np

import mesh_restatement as M

NOISE_OFFSET, NOISE_VOXEL = (1.5, -2.0, 0.25), 0.01
FLOATERS = (((11.5, 11.8, 11.3), 6.3), ((3.2, 3.4, 3.1), 1.3), ((20.3, 19.9, 20.2), 1.6), ((20.1, 3.3, 12.2), 0.8))
# what the floaters scene's mesh is: the four components in label order
FLOATERS_LABELS, FLOATERS_VERTICES, FLOATERS_FACES = (0, 34, 360, 782), (34, 738, 10, 48), (64, 1472, 16, 92)


def _sphere(n, centre, radius, band=3.0):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d / band, -1, 1).astype(np.float32)


def _noise(shape, seed):
    t = np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)
    t[0] = t[-1] = 1
    t[:, 0] = t[:, -1] = 1
    t[:, :, 0] = t[:, :, -1] = 1
    return t


def floaters_volume():
    """a sphere and three small blobs around it in a 24^3 volume"""
    t = _sphere(24, *FLOATERS[0])
    for centre, radius in FLOATERS[1:]:
        t = np.minimum(t, _sphere(24, centre, radius))
    return t


@functools.lru_cache(maxsize=None)
def floaters_mesh():
    t = floaters_volume()
    return M.extract(t, np.ones_like(t), [0, 0, 0], 1.0, normals=True)


@functools.lru_cache(maxsize=None)
def noise_mesh(seed=0):
    t = _noise((14, 14, 14), seed)
    return M.extract(t, np.ones_like(t), list(NOISE_OFFSET), NOISE_VOXEL, normals=True)


def colours(count, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (count, 3), dtype=np.uint8)


def merge(meshes):
    """the concatenation, as fusion.merge_meshes makes it, of (V, F, N) meshes"""
    base, out_v, out_f, out_n = 0, [], [], []
    for v, f, n in meshes:
        out_v.append(v)
        out_f.append(f + base)
        out_n.append(n)
        base += len(v)
    return np.concatenate(out_v), np.concatenate(out_f).astype(np.int32), np.concatenate(out_n)


def split_noise():
    """the noise volume cut at x-cell X // 2 into two volumes that share that layer, each meshed on its own: the two
    meshes, and the whole volume's mesh"""
    t = _noise((14, 14, 14), 0)
    k = t.shape[2] // 2
    w = np.ones_like(t)
    low = M.extract(t[:, :, :k + 1], w[:, :, :k + 1], list(NOISE_OFFSET), NOISE_VOXEL, normals=True)
    high = M.extract(t[:, :, k:], w[:, :, k:], [NOISE_OFFSET[0] + k, NOISE_OFFSET[1], NOISE_OFFSET[2]], NOISE_VOXEL,
                     normals=True)
    return low, high, noise_mesh(0)


def strip(count):
    """the faces of a triangle strip over vertices 0 .. count - 1"""
    i = np.arange(count - 2, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], axis=1)


def fan(count):
    """the faces of a fan around vertex 0 with the rim 1 .. count - 1"""
    i = np.arange(1, count - 1, dtype=np.int64)
    return np.stack([np.zeros_like(i), i, i + 1], axis=1)


def _positions(count, seed):
    v = np.random.default_rng(seed).uniform(-4, 4, (count, 3)).astype(np.float32)
    v[::97, 0] = -0.0  # signed zeros among the coordinates
    return v


@functools.lru_cache(maxsize=None)
def adversarial_mesh(strip_vertices=20000, fan_vertices=9000, isolated=3000, degenerate=600, seed=11):
    """(vertices, faces, parts): a strip whose vertex indices are randomly permuted (deep walks), the same strip with
    its indices reversed (the minimum at the far end), a fan around one hub (every lane contends for one root),
    isolated vertices, and degenerate faces that name a vertex twice or three times and still connect what they name.
    The faces are shuffled.  parts: the number of components each part has."""
    rng = np.random.default_rng(seed)
    blocks, base = [], 0
    permuted = rng.permutation(strip_vertices)
    blocks.append(permuted[strip(strip_vertices)])
    base += strip_vertices
    blocks.append(base + (strip_vertices - 1 - strip(strip_vertices)))
    base += strip_vertices
    hub_last = fan(fan_vertices)
    hub_last = np.where(hub_last == 0, fan_vertices - 1, hub_last - 1)  # the hub is the fan's largest index
    blocks.append(base + hub_last)
    base += fan_vertices
    base += isolated
    pairs = base + np.arange(2 * degenerate, dtype=np.int64).reshape(-1, 2)
    twice = np.stack([pairs[:, 0], pairs[:, 0], pairs[:, 1]], axis=1)   # connects its two vertices
    twice[::3] = twice[::3][:, [2, 0, 0]]
    base += 2 * degenerate
    thrice = np.repeat(base + np.arange(degenerate, dtype=np.int64), 3).reshape(-1, 3)  # connects nothing
    base += degenerate
    faces = np.concatenate(blocks + [twice, thrice])
    faces = faces[rng.permutation(len(faces))].astype(np.int32)
    parts = dict(strips=2, fan=1, isolated=isolated, twice=degenerate, thrice=degenerate)
    return _positions(base, seed), faces, parts


@functools.lru_cache(maxsize=None)
def crossing_mesh(reach):
    """(vertices, faces, components): a strip and a fan of reach // 2 + 1 faces each and reach + 1 isolated vertices
    behind them, so that the vertices, the faces and the components each number more than reach"""
    half = reach // 2 + 3
    faces = np.concatenate([strip(half), half + fan(half)]).astype(np.int32)
    count = 2 * half + reach + 1
    return _positions(count, 3), faces, reach + 3
