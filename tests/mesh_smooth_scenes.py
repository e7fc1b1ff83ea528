"""The meshes the mesh-smoothing tests share (tests/test_mesh_smooth_host.py, tests/test_gpu_mesh_smooth.py) besides
those of mesh_components_scenes: the test sphere clean and noisy, its open half, and the sphere far from the origin at a
small voxel size.  Host numpy only."""
import functools

import numpy as np

import mesh_restatement as M

CENTRE, RADIUS, BAND, NOISE = (11.5, 12.25, 11.75), 6.3, 3.0, 0.35


def sphere_volume(noisy=False, n=24):
    """the test sphere's TSDF; with noisy, NOISE * default_rng(0).standard_normal added to the distance before the clip"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    d = np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2) - RADIUS
    if noisy:
        d = d + NOISE * np.random.default_rng(0).standard_normal(d.shape)
    return np.clip(d / BAND, -1, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_mesh(noisy=False):
    """(vertices, faces, normals) at voxel size 1: 742 vertices and 1480 faces clean, 934 and 1864 noisy; both closed"""
    t = sphere_volume(noisy)
    return M.extract(t, np.ones_like(t), [0, 0, 0], 1.0, normals=True)


@functools.lru_cache(maxsize=None)
def half_sphere_mesh():
    """the clean sphere's [:, :, :12]: 371 vertices, 688 faces, an open border of 52 edges"""
    t = sphere_volume()[:, :, :12]
    return M.extract(t, np.ones_like(t), [0, 0, 0], 1.0, normals=True)


@functools.lru_cache(maxsize=None)
def far_mesh():
    """the noisy sphere 2 m from the origin on every axis at 4 mm voxels: a large B against small edges"""
    t = sphere_volume(True)
    return M.extract(t, np.ones_like(t), [500, 500, 500], 0.004, normals=True)


def radius_std(vertices, centre=CENTRE):
    return float(np.linalg.norm(vertices.astype(np.float64) - np.asarray(centre, np.float64), axis=1).std())


def volume(vertices, faces):
    """the signed volume the faces enclose, in float64"""
    p = vertices.astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
