"""fusion_scene's three spheres and back plane painted in four flat colours: the registered uint8 colour image of a frame,
and which surface every pixel sees.  The hit surface is recomputed here with fusion_scene's own expressions (the depth it
gives equals fusion_scene.render's bit for bit; tests/test_colour_host.py asserts it).  Also the scene check that the
CPU and the GPU tests share: the restated four-frame model at 64^3, and which mesh vertices must carry exactly one
surface's colour.  Host numpy only."""
import functools

import numpy as np

import colour_restatement as C
import fusion_restatement as F
import fusion_scene as S
import mesh_restatement as M
import rigid_restatement as R

PLANE = 3  # surface ids: 0..2 the spheres in fusion_scene.SPHERES' order, 3 the plane, -1 nothing
COLOURS = np.array([[220, 40, 30], [30, 200, 60], [40, 70, 230], [240, 210, 90]], np.uint8)
BACKGROUND = np.array([7, 7, 7], np.uint8)
N, FRAMES, COLOUR_BAND, VOXEL = 64, 4, 0.25, 0.004
EXCLUDED_CAP = 0.20  # the margins may exclude at most this fraction of the vertices


def offset():
    """the array offset (voxels) of the N^3 volume: fusion_scene.offset(N) moved by (32, 16, 0) voxels.  Centred on the
    spheres, 44 % of the vertices lie within the margins of a silhouette (a sphere of 5 cm keeps under half of its seen
    cap, and the spheres' outlines cross the plane behind them); this placement holds the +x halves of the first and the
    third sphere and 0.256 m of the plane, of which the spheres hide less, and the margins exclude 18 %"""
    return S.offset(N) + np.array([32.0, 16.0, 0.0])


def render(twist, width=S.WIDTH, height=S.HEIGHT, K_=S.K):
    """(depth float32 (H, W) in metres, colour uint8 (H, W, 3), surface int8 (H, W)) of the scene seen from a camera at
    twist; depth 0, BACKGROUND and -1 where nothing is hit"""
    m = R.matrix3d(np.asarray(twist, dtype=np.float64))
    rot, t = m[:3, :3], m[:3, 3]
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    d = np.stack([(u - float(K_[0, 2])) / float(K_[0, 0]), (v - float(K_[1, 2])) / float(K_[1, 1]),
                  np.ones_like(u)], axis=-1)
    best = np.full(u.shape, np.inf)
    surface = np.full(u.shape, -1, np.int8)
    normal = rot @ np.array([0.0, 0.0, 1.0])
    p0 = rot @ np.array([0.0, 0.0, S.PLANE_Z]) + t
    denom = d @ normal
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(np.abs(denom) > 1e-12, (p0 @ normal) / denom, np.inf)
    nearer = (s > 0) & (s < best)
    best, surface = np.where(nearer, s, best), np.where(nearer, np.int8(PLANE), surface)
    for k, (c, r) in enumerate(S.SPHERES):
        cc = rot @ np.asarray(c) + t
        a = np.sum(d * d, axis=-1)
        b = d @ cc
        disc = b * b - a * (cc @ cc - r * r)
        with np.errstate(invalid="ignore"):
            s = (b - np.sqrt(disc)) / a
        nearer = (disc >= 0) & (s > 0) & (s < best)
        best, surface = np.where(nearer, s, best), np.where(nearer, np.int8(k), surface)
    hit = np.isfinite(best)
    surface = np.where(hit, surface, np.int8(-1))
    image = np.where(hit[..., None], COLOURS[np.maximum(surface, 0)], BACKGROUND).astype(np.uint8)
    return np.where(hit, best, 0.0).astype(np.float32), np.ascontiguousarray(image), surface


@functools.lru_cache(maxsize=None)
def frames():
    """FRAMES x (depth, colour image, surface ids) at the true twists; nothing modifies them"""
    out = tuple(render(S.true_twist(k)) for k in range(FRAMES))
    for f in out:
        for a in f:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_model():
    """(tsdf, weight, colour, records) of the FRAMES frames fused at their true twists into the empty N^3 volume with
    COLOUR_BAND, and the model's mesh with its colours: (vertices, faces, normals, colours) -- all by the restatements"""
    off = offset()
    t, w = F.empty_model((N,) * 3)
    c = np.zeros((N,) * 3 + (4,), np.float32)
    records = []
    for k, (depth, image, _) in enumerate(frames()):
        t, w, c, rec = C.fuse_depth_colour(t, w, c, depth, image, S.K, 1.0, off, S.true_twist(k),
                                           colour_band=COLOUR_BAND)
        records.append(rec)
    verts, faces, normals = M.extract(t, w, off, VOXEL, normals=True)
    colours = C.vertex_colours(t, w, c)
    for a in (t, w, c, verts, faces, normals, colours):
        a.setflags(write=False)
    return t, w, c, records, (verts, faces, normals, colours)


def surface_distances(points):
    """(P, 4): the distance of each world point to the three spheres and the plane"""
    points = np.asarray(points, np.float64)
    d = [np.abs(np.linalg.norm(points - np.asarray(c), axis=1) - r) for c, r in S.SPHERES]
    d.append(np.abs(points[:, 2] - S.PLANE_Z))
    return np.stack(d, axis=1)


def _uniform_within(surface, u, v, radius, want):
    """per point: every pixel within `radius` pixels (a square window, which holds the disc) of (u, v) lies in the image
    and sees surface `want`"""
    h, w = surface.shape
    ok = np.zeros(u.shape, bool)
    for n in range(u.size):
        r = int(np.ceil(radius[n]))
        x, y = int(np.floor(u[n] + 0.5)), int(np.floor(v[n] + 0.5))
        if x - r < 0 or y - r < 0 or x + r >= w or y + r >= h:
            continue
        ok[n] = np.all(surface[y - r:y + r + 1, x - r:x + r + 1] == want[n])
    return ok


def qualifying(vertices):
    """(mask, surface id) per vertex.  A vertex qualifies when it is within one voxel of exactly one surface and, in every
    frame, farther than the margin from every other surface and from that surface's silhouette -- the border of the
    pixels that see it, the image border included -- measured at the vertex's depth.  The margin is two voxels plus one
    pixel's footprint at the vertex's depth in that frame, z / fx."""
    vertices = np.asarray(vertices, np.float64)
    dist = surface_distances(vertices)
    near = dist <= VOXEL
    one = near.sum(axis=1) == 1
    sid = np.argmax(near, axis=1)
    others = np.where(np.arange(4)[None, :] == sid[:, None], np.inf, dist).min(axis=1)
    fx, fy, cx, cy = float(S.K[0, 0]), float(S.K[1, 1]), float(S.K[0, 2]), float(S.K[1, 2])
    ok = one.copy()
    for k, (_, _, surface) in enumerate(frames()):
        m = R.matrix3d(np.asarray(S.true_twist(k), dtype=np.float64))
        p = vertices @ m[:3, :3].T + m[:3, 3]
        z = p[:, 2]
        ok &= z > 0
        zs = np.where(z > 0, z, 1.0)
        footprint = zs / min(fx, fy)
        margin = 2 * VOXEL + footprint
        ok &= others > margin
        u, v = fx * p[:, 0] / zs + cx, fy * p[:, 1] / zs + cy
        idx = np.nonzero(ok)[0]
        ok[idx] = _uniform_within(surface, u[idx], v[idx], margin[idx] / footprint[idx], sid[idx])
    return ok, sid
