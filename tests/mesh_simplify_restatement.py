"""numpy restatement of mesh simplification by vertex clustering ("Mesh simplification").  The
HIP kernels (csrc/lsf_mesh_simplify.hip) must equal simplify() exactly: vertex and normal float32 bit patterns, colours,
face indices, the order of both arrays and the whole record.  Every float step below is one float64 IEEE operation in
the order written; every sum is an integer sum, so no result depends on an order of summation.  Host numpy only: no
package import.  Test infrastructure, not a CPU path of the package."""
import numpy as np

__all__ = ["RECORD_FIELDS", "simplify", "vertex_keys"]

RECORD_FIELDS = ("vertices_in", "faces_in", "invalid_vertices", "invalid_faces", "clusters", "degenerate_faces",
                 "face_groups", "cancelled_groups", "multi_cover_groups", "orphan_clusters", "vertices_out",
                 "faces_out", "table_overflow")
Q_ONE = 1 << 24          # quantisation bins of a cell per axis
MAX_CELL = 1 << 20       # |c| beyond this is invalid
NORMAL_ONE = float(1 << 30)
NORMAL_CLAMP = 2.0       # a normal component is clamped to +-2 before it is scaled: unit normals never reach it, and
#                          2^31 members of 2^31 each stay inside int64


def vertex_keys(vertices, cell_size=None, origin=(0.0, 0.0, 0.0)):
    """(valid (V,) bool, key (V, 3) int64, q (V, 3) int64): the key is the three bit patterns with -0 read as +0
    (weld) or the lattice cell (cluster); q is the quantised position inside the cell, 0 in weld mode"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    valid = np.isfinite(v).all(axis=1)
    if cell_size is None:
        bits = v.view(np.uint32).astype(np.int64)
        bits[bits == 0x80000000] = 0
        return valid, bits, np.zeros_like(bits)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    cell = float(cell_size)
    with np.errstate(over="ignore", invalid="ignore"):
        r = (v.astype(np.float64) - o) / cell
        c = np.floor(r)
        valid &= (np.abs(c) <= MAX_CELL).all(axis=1)  # false for an overflow to inf and for a NaN
        c = np.where(valid[:, None], c, 0.0)
        fq = np.floor((np.where(valid[:, None], r, 0.0) - c) * float(Q_ONE))
    q = np.minimum(fq.astype(np.int64), Q_ONE - 1)
    return valid, c.astype(np.int64), q


def _group(keys):
    """(id (N,), first (G,)): equal rows of keys share an id; ids count the groups by their smallest row index"""
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    return rank[inverse], first[order]


def _sum_by(ids, values, groups):
    out = np.zeros((groups,) + values.shape[1:], np.int64)
    np.add.at(out, ids, values)
    return out


def simplify(vertices, faces, normals=None, colours=None, cell_size=None, origin=(0.0, 0.0, 0.0), details=None):
    """(vertices float32 (V', 3), faces int32 (F', 3), normals float32 (V', 3) or None, colours uint8 (V', 3) or None,
    record dict of RECORD_FIELDS).  cell_size None welds vertices of equal bits; a cell size clusters them.  details: a
    dict that receives group_sizes and net, one entry per face group, for the tests that ask which branches ran."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3).astype(np.int64)
    V, F = len(v), len(f)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    valid, key, q = vertex_keys(v, cell_size, o)
    members = np.nonzero(valid)[0]
    cid_of_member, first_of_cluster = _group(key[members])
    first_of_cluster = members[first_of_cluster] if len(members) else first_of_cluster
    clusters = len(first_of_cluster)
    cid = np.full(V, -1, np.int64)
    cid[members] = cid_of_member
    n = np.bincount(cid_of_member, minlength=clusters).astype(np.int64)
    # representatives
    if cell_size is None:
        pos = v[first_of_cluster]
    else:
        Q = _sum_by(cid_of_member, q[members], clusters)
        c = key[first_of_cluster].astype(np.float64)
        n64 = n.astype(np.float64)[:, None]
        inside = (Q.astype(np.float64) + 0.5 * n64) / (n64 * float(Q_ONE))
        pos = (o + float(cell_size) * (c + inside)).astype(np.float32)
    out_normals = out_colours = None
    if normals is not None:
        nv = np.ascontiguousarray(normals, dtype=np.float32).reshape(V, 3).astype(np.float64)
        nv = np.clip(np.where(np.isfinite(nv), nv, 0.0), -NORMAL_CLAMP, NORMAL_CLAMP)
        m = np.rint(nv * NORMAL_ONE).astype(np.int64)  # ties to even
        S = _sum_by(cid_of_member, m[members], clusters).astype(np.float64)
        L = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        safe = np.where(L != 0.0, L, 1.0)
        out_normals = np.where((L != 0.0)[:, None], S / safe[:, None], 0.0).astype(np.float32)
    if colours is not None:
        cv = np.ascontiguousarray(colours, dtype=np.uint8).reshape(V, 3).astype(np.int64)
        C = _sum_by(cid_of_member, cv[members], clusters)
        out_colours = ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    # faces
    in_range = ((f >= 0) & (f < V)).all(axis=1)
    ids = np.where(in_range[:, None], cid[np.clip(f, 0, V - 1)], -1) if V else np.full((F, 3), -1, np.int64)
    face_ok = in_range & (ids >= 0).all(axis=1)
    degenerate = face_ok & ((ids[:, 0] == ids[:, 1]) | (ids[:, 1] == ids[:, 2]) | (ids[:, 0] == ids[:, 2]))
    live = np.nonzero(face_ok & ~degenerate)[0]
    t = ids[live]
    s = np.sort(t, axis=1)
    lowest = np.argmin(t, axis=1)
    rotated = np.take_along_axis(t, (lowest[:, None] + np.arange(3)) % 3, axis=1)  # the face begun at its smallest id
    sign = np.where((rotated == s).all(axis=1), 1, -1).astype(np.int64)
    gid, _ = _group(s)
    groups = int(gid.max()) + 1 if len(gid) else 0
    net = _sum_by(gid, sign, groups)
    big = np.iinfo(np.int64).max
    first_pos = np.full(groups, big)
    first_neg = np.full(groups, big)
    np.minimum.at(first_pos, gid[sign > 0], live[sign > 0])
    np.minimum.at(first_neg, gid[sign < 0], live[sign < 0])
    if details is not None:
        details.update(group_sizes=np.bincount(gid, minlength=groups), net=net)
    winner = np.where(net > 0, first_pos, np.where(net < 0, first_neg, -1))
    kept = np.sort(winner[winner >= 0])
    kept_ids = cid[f[kept]]
    used = np.zeros(clusters, bool)
    used[kept_ids.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    out_faces = new_id[kept_ids].astype(np.int32).reshape(-1, 3)
    record = dict(vertices_in=V, faces_in=F, invalid_vertices=int(V - len(members)),
                  invalid_faces=int(F - face_ok.sum()), clusters=clusters, degenerate_faces=int(degenerate.sum()),
                  face_groups=groups, cancelled_groups=int((net == 0).sum()),
                  multi_cover_groups=int((np.abs(net) >= 2).sum()), orphan_clusters=int(clusters - used.sum()),
                  vertices_out=int(used.sum()), faces_out=len(kept), table_overflow=0)
    return (np.ascontiguousarray(pos[used]).reshape(-1, 3), out_faces,
            None if out_normals is None else out_normals[used].reshape(-1, 3),
            None if out_colours is None else out_colours[used].reshape(-1, 3), record)
