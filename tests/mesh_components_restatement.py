"""numpy restatement of mesh components ("Mesh components").  The HIP kernels
(csrc/lsf_mesh_components.hip) must equal components() and filter() exactly: the labels, the table, the order of both
output arrays, the bit patterns of positions, normals and colours, and the whole record.  Labels are found by label
propagation with pointer jumping, every step vectorised; nothing here depends on an order of evaluation, since every
step takes minima.  Host numpy only: no package import.  Test infrastructure, not a CPU path of the package."""
import numpy as np

__all__ = ["RECORD_FIELDS", "TABLE_FIELDS", "labels", "components", "keep_rows", "filter"]

RECORD_FIELDS = ("vertices_in", "faces_in", "invalid_vertices", "invalid_faces", "components", "step_cap",
                 "components_kept", "vertices_out", "faces_out")
TABLE_FIELDS = ("labels", "vertex_counts", "face_counts", "bounds")


def labels(vertex_count, faces):
    """int64 (V,): per vertex the smallest vertex index of its component.  faces int (F, 3), every index in [0, V)"""
    lab = np.arange(vertex_count, dtype=np.int64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(f):
        return lab
    u = np.concatenate([f[:, 0], f[:, 0]])
    w = np.concatenate([f[:, 1], f[:, 2]])
    while True:
        lu, lw = lab[u], lab[w]
        if np.array_equal(lu, lw):
            return lab
        low = np.minimum(lu, lw)
        np.minimum.at(lab, lu, low)  # the larger label's own vertex moves under the smaller
        np.minimum.at(lab, lw, low)
        while True:  # pointer jumping, to the fixed point: every vertex at a vertex that is its own label
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def _checked(vertices, faces):
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    bad_v = int((~np.isfinite(v).all(axis=1)).sum())
    bad_f = int((~((f >= 0) & (f < len(v))).all(axis=1)).sum())
    if bad_v:
        raise ValueError("%d vertices with a non-finite coordinate" % bad_v)
    if bad_f:
        raise ValueError("%d faces with an index outside [0, %d)" % (bad_f, len(v)))
    return v, f


def components(vertices, faces):
    """(vertex_labels int32 (V,), face_labels int32 (F,), table): table a dict of labels, vertex_counts, face_counts
    int32 (C,) and bounds float32 (C, 2, 3), the components in ascending label order.  Raises ValueError on a non-finite
    vertex or a face index outside [0, V)."""
    v, f = _checked(vertices, faces)
    V = len(v)
    lab = labels(V, f)
    face_lab = lab[f[:, 0].astype(np.int64)] if len(f) else np.zeros(0, np.int64)
    roots = np.nonzero(lab == np.arange(V))[0]
    row = np.full(V, -1, np.int64)
    row[roots] = np.arange(len(roots))
    vertex_counts = np.bincount(row[lab], minlength=len(roots))
    face_counts = np.bincount(row[face_lab], minlength=len(roots))
    bits = v.view(np.uint32).copy()
    bits[bits == 0x80000000] = 0  # -0 read as +0
    pos = bits.view(np.float32)
    bounds = np.empty((len(roots), 2, 3), np.float32)
    bounds[:, 0] = np.inf
    bounds[:, 1] = -np.inf
    np.minimum.at(bounds[:, 0], row[lab], pos)
    np.maximum.at(bounds[:, 1], row[lab], pos)
    table = dict(labels=roots.astype(np.int32), vertex_counts=vertex_counts.astype(np.int32),
                 face_counts=face_counts.astype(np.int32), bounds=bounds)
    return lab.astype(np.int32), face_lab.astype(np.int32), table


def keep_rows(table, min_faces=None, min_vertices=None, min_extent=None, keep_largest=None):
    """bool (C,): the rows of the table that stay.  A row passes when it meets every threshold given; with keep_largest
    = k the first k passing rows stay, in the order face count descending, label ascending."""
    if min_faces is None and min_vertices is None and min_extent is None and keep_largest is None:
        raise ValueError("no criterion")
    passing = np.ones(len(table["labels"]), bool)
    if min_faces is not None:
        passing &= table["face_counts"] >= min_faces
    if min_vertices is not None:
        passing &= table["vertex_counts"] >= min_vertices
    if min_extent is not None:
        b = table["bounds"].astype(np.float64)
        edge = (b[:, 1] - b[:, 0]).max(axis=1) if len(b) else np.zeros(0)
        passing &= edge >= float(min_extent)
    if keep_largest is not None:
        rows = np.nonzero(passing)[0]
        order = rows[np.lexsort((table["labels"][rows], -table["face_counts"][rows].astype(np.int64)))]
        passing = np.zeros_like(passing)
        passing[order[:keep_largest]] = True
    return passing


def filter(vertices, faces, normals=None, colours=None, min_faces=None, min_vertices=None, min_extent=None,
           keep_largest=None):
    """(vertices float32 (V', 3), faces int32 (F', 3), normals or None, colours or None, record dict of RECORD_FIELDS):
    the mesh without the components the criteria reject, kept vertices and faces in input order, faces re-indexed."""
    v, f = _checked(vertices, faces)
    vertex_lab, face_lab, table = components(v, f)
    keep = keep_rows(table, min_faces, min_vertices, min_extent, keep_largest)
    row = np.full(len(v), -1, np.int64)
    row[table["labels"]] = np.arange(len(keep))
    keep_v = keep[row[vertex_lab]] if len(v) else np.zeros(0, bool)
    keep_f = keep[row[face_lab]] if len(f) else np.zeros(0, bool)
    new = np.cumsum(keep_v) - 1
    out_f = new[f[keep_f].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    record = dict(vertices_in=len(v), faces_in=len(f), invalid_vertices=0, invalid_faces=0,
                  components=len(keep), step_cap=0, components_kept=int(keep.sum()), vertices_out=int(keep_v.sum()),
                  faces_out=int(keep_f.sum()))
    carried = [None if a is None else np.ascontiguousarray(a)[keep_v] for a in (normals, colours)]
    return np.ascontiguousarray(v[keep_v]), out_f, carried[0], carried[1], record
