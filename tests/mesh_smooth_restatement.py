"""numpy restatement of mesh smoothing and of vertex normals from faces ("Mesh smoothing").
The HIP kernels (csrc/lsf_mesh_smooth.hip) must equal smooth() and vertex_normals() exactly: the bit patterns of the
positions and normals and the whole record.  Edges come from np.unique, the neighbour sums and the normals' sums from
np.add.at on int64, so nothing here depends on an order of evaluation.  Host numpy only: no package import.  Test
infrastructure, not a CPU path of the package."""
import numpy as np

__all__ = ["RECORD_FIELDS", "edges", "topology", "quantum", "one_pass", "smooth", "normal_quantum", "vertex_normals"]

RECORD_FIELDS = ("vertices_in", "faces_in", "invalid_vertices", "invalid_faces", "edges", "boundary_edges",
                 "nonmanifold_edges", "pinned_vertices", "isolated_vertices", "max_degree", "table_overflow",
                 "nonfinite_out", "zero_normals")
BOUNDARIES = ("fixed", "free")


def _checked(vertices, faces):
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    bad_v = int((~np.isfinite(v).all(axis=1)).sum())
    bad_f = int(((f < 0) | (f >= len(v))).any(axis=1).sum())
    if bad_v:
        raise ValueError("mesh smoothing refused: %d vertices with a non-finite coordinate" % bad_v)
    if bad_f:
        raise ValueError("mesh smoothing refused: %d faces with an index outside [0, %d)" % (bad_f, len(v)))
    return v, f


def edges(faces):
    """(edges int64 (E, 2) with lo < hi, in ascending order; counts int64 (E,)): every face's corner pairs (0,1), (1,2),
    (2,0), a pair with equal ends skipped, every other pair one more face of the undirected edge"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pairs = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    if not len(pairs):
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    pairs = np.stack([pairs.min(axis=1), pairs.max(axis=1)], axis=1)
    return np.unique(pairs, axis=0, return_counts=True)


def topology(vertex_count, faces, boundary="fixed"):
    """(edges, counts, degree int64 (V,), pinned bool (V,)) of a mesh whose face indices are all in [0, V)"""
    if boundary not in BOUNDARIES:
        raise ValueError("boundary must be 'fixed' or 'free', got %r" % (boundary,))
    e, counts = edges(faces)
    degree = np.zeros(vertex_count, np.int64)
    np.add.at(degree, e[:, 0], 1)
    np.add.at(degree, e[:, 1], 1)
    pinned = np.zeros(vertex_count, bool)
    if boundary == "fixed":
        pinned[e[counts != 2].reshape(-1)] = True
    return e, counts, degree, pinned


def quantum(positions):
    """q of a pass: with B the largest |coordinate| by an integer maximum on the float bits and E the exponent field of
    B's bits, e = max(E, 1) - 126 (B < 2^e, and B >= 2^(e-1) for a normal B) and q = 2^(e-32); 1 when B is 0"""
    bits = np.ascontiguousarray(positions, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    top = int(bits.max()) if bits.size else 0
    if top == 0:
        return 1.0
    return float(np.ldexp(1.0, max(top >> 23, 1) - 126 - 32))


def _quantised(values, q):
    """(int64) rint(double(x) / q), ties to even; a non-finite x gives 0"""
    x = values.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(x / q)
    return np.where(np.isfinite(x), r, 0.0).astype(np.int64)


def one_pass(positions, e, degree, pinned, w):
    """float32 (V, 3): one pass with the weight w over the float32 positions"""
    p = np.ascontiguousarray(positions, dtype=np.float32)
    q = quantum(p)
    quant = _quantised(p, q)
    sums = np.zeros(p.shape, np.int64)
    np.add.at(sums, e[:, 0], quant[e[:, 1]])
    np.add.at(sums, e[:, 1], quant[e[:, 0]])
    moves = ~pinned & (degree > 0)
    p64 = p.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (sums.astype(np.float64) * q) / np.maximum(degree, 1).astype(np.float64)[:, None]
        new = (p64 + np.float64(w) * (m - p64)).astype(np.float32)
    return np.where(moves[:, None], new, p)


def normal_quantum(cross):
    """qn: with M the largest |component| by an integer maximum on the doubles' bits and E the exponent field of M's
    bits, em = max(E, 1) - 1022 (M < 2^em) and qn = 2^(em-32); 1 when M is 0"""
    bits = np.ascontiguousarray(cross, dtype=np.float64).view(np.uint64) & np.uint64(0x7fffffffffffffff)
    top = int(bits.max()) if bits.size else 0
    if top == 0:
        return 1.0
    return float(np.ldexp(1.0, max(top >> 52, 1) - 1022 - 32))


def _normals(v, f):
    """(normals float32 (V, 3), the number of zero normals) of checked arrays"""
    p = v.astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        u, w = b - a, c - a
        cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                          u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        qn = normal_quantum(cross)
        quant = np.where(np.isfinite(cross), np.rint(cross / qn), 0.0).astype(np.int64)
    sums = np.zeros((len(v), 3), np.int64)
    for corner in range(3):
        np.add.at(sums, f[:, corner].astype(np.int64), quant)
    s = sums.astype(np.float64)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    zero = length == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (s / length[:, None]).astype(np.float32)
    n[zero] = 0.0
    return n, int(zero.sum())


def _record(v, f, **fields):
    rec = dict.fromkeys(RECORD_FIELDS, 0)
    rec.update(vertices_in=len(v), faces_in=len(f))
    rec.update(fields)
    return rec


def vertex_normals(vertices, faces, return_record=False):
    """float32 (V, 3): the area-weighted vertex normals of the faces, (0, 0, 0) where the sum has no length"""
    v, f = _checked(vertices, faces)
    n, zero = _normals(v, f)
    return (n, _record(v, f, zero_normals=zero)) if return_record else n


def smooth(vertices, faces, normals=None, colours=None, iterations=10, lam=0.5, mu=-0.53, boundary="fixed",
           recompute_normals=True):
    """(vertices, faces, normals or None, colours or None, record): iterations of a lam pass and, when mu is not 0, a
    mu pass; faces and colours as they came, normals rebuilt from the smoothed faces when the mesh has them and
    recompute_normals is set, else as they came"""
    v, f = _checked(vertices, faces)
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= iterations <= 1000:
        raise ValueError("iterations must be a whole number in 0 .. 1000, got %r" % (iterations,))
    if not (np.isfinite(lam) and 0 < lam <= 1):
        raise ValueError("lam must be finite and in (0, 1], got %r" % (lam,))
    if not (np.isfinite(mu) and mu <= 0):
        raise ValueError("mu must be finite and <= 0, got %r" % (mu,))
    e, counts, degree, pinned = topology(len(v), f, boundary)
    p = v
    for _ in range(int(iterations)):
        p = one_pass(p, e, degree, pinned, lam)
        if mu != 0:
            p = one_pass(p, e, degree, pinned, mu)
    rec = _record(v, f, edges=len(e), boundary_edges=int((counts == 1).sum()),
                  nonmanifold_edges=int((counts > 2).sum()), pinned_vertices=int(pinned.sum()),
                  isolated_vertices=int((degree == 0).sum()), max_degree=int(degree.max()) if len(v) else 0,
                  nonfinite_out=int((~np.isfinite(p)).sum()) if iterations else 0)
    if normals is not None and recompute_normals:
        normals, rec["zero_normals"] = _normals(p, f)
    return p.copy(), f, normals, colours, rec
