"""Triangle-mesh files without a mesh library: write_ply() writes the binary little-endian PLY format (float32 x, y, z
and optionally nx, ny, nz, then optionally uchar red, green, blue per vertex; a uchar count and int32 indices per
face), the output of fusion.CanonicalVolume.extract_mesh; read_ply() reads back exactly what write_ply() writes and
refuses anything else -- a coloured file too, unless it is called with colours=True.  Host numpy only."""
import numpy as np

_VERTEX = ("x", "y", "z")
_NORMAL = ("nx", "ny", "nz")
_COLOUR = ("red", "green", "blue")


def _as_host(a, dtype, name):
    if hasattr(a, "detach"):  # a torch tensor, on the host or the GPU
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must have shape (N, 3), got %s" % (name, a.shape))
    return np.ascontiguousarray(a, dtype=dtype)


def _as_colours(a, rows):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError("colours must be uint8, got %s" % a.dtype)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("colours must have shape (N, 3), got %s" % (a.shape,))
    if len(a) != rows:
        raise ValueError("colours has %d rows, vertices %d" % (len(a), rows))
    return np.ascontiguousarray(a)


def write_ply(path, vertices, faces, normals=None, colours=None):
    """write a binary little-endian PLY: vertices (V, 3) and optional normals (V, 3) as float32, optional colours
    (V, 3) uint8 as uchar red, green, blue after them, faces (F, 3) as int32 indices into the vertices"""
    v = _as_host(vertices, np.float32, "vertices")
    f = _as_host(faces, np.int64, "faces")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("faces index vertices outside [0, %d)" % len(v))
    names = _VERTEX
    if normals is not None:
        n = _as_host(normals, np.float32, "normals")
        if len(n) != len(v):
            raise ValueError("normals has %d rows, vertices %d" % (len(n), len(v)))
        v = np.concatenate([v, n], axis=1)
        names = _VERTEX + _NORMAL
    c = None if colours is None else _as_colours(colours, len(v))
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
    header += ["property float %s" % name for name in names]
    if c is not None:
        header += ["property uchar %s" % name for name in _COLOUR]
    header += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    record = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    rows = np.empty(len(f), record)
    rows["n"] = 3
    rows["i"] = f.astype("<i4")
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        if c is None:
            out.write(v.astype("<f4").tobytes())
        else:
            vertex = np.empty(len(v), np.dtype([("f", "<f4", (len(names),)), ("c", "u1", (3,))]))
            vertex["f"], vertex["c"] = v, c
            out.write(vertex.tobytes())
        out.write(rows.tobytes())


def read_ply(path, colours=False):
    """(vertices (V, 3) float32, faces (F, 3) int32, normals (V, 3) float32 or None) of a file write_ply() wrote without
    colours; with colours=True also a file it wrote with them, and a fourth entry: colours (V, 3) uint8 or None"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    lines = data[:end].decode("ascii").split("\n")[:-1]
    body = data[end + len(b"end_header\n"):]
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError("only binary little-endian PLY is read, got %r" % lines[1])
    if not lines[2].startswith("element vertex "):
        raise ValueError("unexpected PLY layout: %r" % lines[2])
    nv = int(lines[2].split()[2])
    names = _VERTEX + _NORMAL if lines[6:7] == ["property float nx"] else _VERTEX
    if lines[3:3 + len(names)] != ["property float %s" % name for name in names]:
        raise ValueError("unexpected vertex properties %s" % (lines[3:],))
    rest = lines[3 + len(names):]
    coloured = bool(colours) and rest[:3] == ["property uchar %s" % name for name in _COLOUR]
    if coloured:
        rest = rest[3:]
    if len(rest) != 2 or not rest[0].startswith("element face ") or \
            rest[1] != "property list uchar int vertex_indices":
        raise ValueError("unexpected PLY layout after the vertex properties: %s" % rest)
    nf = int(rest[0].split()[2])
    vertex = np.dtype([("f", "<f4", (len(names),))] + ([("c", "u1", (3,))] if coloured else []))
    vbytes = nv * vertex.itemsize
    record = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(body) != vbytes + nf * record.itemsize:
        raise ValueError("%s: %d bytes of data, the header promises %d" % (path, len(body),
                                                                           vbytes + nf * record.itemsize))
    table = np.frombuffer(body[:vbytes], vertex)
    v = table["f"].reshape(nv, len(names)).astype(np.float32)
    rows = np.frombuffer(body[vbytes:], record)
    if nf and not np.all(rows["n"] == 3):
        raise ValueError("only triangles are read")
    faces = rows["i"].astype(np.int32).reshape(nf, 3)
    out = v[:, :3].copy(), faces, (v[:, 3:].copy() if len(names) == 6 else None)
    if not colours:
        return out
    return out + (table["c"].reshape(nv, 3).copy() if coloured else None,)
