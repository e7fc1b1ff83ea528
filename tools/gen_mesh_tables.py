"""Generates csrc/lsf_mesh_tables.h, the marching-cubes case table of mesh extraction ("Mesh
extraction").  The table is derived, not pasted: `python tools/gen_mesh_tables.py` rewrites the header, and
tests/test_mesh_host.py checks that the committed header is what this script writes.

Corner c = x + 2y + 4z of a cell.  Edges, axis-major: 0-3 the x-edges from corners 0, 2, 4, 6; 4-7 the y-edges from
corners 0, 1, 4, 5; 8-11 the z-edges from corners 0, 1, 2, 3.  A corner is inside when its bit of the case is set.

1. On each cube face, walk its 4 corners counter-clockwise as seen from outside.  A crossing face-edge is entering
   when the walk goes from an outside corner to an inside one, leaving otherwise; each entering crossing is joined to
   the next leaving crossing in walk order.  On a face with 4 crossings this cuts off each inside corner on its own.
2. Every crossing cube-edge then has one successor; following successors gives cycles, listed by their lowest edge.
3. Each cycle is a fan from its apex: the lowest-numbered edge of the cycle such that no fan diagonal joins two edges
   on a common cube face.
4. Triangles (apex, c[i], c[i+1]), oriented so that their right-hand normal points towards larger values (outside)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "levelsetfusion-python_amd", "csrc", "lsf_mesh_tables.h")
MAX_TRIANGLES = 5

CORNERS = [np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1]) for c in range(8)]
# (lower corner, axis) of each edge
EDGE_LOW = [0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3]
EDGE_AXIS = [0] * 4 + [1] * 4 + [2] * 4
EDGE_HIGH = [c + (1 << a) for c, a in zip(EDGE_LOW, EDGE_AXIS)]


def edge_of(c0, c1):
    lo, hi = min(c0, c1), max(c0, c1)
    for e in range(12):
        if EDGE_LOW[e] == lo and EDGE_HIGH[e] == hi:
            return e
    raise ValueError("corners %d, %d are not joined by an edge" % (c0, c1))


def faces():
    """the 6 cube faces as corner walks, counter-clockwise seen from outside"""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            u, v = [a for a in range(3) if a != axis]
            # a cycle around the square in the (u, v) plane
            square = [(0, 0), (1, 0), (1, 1), (0, 1)]
            walk = [next(c for c in cs if CORNERS[c][u] == p and CORNERS[c][v] == q) for p, q in square]
            p = [CORNERS[c].astype(float) for c in walk]
            normal = np.cross(p[1] - p[0], p[2] - p[1])
            outward = np.zeros(3)
            outward[axis] = 1.0 if side else -1.0
            if normal @ outward < 0:
                walk = walk[::-1]
            out.append(walk)
    return out


FACES = faces()
EDGE_FACES = [frozenset(f for f, walk in enumerate(FACES) if EDGE_LOW[e] in walk and EDGE_HIGH[e] in walk)
              for e in range(12)]


def share_face(e0, e1):
    return bool(EDGE_FACES[e0] & EDGE_FACES[e1])


def cycles(case):
    inside = [(case >> c) & 1 == 1 for c in range(8)]
    succ = {}
    for walk in FACES:
        crossings = []  # (edge, entering) in walk order
        for i in range(4):
            a, b = walk[i], walk[(i + 1) % 4]
            if inside[a] != inside[b]:
                crossings.append((edge_of(a, b), inside[b]))
        for i, (e, entering) in enumerate(crossings):
            if not entering:
                continue
            for j in range(1, len(crossings)):
                f, f_entering = crossings[(i + j) % len(crossings)]
                if not f_entering:
                    assert e not in succ
                    succ[e] = f
                    break
    out, seen = [], set()
    for e in sorted(succ):
        if e in seen:
            continue
        cyc = [e]
        seen.add(e)
        while succ[cyc[-1]] != e:
            cyc.append(succ[cyc[-1]])
            seen.add(cyc[-1])
        out.append(cyc)
    return out


def fan(cycle):
    """the cycle rotated to start at its apex"""
    for apex in sorted(cycle):
        i = cycle.index(apex)
        c = cycle[i:] + cycle[:i]
        if not any(share_face(c[0], c[k]) for k in range(2, len(c) - 1)):
            return c
    raise ValueError("no apex for cycle %s" % (cycle,))


def _midpoint(e):
    return (CORNERS[EDGE_LOW[e]] + CORNERS[EDGE_HIGH[e]]) / 2.0


def _successor_order_points_inwards():
    """whether the successor order's right-hand normal points to the inside; decided on case 1 (corner 0 inside)"""
    (c,) = cycles(1)
    p = [_midpoint(e) for e in c]
    normal = np.cross(p[1] - p[0], p[2] - p[0])
    return normal @ (CORNERS[0] - p[0]) > 0


REVERSE = _successor_order_points_inwards()


def triangles(case):
    """the case's triangles as edge triples, in table order"""
    out = []
    for cyc in cycles(case):
        if REVERSE:
            cyc = [cyc[0]] + cyc[1:][::-1]
        c = fan(cyc)
        out += [(c[0], c[i], c[i + 1]) for i in range(1, len(c) - 1)]
    return out


def tables():
    """(count uint8 (256,), edges uint8 (256, 3 * MAX_TRIANGLES), unused entries 0)"""
    count = np.zeros(256, np.uint8)
    edges = np.zeros((256, 3 * MAX_TRIANGLES), np.uint8)
    for case in range(256):
        tris = triangles(case)
        assert len(tris) <= MAX_TRIANGLES, (case, tris)
        count[case] = len(tris)
        edges[case, :3 * len(tris)] = np.array(tris, np.uint8).reshape(-1)
    return count, edges


def header_text():
    count, edges = tables()
    lines = ["// Generated by tools/gen_mesh_tables.py: do not edit.  The marching-cubes case table of mesh extraction",
             "// (INTEGRATION.md section 3, \"Mesh extraction\"): corner c = x + 2y + 4z, bit c of the case set when "
             "corner",
             "// c is inside; edges 0-3 the x-edges from corners 0, 2, 4, 6, 4-7 the y-edges from corners 0, 1, 4, 5, "
             "8-11",
             "// the z-edges from corners 0, 1, 2, 3.",
             "#pragma once",
             "",
             "#define LSF_MESH_MAX_TRIANGLES %d" % MAX_TRIANGLES,
             "",
             "// the lower corner of each edge; its axis is edge / 4",
             "static constexpr unsigned char kMeshEdgeLow[12] = {%s};" % ", ".join(str(c) for c in EDGE_LOW),
             "",
             "// triangles of each case",
             "static constexpr unsigned char kMeshTriangleCount[256] = {"]
    for row in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(v)) for v in count[row:row + 32]) + ",")
    lines += ["};", "",
              "// each case's triangles as edge triples (apex, c[i], c[i + 1]), %d triples, unused entries 0"
              % MAX_TRIANGLES,
              "static constexpr unsigned char kMeshTriangleEdges[256][%d] = {" % (3 * MAX_TRIANGLES)]
    for case in range(256):
        lines.append("    {" + ", ".join(str(int(v)) for v in edges[case]) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else HEADER
    with open(path, "w") as f:
        f.write(header_text())
    print(path)
