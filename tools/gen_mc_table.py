#!/usr/bin/env python3
"""Derives the 256-case marching-cubes triangle table and writes nice-slam_amd/csrc/nslam_mc_table.h.

Nothing is copied from a published table: every case is derived from the cube's geometry.

Conventions (shared with csrc/nslam_mesh.hip):
  corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) in (x, y, z);
  bit c of the case index is set when the field at corner c is BELOW the level (value < level);
  edge e = axis * 4 + (a + 2 b) runs along `axis` (0 = x, 1 = y, 2 = z) from the corner whose two other
  offsets are (a, b), taken in ascending axis order: x edges (dy, dz), y edges (dx, dz), z edges (dx, dy).

Derivation of one case:
  1. an edge crosses when its two corners differ in sign;
  2. every face of the cube holds 0, 2 or 4 crossing edges.  Two are joined by a segment.  Four (an
     ambiguous face: the diagonal corners agree) are joined in the two pairs that cut off the face's
     lowest-numbered corner and the corner diagonal to it.  The rule reads only that face's four corner
     signs and is the same seen from the cell on either side, so neighbouring cells agree and the surface
     closes; it is also unchanged when every sign flips;
  3. every segment gets a direction such that the surface normal (right-hand rule around the loop) points
     to the below side: for a face with outward normal n, a segment direction d and an in-face vector b
     toward the below corners, (n x d) . b > 0;
  4. every crossing edge then has one incoming and one outgoing segment: the segments form closed
     directed loops, each of which is fan-triangulated from its first vertex.

The row width is the largest triangle count found.
"""
from __future__ import annotations

import os
import sys

CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]


def corner_id(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def edge_corners(e):
    """The two corner ids of edge e (low end first)."""
    axis, ab = divmod(e, 4)
    a, b = ab & 1, ab >> 1
    others = [ax for ax in range(3) if ax != axis]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = a, b
    lo = corner_id(off)
    off[axis] = 1
    return lo, corner_id(off)


EDGES = [edge_corners(e) for e in range(12)]
EDGE_OF = {frozenset(p): e for e, p in enumerate(EDGES)}


def faces():
    """Six faces: (outward normal, four corner ids in cyclic order)."""
    out = []
    for axis in range(3):
        u, v = [ax for ax in range(3) if ax != axis]
        for side in (0, 1):
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[u], off[v] = side, du, dv
                ring.append(corner_id(off))
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((tuple(n), ring))
    return out


FACES = faces()


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _mid(e):
    p, q = (CORNERS[c] for c in EDGES[e])
    return ((p[0] + q[0]) / 2, (p[1] + q[1]) / 2, (p[2] + q[2]) / 2)


def _mean(cs):
    pts = [CORNERS[c] for c in cs]
    return tuple(sum(p[i] for p in pts) / len(pts) for i in range(3))


def face_segments(case, normal, ring):
    """Directed segments (edge_from, edge_to) of one face for one sign configuration."""
    below = [(case >> c) & 1 for c in ring]
    ring_edges = [EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))] for i in range(4)]
    crossing = [i for i in range(4) if below[i] != below[(i + 1) % 4]]
    if not crossing:
        return []
    pairs = []  # (edge p, edge q, in-face vector toward the below side)
    if len(crossing) == 2:
        lo = [ring[i] for i in range(4) if below[i]]
        hi = [ring[i] for i in range(4) if not below[i]]
        pairs.append((ring_edges[crossing[0]], ring_edges[crossing[1]], _sub(_mean(lo), _mean(hi))))
    else:
        k = ring.index(min(ring))  # cut off the lowest-numbered corner and its diagonal partner
        centre = _mean(ring)
        for i in (k, (k + 2) % 4):
            toward = _sub(CORNERS[ring[i]], centre)
            if not below[i]:
                toward = tuple(-t for t in toward)
            pairs.append((ring_edges[(i - 1) % 4], ring_edges[i], toward))
    out = []
    for p, q, b in pairs:
        d = _sub(_mid(q), _mid(p))
        s = _dot(_cross(normal, d), b)
        assert s != 0
        out.append((p, q) if s > 0 else (q, p))
    return out


def case_loops(case):
    """Closed directed loops of edge ids for one sign configuration."""
    nxt = {}
    for normal, ring in FACES:
        for p, q in face_segments(case, normal, ring):
            assert p not in nxt, (case, p)
            nxt[p] = q
    crossing = [e for e, (a, b) in enumerate(EDGES) if ((case >> a) & 1) != ((case >> b) & 1)]
    assert sorted(nxt) == crossing and sorted(nxt.values()) == crossing, case
    loops, seen = [], set()
    for e in crossing:
        if e in seen:
            continue
        loop, cur = [], e
        while cur not in seen:
            seen.add(cur)
            loop.append(cur)
            cur = nxt[cur]
        assert cur == e, case
        loops.append(loop)
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def build_table():
    """(rows, width): rows[case] = list of triangles (edge-id triples); width = the largest count."""
    rows = [case_triangles(c) for c in range(256)]
    return rows, max(len(r) for r in rows)


def render_header():
    rows, width = build_table()
    out = ["// nslam_mc_table.h: written by tools/gen_mc_table.py; do not edit (regenerate instead).",
           "// Marching-cubes case table: bit c of the case = corner c (offset c&1, c>>1&1, c>>2&1) is below the",
           "// level; edge e = axis*4 + (a + 2b); rows hold edge-id triples, -1 padded.",
           "#pragma once",
           f"#define NSLAM_MC_MAX_TRI {width}",
           "static __device__ const unsigned char kMcNumTri[256] = {"]
    for i in range(0, 256, 32):
        out.append("    " + ", ".join(str(len(r)) for r in rows[i:i + 32]) + ",")
    out.append("};")
    out.append(f"static __device__ const signed char kMcTri[256][{3 * width}] = {{")
    for r in rows:
        flat = [e for t in r for e in t]
        flat += [-1] * (3 * width - len(flat))
        out.append("    {" + ", ".join(str(e) for e in flat) + "},")
    out.append("};")
    return "\n".join(out) + "\n"


def header_path():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(repo, "nice-slam_amd", "csrc", "nslam_mc_table.h")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else header_path()
    with open(path, "w") as f:
        f.write(render_header())
    rows, width = build_table()
    print(f"wrote {path}: 256 cases, up to {width} triangles per cell")


if __name__ == "__main__":
    main()
