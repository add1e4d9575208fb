"""Fields, a plain numpy marching cubes and mesh invariants for the dense extractor (csrc/nslam_mesh.hip:
nslam_mc_count / nslam_mc_emit, ops.marching_cubes) and for mesh cleaning, shared by tests/test_mc_cases_cpu.py
and tests/test_gpu_mc_cases.py.  Everything is procedural: nothing is stored, and no kernel code is read.

The contract is DESIGN.md §7f: corner c of a cell sits at offset (c & 1, c >> 1 & 1, c >> 2 & 1); bit c of the
case is set when the value there is below the level (value < level: a value at the level is not below it); a
lattice point owns its +x, +y, +z edges; one vertex per owned edge with (a < level) != (b < level), at
origin + (i + t)·spacing with t = (level - a) / (b - a) in float32 and the position in float64; vertices in
owner-edge order, faces in cell order.  A cell's triangles are the loops of tools/gen_mc_table.py, each fanned
from its valid vertex with the lowest edge id (`refan`), in the table's winding.

The invariants at the end read no table: they see a mesh and, for the volume bracket, the field.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gen():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(REPO, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_ROWS = None


def rows():
    """gen_mc_table.build_table()'s rows (derived once)."""
    global _ROWS
    if _ROWS is None:
        _ROWS = gen().build_table()[0]
    return _ROWS


# ------------------------------------------------------------------------------------------------
# the fan rule
# ------------------------------------------------------------------------------------------------
def edge_faces(e):
    """The two faces (axis, side) of the cell that edge e = axis * 4 + (a + 2 b) lies in."""
    ax, a, b = e >> 2, e & 1, (e >> 1) & 1
    o1, o2 = [x for x in range(3) if x != ax]
    return {(o1, a), (o2, b)}


def row_loops(row):
    """The loops behind a table row, which holds a fan per loop from the loop's first vertex."""
    loops = []
    for t in row:
        if loops and loops[-1][0] == t[0] and loops[-1][-1] == t[1]:
            loops[-1].append(t[2])
        else:
            loops.append(list(t))
    return loops


def valid_apices(loop):
    """Positions c of the loop from which no fan diagonal lies in a face of the cell: loop[c] shares no face
    with loop[c + 2] .. loop[c + n - 2]."""
    n = len(loop)
    return [c for c in range(n)
            if not any(edge_faces(loop[c]) & edge_faces(loop[(c + d) % n]) for d in range(2, n - 1))]


def fan(loop, apex):
    n = len(loop)
    return [(loop[apex], loop[(apex + i) % n], loop[(apex + i + 1) % n]) for i in range(1, n - 1)]


def refan(row):
    """The row's loops, each fanned from its valid apex with the lowest edge id: same loops, same count, same
    winding, and a choice that does not depend on the direction in which the loop is listed."""
    tris = []
    for loop in row_loops(row):
        tris += fan(loop, min(valid_apices(loop), key=lambda c: loop[c]))
    return tris


def first_valid_fan(row):
    """The earlier rule of the block-volume extractor: the first valid apex in loop order."""
    tris = []
    for loop in row_loops(row):
        tris += fan(loop, valid_apices(loop)[0])
    return tris


def table_fan(row):
    """The table's own fans (every loop from its first vertex)."""
    return list(row)


# ------------------------------------------------------------------------------------------------
# fields
# ------------------------------------------------------------------------------------------------
CASE_SHAPE = (4, 4, 1024)


def case_volume():
    """float32 4 x 4 x 1024, +1 everywhere; case c lives in the block z in [4c, 4c + 4): corner k of the cell at
    (1, 1, 4c + 1) is -1 when bit k of c is set.  Every case's cell is surrounded by above-level values."""
    vol = np.ones(CASE_SHAPE, dtype=np.float32)
    for c in range(256):
        for k in range(8):
            if (c >> k) & 1:
                vol[1 + (k & 1), 1 + ((k >> 1) & 1), 4 * c + 1 + ((k >> 2) & 1)] = -1.0
    return vol


def case_cells():
    """Low corners [256,3] of the case volume's centre cells."""
    return np.array([(1, 1, 4 * c + 1) for c in range(256)])


def random_field(shape, seed):
    """Uniform values in (-0.5, 0.5) inside a one-voxel shell of -1.  An axis of length 2 (a single layer of
    cells) has no room for a shell and an interior: it gets none, and the surface is open along it.
    → float32 [shape]"""
    rng = np.random.default_rng(seed)
    vol = np.full(shape, -1.0, dtype=np.float32)
    inner = tuple(slice(1, -1) if n > 2 else slice(None) for n in shape)
    vol[inner] = (rng.random(vol[inner].shape) - 0.5).astype(np.float32)
    return vol


def is_closed_shape(shape):
    """Does random_field(shape) / plateau_field(shape) carry its shell on every axis?"""
    return all(n > 2 for n in shape)


def plateau_field(shape, seed):
    """A smooth field (two blobs, values within about +-3) over which two independent random voxel masks write
    -100 and +100, the way Mesher.get_mesh writes `unseen` and `~inside`: plateaus side by side on voxel-jagged
    masks.  A one-voxel shell of -100 closes the surface.  → float32 [shape]"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    s = np.asarray(shape, dtype=np.float64)
    f = np.full(shape, -np.inf)
    for ctr, r in (((0.38, 0.45, 0.42), 0.30), ((0.70, 0.55, 0.66), 0.22)):
        d2 = sum((g[a] - ctr[a] * (s[a] - 1)) ** 2 for a in range(3))
        f = np.maximum(f, r * s.min() - np.sqrt(d2))
    vol = f.astype(np.float32)
    unseen = rng.random(shape) < 0.18
    outside = rng.random(shape) < 0.18
    vol[unseen] = -100.0
    vol[outside] = 100.0
    shell = np.ones(shape, bool)
    shell[tuple(slice(1, -1) if n > 2 else slice(None) for n in shape)] = False
    vol[shell] = -100.0
    return vol


def with_level_hits(vol, level, seed, frac=0.05):
    """The field with about `frac` of the values inside its shell set to the level itself."""
    rng = np.random.default_rng(seed)
    out = vol.copy()
    inner = tuple(slice(1, -1) if n > 2 else slice(None) for n in vol.shape)
    hit = rng.random(out[inner].shape) < frac
    out[inner][hit] = np.float32(level)
    return out


def strip_mesh(n, seed):
    """One triangle strip of n faces over n + 2 vertices whose ids are permuted among n + 5, three isolated
    vertices, and one more face that repeats a vertex (a zero-area face hanging on the strip).
    → dict(vertices float64 [n + 5, 3], faces int32 [n + 1, 3], strip: the strip's vertex ids, isolated: the
    three others)"""
    rng = np.random.default_rng(seed)
    nv = n + 5
    perm = rng.permutation(nv)
    strip, isolated = perm[:n + 2], perm[n + 2:]
    pos = np.zeros((nv, 3))
    i = np.arange(n + 2)
    pos[strip] = np.stack([0.5 * i, (i & 1) * 1.0, 0.1 * np.sin(0.01 * i)], 1)
    pos[isolated] = rng.random((3, 3)) + 10.0
    tri = np.stack([i[:n], i[:n] + 1, i[:n] + 2], 1)
    tri[1::2] = tri[1::2][:, [0, 2, 1]]                     # a strip alternates its winding
    faces = strip[tri]
    extra = np.array([[strip[n // 2], strip[n // 2], strip[n // 2 + 1]]])
    faces = np.concatenate([faces, extra], 0).astype(np.int32)
    return {"vertices": pos, "faces": np.ascontiguousarray(faces), "strip": np.sort(strip),
            "isolated": np.sort(isolated)}


# the fields of tests/test_gpu_mc_cases.py: name → (maker, seed).  (12, 10, 14) with seed 3 is the field of
# test_marching_cubes_random_field_is_closed_and_deterministic; (2, 3, 257) and (17, 2, 5) are single layers of
# cells (open along that axis), the first with a z line longer than a 256-thread workgroup; (3, 3, 3) has one
# free value; none of the four point counts is a multiple of 256.
RANDOM_SHAPES = {"random_12x10x14": ((12, 10, 14), 3), "random_2x3x257": ((2, 3, 257), 4),
                 "random_17x2x5": ((17, 2, 5), 5), "random_3x3x3": ((3, 3, 3), 9)}
PLATEAU = ((16, 16, 16), 7)
PAIR_FIELD = ((32, 32, 16), 11)           # the field both extractors get (section B)
ORIGIN = (0.5, -1.0, 2.0)
SPACING = (0.1, 0.15, 0.2)
# variant → (level, origin, spacing, level hits)
VARIANTS = {"plain": (0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False),
            "placed": (0.25, ORIGIN, SPACING, False),
            "hits": (0.25, ORIGIN, SPACING, True)}


def gpu_fields():
    """name → (float32 volume, closed).  closed = +1: a below-level shell surrounds the field, its surface is
    closed and encloses the values at or above the level (positive signed volume); -1: the shell is above the
    level (the case volume), the closed surface encloses the values below it and the signed volume is negative;
    0: a single layer of cells, open along that axis."""
    out = {"cases": (case_volume(), -1)}
    for name, (shape, seed) in RANDOM_SHAPES.items():
        out[name] = (random_field(shape, seed), 1 if is_closed_shape(shape) else 0)
    out["plateau_16x16x16"] = (plateau_field(*PLATEAU), 1)
    return out


def variant_of(vol, variant, seed=99):
    """(volume, level, origin, spacing) of a field under a variant."""
    level, origin, spacing, hits = VARIANTS[variant]
    return (with_level_hits(vol, level, seed) if hits else vol), level, origin, spacing


# ------------------------------------------------------------------------------------------------
# the reference extractor
# ------------------------------------------------------------------------------------------------
def cell_cases(vol, level):
    """Case index of every cell, [nx - 1, ny - 1, nz - 1] int64 (empty when an axis has length 1)."""
    nx, ny, nz = vol.shape
    below = vol < np.float32(level)
    case = np.zeros((max(nx - 1, 0), max(ny - 1, 0), max(nz - 1, 0)), np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        case |= below[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << k
    return case


def has_four_crossing_face(vol, level):
    """Is there a cell face whose diagonal corners agree and whose neighbours differ (four crossings)?"""
    below = vol < np.float32(level)
    for ax in range(3):
        u, v = [a for a in range(3) if a != ax]
        b = np.moveaxis(below, (u, v), (0, 1))
        c00, c10, c01, c11 = b[:-1, :-1], b[1:, :-1], b[:-1, 1:], b[1:, 1:]
        # a face counts only when a cell holds it: the third axis needs two layers
        if below.shape[ax] > 1 and ((c00 == c11) & (c10 == c01) & (c00 != c10)).any():
            return True
    return False


def reference_mc(vol, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), fan_rule=refan):
    """Marching cubes of a float32 volume → (vertices float64 [V,3], faces int32 [F,3]) as the contract orders
    them.  A volume with an axis of length 1 holds no cell: the empty mesh."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    if min(vol.shape) < 2:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    lv = np.float32(level)
    below = vol < lv
    n = vol.size
    flags = np.zeros((nx, ny, nz, 3), bool)
    tt = np.zeros((nx, ny, nz, 3), np.float32)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        a, b = vol[lo], vol[hi]
        cross = below[lo] != below[hi]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (lv - a) / (b - a)                           # float32 throughout
        flags[lo + (ax,)] = cross
        tt[lo + (ax,)] = np.where(cross, t, np.float32(0))
    flat = flags.reshape(n * 3)
    vert_id = (np.cumsum(flat) - flat).reshape(nx, ny, nz, 3)
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in vol.shape], indexing="ij"), -1)
    o, sp = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    pos = np.repeat(idx[..., None, :], 3, axis=3)            # [nx,ny,nz,axis,xyz]
    for ax in range(3):
        pos[..., ax, ax] += tt[..., ax].astype(np.float64)
    verts = (o + pos * sp).reshape(n * 3, 3)[flat]

    table = [fan_rule(r) for r in rows()]
    width = max(len(r) for r in table)
    ntri = np.array([len(r) for r in table])
    tri = np.full((256, width, 3), -1, np.int64)
    for c, r in enumerate(table):
        if r:
            tri[c, :len(r)] = np.asarray(r)
    case = cell_cases(vol, level)
    cells = np.argwhere(np.ones_like(case, bool))            # C order = the order of the low corners' points
    cs = case.reshape(-1)
    nt = ntri[cs]
    off = np.cumsum(nt) - nt
    faces = np.zeros((int(nt.sum()), 3), np.int32)
    for t in range(width):
        sel = np.flatnonzero(nt > t)
        if sel.size == 0:
            break
        for k in range(3):
            e = tri[cs[sel], t, k]
            ax, ea, eb = e >> 2, e & 1, (e >> 1) & 1
            offx = np.where(ax == 0, 0, ea)
            offy = np.where(ax == 0, ea, np.where(ax == 1, 0, eb))
            offz = np.where(ax == 2, 0, eb)
            g = cells[sel]
            faces[off[sel] + t, k] = vert_id[g[:, 0] + offx, g[:, 1] + offy, g[:, 2] + offz, ax]
    return verts, faces


# ------------------------------------------------------------------------------------------------
# invariants that read no table
# ------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def directed_edge_stats(faces, n_verts):
    """→ dict(doubled: directed edges used more than once, unmatched: directed edges whose reverse occurs a
    different number of times, same_triple: pairs of faces on the same three vertices)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return {"doubled": 0, "unmatched": 0, "same_triple": 0}
    d = directed_edges(f)
    key, cnt = np.unique(d[:, 0] * n_verts + d[:, 1], return_counts=True)
    fwd = dict(zip(key.tolist(), cnt.tolist()))
    unmatched = sum(1 for k, c in fwd.items() if fwd.get((k % n_verts) * n_verts + k // n_verts, 0) != c)
    s = np.sort(f, 1)
    _, tc = np.unique((s[:, 0] * n_verts + s[:, 1]) * n_verts + s[:, 2], return_counts=True)
    return {"doubled": int((cnt > 1).sum()), "unmatched": unmatched, "same_triple": int((tc * (tc - 1) // 2).sum())}


def components(faces, n_verts):
    """Union-find over the faces → label int64 [V]: the lowest vertex id of each vertex's component."""
    parent = np.arange(n_verts, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        ra, rb, rc = find(a), find(b), find(c)
        m = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = m
    return np.array([find(v) for v in range(n_verts)], dtype=np.int64)


def euler_by_component(faces, n_verts):
    """{label: V - E + F} over the components that have faces."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = components(f, n_verts)
    d = np.sort(directed_edges(f), 1)
    und = np.unique(d[:, 0] * n_verts + d[:, 1]) // n_verts   # one low end per undirected edge
    used = np.unique(f)
    out = {}
    for lab, cnt in zip(*np.unique(label[used], return_counts=True)):
        out[int(lab)] = int(cnt)
    for lab, cnt in zip(*np.unique(label[und], return_counts=True)):
        out[int(lab)] -= int(cnt)
    for lab, cnt in zip(*np.unique(label[f[:, 0]], return_counts=True)):
        out[int(lab)] += int(cnt)
    return out


def face_areas(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)


def signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def volume_bracket(vol, level, spacing):
    """(lower, upper): the cells whose corners are all / any at or above the level, times the cell volume.  The
    surface of a closed field cuts only mixed cells, so its signed volume lies between the two."""
    case = cell_cases(vol, level)
    cell = float(np.prod(np.asarray(spacing, dtype=np.float64)))
    return float((case == 0).sum()) * cell, float((case != 255).sum()) * cell


def canon_rows(f):
    """Faces rotated to start at their lowest vertex and sorted: equal sets of oriented triangles compare equal."""
    f = np.asarray(f).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    k = np.argmin(f, 1)
    i = np.arange(f.shape[0])
    r = np.stack([f[i, k], f[i, (k + 1) % 3], f[i, (k + 2) % 3]], 1)
    return r[np.lexsort(r.T[::-1])]
