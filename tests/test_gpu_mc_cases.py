"""GPU tests of the two marching-cubes extractors and of mesh cleaning on fields that hold every one of the 256
cases, ambiguous faces included (tests/mc_cases.py; its inputs and reference are checked in
tests/test_mc_cases_cpu.py).

A  ops.marching_cubes (nslam_mc_count / nslam_mc_emit) against the plain numpy reference, bit for bit, and
   against invariants that read no table;
B  ops.marching_cubes against ops.tsdf_marching_cubes on one field;
C  ops.tsdf_marching_cubes on a hand-built pool against tsdf_cases.extract_ref;
D  ops.mesh_components / mesh_keep_components on many components and on a long strip;
E  volumes that hold no cell.

Values of +-inf and NaN stay unpinned: what the extractors make of them is not part of the contract (the
mesher writes +-100 for unseen and outside points, which the plateau field covers)."""
import numpy as np
import pytest

import mc_cases as mc
import tsdf_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLEAN = {"doubled": 0, "unmatched": 0, "same_triple": 0}


def _mc(pkg, vol, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    import torch
    v, f = pkg.ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level, origin, spacing)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


@pytest.fixture(scope="module")
def fields():
    return mc.gpu_fields()


# ------------------------------------------------------------------------------------------------
# A: the dense extractor against the reference
# ------------------------------------------------------------------------------------------------
FIELD_NAMES = ["cases"] + list(mc.RANDOM_SHAPES) + ["plateau_16x16x16"]


@pytest.mark.parametrize("variant", list(mc.VARIANTS))
@pytest.mark.parametrize("name", FIELD_NAMES)
def test_dense_extractor_matches_the_reference(pkg, fields, name, variant):
    """Vertices byte for byte, faces entry for entry.  On the closed fields every directed edge occurs once and
    its reverse once, no two faces use the same three vertices, and the signed volume lies between the cells
    wholly and partly on the enclosed side (positive where the shell is below the level; the case volume's
    shell is above it, so there the enclosed side is the below side and the volume is negative).  Without
    level hits, the negated field at the negated level gives the same vertices and every face flipped."""
    base, closed = fields[name]
    vol, level, origin, spacing = mc.variant_of(base, variant)
    want_v, want_f = mc.reference_mc(vol, level, origin, spacing)
    v, f = _mc(pkg, vol, level, origin, spacing)
    st = mc.directed_edge_stats(f, max(len(v), 1))
    print(f"{name}/{variant}: V {len(v)} (want {len(want_v)}) F {len(f)} (want {len(want_f)}) {st}")
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert v.shape == want_v.shape and f.shape == want_f.shape and len(f) > 0
    assert v.tobytes() == want_v.tobytes()
    assert np.array_equal(f, want_f)
    assert st["doubled"] == 0 and st["same_triple"] == 0          # also on the open fields
    if closed:
        assert st == CLEAN
        sv = mc.signed_volume(v - np.asarray(origin), f)
        lo, hi = mc.volume_bracket(vol, level, spacing)
        if closed < 0:                                             # the cells wholly / partly below the level
            case = mc.cell_cases(vol, level)
            cell = float(np.prod(spacing))
            lo, hi = float((case == 255).sum()) * cell, float((case != 0).sum()) * cell
        print(f"{name}/{variant}: signed volume {sv:.6f}, bracket [{lo:.6f}, {hi:.6f}]")
        assert closed * sv > 0 and lo <= closed * sv <= hi
    if not mc.VARIANTS[variant][3]:
        v2, f2 = _mc(pkg, -vol, -level, origin, spacing)
        assert v2.tobytes() == v.tobytes()
        assert np.array_equal(mc.canon_rows(f2[:, ::-1]), mc.canon_rows(f))


def test_fields_exercise_the_cases_whose_fans_moved(fields):
    """The fields above hold the cases the fan rule changes, the 26 whose complement the earlier rule treated
    differently among them: the negated-field comparison is not vacuous."""
    rows = mc.rows()
    moved = {c for c in range(256) if mc.refan(rows[c]) != list(rows[c])}
    asym = {c for c in range(256) if mc.refan(rows[c]) != mc.first_valid_fan(rows[c])}
    for name in ("cases", "random_12x10x14", "plateau_16x16x16"):
        seen = set(np.unique(mc.cell_cases(fields[name][0], 0.0)).tolist())
        assert seen & moved, name
    assert moved <= set(np.unique(mc.cell_cases(fields["cases"][0], 0.0)).tolist())
    assert len(asym) == 16 and asym & set(np.unique(mc.cell_cases(fields["random_12x10x14"][0], 0.0)).tolist())


# ------------------------------------------------------------------------------------------------
# B: the two extractors against each other
# ------------------------------------------------------------------------------------------------
def _keys(pos, dims):
    """(lattice point, axis) of vertices at lattice positions `pos` (unit spacing, one fractional coordinate)
    → (key int64 [V], t float64 [V])."""
    base = np.floor(pos)
    frac = pos - base
    assert ((frac > 0).sum(1) == 1).all()                              # 0 < t < 1 on exactly one axis
    ax = np.argmax(frac > 0, 1)
    p = base.astype(np.int64)
    lin = (p[:, 0] * dims[1] + p[:, 1]) * dims[2] + p[:, 2]
    return lin * 3 + ax, frac[np.arange(len(pos)), ax]


def test_dense_and_block_extractors_agree(pkg):
    """One 32 x 32 x 16 field (all 256 cases) through both: the same vertices on the same lattice edges with
    bit-equal t ((0 - a) / (b - a) and a / (a - b) round alike; positions are exact in float64 at unit
    spacing), and the same triangles with opposite winding (the block volume's outside is above the level)."""
    import torch
    shape, seed = mc.PAIR_FIELD
    vol = mc.random_field(shape, seed)
    v, f = _mc(pkg, vol, 0.0)
    blocks = [(bx, by) for bx in range(2) for by in range(2)]
    tsdf = np.stack([vol[16 * bx:16 * bx + 16, 16 * by:16 * by + 16, :].reshape(4096) for bx, by in blocks], 0)
    key = np.array([bx * 2 + by for bx, by in blocks], dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tv, tf, tcol = pkg.ops.tsdf_marching_cubes(t(tsdf), t(np.ones_like(tsdf)), None, t(key), 4,
                                               t(np.arange(4, dtype=np.int32)), (0, 0, 0), (2, 2, 1), 1.0)
    torch.cuda.synchronize()
    tv, tf = tv.cpu().numpy(), tf.cpu().numpy()
    assert tcol is None and len(f) > 10000 and tf.shape == f.shape and tv.shape == v.shape
    kd, td = _keys(v, shape)
    kt, tt = _keys(tv - 0.5, shape)                                    # the block volume samples voxel centres
    assert np.unique(kd).size == kd.size and np.array_equal(np.sort(kd), np.sort(kt))
    od, ot = np.argsort(kd), np.argsort(kt)
    assert td[od].tobytes() == tt[ot].tobytes()
    assert np.array_equal(mc.canon_rows(kd[f]), mc.canon_rows(kt[tf][:, ::-1]))
    assert mc.directed_edge_stats(f, len(v))["doubled"] == 0


# ------------------------------------------------------------------------------------------------
# C: a hand-built pool
# ------------------------------------------------------------------------------------------------
def test_block_extractor_on_a_hand_built_pool(pkg):
    """A 2 x 2 x 2 table with five blocks in a scrambled pool order, random values, about 10 % zero weights, a
    colour pool, and a sixth pool slot that is not in use: vertices, faces and colours equal
    tsdf_cases.extract_ref bit for bit, no edge has more than two faces, and the valid cells hold all 256
    cases: the fan rule is exercised on every row, not on cases 159 and 249 alone."""
    import torch
    rng = np.random.default_rng(21)
    lo, hi = (-1, -1, -1), (1, 1, 1)
    cells = rng.permutation(8)[:5]
    assert (np.diff(cells) < 0).any()                                  # not in key order
    cap, n = 6, 5
    tsdf = (rng.random((cap, 4096)) * 2 - 1).astype(np.float32)
    weight = np.where(rng.random((cap, 4096)) < 0.1, 0.0, rng.integers(1, 4, (cap, 4096))).astype(np.float32)
    color = (rng.random((3, cap, 4096)) * 255).astype(np.float32)
    key = np.full(cap, -1, np.int32)
    key[:n] = cells
    table = np.full(8, -1, np.int32)
    table[cells] = np.arange(n, dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    v, f, c = pkg.ops.tsdf_marching_cubes(t(tsdf), t(weight), t(color), t(key), n, t(table), lo, hi, tc.L)
    torch.cuda.synchronize()
    v, f, c = v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()
    want = tc.extract_ref(tsdf[:n], weight[:n], color[:, :n], cells, lo, hi)
    print(f"pool: V {len(v)} F {len(f)}, valid cells {len(want['cases'])}")
    assert np.bincount(want["cases"], minlength=256).min() > 0
    assert f.shape == want["faces"].shape and len(f) > 5000
    assert np.array_equal(f, want["faces"])
    assert v.tobytes() == want["vertices"].tobytes()
    assert np.array_equal(c, want["colors"])
    e = np.sort(mc.directed_edges(f), 1)
    assert np.unique(e[:, 0] * len(v) + e[:, 1], return_counts=True)[1].max() <= 2
    assert mc.directed_edge_stats(f, len(v))["doubled"] == 0


# ------------------------------------------------------------------------------------------------
# D: cleaning
# ------------------------------------------------------------------------------------------------
def _host_keep(v, f, label, keep_labels):
    """(vertex ids kept, their positions, the kept faces' corner positions) of a host selection."""
    fk = np.isin(label[f[:, 0]], keep_labels)
    used = np.zeros(len(v), bool)
    used[f[fk].reshape(-1)] = True
    return np.flatnonzero(used), v[used], v[f[fk]]


def test_components_of_the_case_volume(pkg, fields):
    """296 components of very different sizes in one mesh: labels are the lowest vertex id of each component
    (the host union-find's), areas are within 1e-9 relative of float64 sums, and the two selections of
    mesh_keep_components equal host selections."""
    import torch
    ops = pkg.ops
    vol, level, origin, spacing = mc.variant_of(fields["cases"][0], "placed")
    v, f = mc.reference_mc(vol, level, origin, spacing)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    label = mc.components(f, len(v))
    roots = np.unique(label)
    fa = mc.face_areas(v, f)
    area = np.zeros(len(v))
    np.add.at(area, label[f[:, 0]], fa)
    assert len(roots) == 296

    got_l, got_a = ops.mesh_components(tv, tf)
    got_l, got_a = got_l.cpu().numpy(), got_a.cpu().numpy()
    assert got_l.dtype == np.int32 and np.array_equal(got_l, label)
    rel = np.abs(got_a[roots] - area[roots]) / area[roots]
    print(f"components {len(roots)}, areas {area[roots].min():.6f} .. {area[roots].max():.6f}, "
          f"max relative error {rel.max():.2e}")
    assert rel.max() <= 1e-9
    assert np.count_nonzero(got_a) == len(roots) and (got_a[np.setdiff1d(np.arange(len(v)), roots)] == 0).all()

    def check(out, keep_labels):
        kv, kf, ids = (x.cpu().numpy() for x in out)
        want_ids, want_v, want_tri = _host_keep(v, f, label, keep_labels)
        assert np.array_equal(ids, want_ids) and np.array_equal(kv, want_v)
        assert kf.dtype == np.int32 and np.array_equal(kv[kf], want_tri)        # same triangles, same order

    a = np.sort(area[roots])
    assert a[-1] > 1.01 * a[-2]                                 # one largest component (case 255's), no tie
    check(ops.mesh_keep_components(tv, tf, True), roots[[np.argmax(area[roots])]])
    gap = 50 + int(np.argmax(a[51:-50] / a[50:-51]))           # the widest gap between neighbours of the middle ranks
    thr = float(np.sqrt(a[gap] * a[gap + 1]))
    assert a[gap + 1] > 1.01 * a[gap]
    keep = roots[area[roots] > thr]
    assert 50 < len(keep) < len(roots) - 50
    check(ops.mesh_keep_components(tv, tf, False, thr), keep)


def test_components_of_a_long_strip(pkg):
    """One strip of 5000 faces with permuted vertex ids: labels travel a long way (many hook / jump rounds), and
    the call returns with one label for the strip, the lowest id in it; the isolated vertices keep their own
    label and area 0; a face that repeats a vertex adds nothing."""
    import torch
    m = mc.strip_mesh(5000, 5)
    v, f = m["vertices"], m["faces"]
    label, area = pkg.ops.mesh_components(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    torch.cuda.synchronize()
    label, area = label.cpu().numpy(), area.cpu().numpy()
    root = m["strip"].min()
    assert (label[m["strip"]] == root).all()
    assert np.array_equal(label[m["isolated"]], m["isolated"]) and (area[m["isolated"]] == 0).all()
    want = mc.face_areas(v, f).sum()
    print(f"strip: area {area[root]:.9f} vs {want:.9f}")
    assert abs(area[root] - want) <= 1e-9 * want and np.count_nonzero(area) == 1
    kv, kf, ids = pkg.ops.mesh_keep_components(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), True)
    assert np.array_equal(ids.cpu().numpy(), m["strip"]) and kf.shape[0] == f.shape[0]
    assert np.array_equal(kv.cpu().numpy()[kf.cpu().numpy()], v[f])


# ------------------------------------------------------------------------------------------------
# E: no cell, no mesh
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 5), (5, 1, 5), (5, 5, 1)])
def test_a_volume_without_a_cell_gives_the_empty_mesh(pkg, shape):
    vol = (np.random.default_rng(0).random(shape) - 0.5).astype(np.float32)
    assert (vol < 0).any() and (vol > 0).any()                        # its lattice edges do cross the level
    v, f = _mc(pkg, vol, 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float64 and f.dtype == np.int32
