"""CPU-side checks of tests/mc_cases.py: the inputs of tests/test_gpu_mc_cases.py hold what that file says they
hold, the plain reference extractor gives a closed mesh of the expected topology, its invariants can fail (the
table's own fans do fail them), and the fan rule is the one both extractors' twins use and is symmetric under a
sign flip.  No device, no kernel code."""
import numpy as np
import pytest

import mc_cases as mc
import tsdf_cases as tc

# the block-volume extractor's earlier rule (first valid apex in loop order) gave these cases and their
# complements different triangles
FIRST_VALID_ASYMMETRIC = (6, 18, 26, 38, 70, 72, 73, 82, 88, 96, 97, 109, 121)


@pytest.fixture(scope="module")
def case_mesh():
    vol = mc.case_volume()
    return (vol,) + mc.reference_mc(vol, 0.0)


def test_case_volume_holds_every_case_in_a_centre_cell():
    vol = mc.case_volume()
    assert vol.shape == (4, 4, 1024) and vol.dtype == np.float32 and set(np.unique(vol)) == {-1.0, 1.0}
    case = mc.cell_cases(vol, 0.0)
    assert np.array_equal(case[tuple(mc.case_cells().T)], np.arange(256))
    # every block's outer layer is above the level: the case's surface closes inside its own block
    b = vol.reshape(4, 4, 256, 4)
    assert (b[[0, 3]] == 1).all() and (b[:, [0, 3]] == 1).all() and (b[:, :, :, [0, 3]] == 1).all()
    assert np.array_equal(mc.cell_cases(vol, 0.25), case)


def test_reference_mesh_of_the_case_volume_is_closed(case_mesh):
    """8032 faces in 296 closed components of Euler characteristic 2 each (counted here by union-find over the
    reference's faces; the issue's host emulation gave the same figures)."""
    vol, v, f = case_mesh
    st = mc.directed_edge_stats(f, len(v))
    print(f"case volume: V {len(v)} F {len(f)} {st}")
    assert st == {"doubled": 0, "unmatched": 0, "same_triple": 0}
    assert np.array_equal(np.unique(f), np.arange(len(v)))           # every vertex is used
    eu = mc.euler_by_component(f, len(v))
    assert len(f) == 8032 and len(eu) == 296 and set(eu.values()) == {2}
    # the surface encloses the below-level corners: negative volume, between the all-below and any-below cells
    lo, hi = mc.volume_bracket(-vol, 0.0, (1.0, 1.0, 1.0))
    sv = mc.signed_volume(v, f)
    assert lo <= -sv <= hi and sv < 0


def test_the_invariants_can_fail():
    """With the table's own fans the same emulation shows doubled directed edges and pairs of triangles on the
    same three vertices: 76 / 19 on the case volume, 80 / 20 on the seed-3 field."""
    for name, vol in (("cases", mc.case_volume()), ("seed 3", mc.random_field((12, 10, 14), 3))):
        v, f = mc.reference_mc(vol, 0.0, fan_rule=mc.table_fan)
        st = mc.directed_edge_stats(f, len(v))
        print(f"{name}: table fans: F {len(f)} {st}")
        assert st["doubled"] > 0 and st["same_triple"] > 0, name
        assert st["unmatched"] == 0, name      # which is why sort(key) == sort(rev) alone did not notice
        v2, f2 = mc.reference_mc(vol, 0.0)
        assert np.array_equal(v2, v) and len(f2) == len(f) and not np.array_equal(f2, f)


def _oriented(tris):
    """A row's triangles as a sorted list of rotations that start at the lowest edge id."""
    out = []
    for t in tris:
        k = t.index(min(t))
        out.append((t[k], t[(k + 1) % 3], t[(k + 2) % 3]))
    return sorted(out)


def test_the_rule_is_symmetric_under_a_sign_flip():
    rows = mc.rows()
    bad_new, bad_old = [], []
    for c in range(256):
        for rule, bad in ((mc.refan, bad_new), (mc.first_valid_fan, bad_old)):
            flipped = [(t[0], t[2], t[1]) for t in rule(rows[255 - c])]
            if _oriented(rule(rows[c])) != _oriented(flipped):
                bad.append(c)
    assert bad_new == []
    want = sorted(FIRST_VALID_ASYMMETRIC + tuple(255 - c for c in FIRST_VALID_ASYMMETRIC))
    assert bad_old == want                    # the finding this rule answers


def test_every_loop_has_a_valid_apex_and_the_twins_agree():
    rows = mc.rows()
    changed, differs = [], []
    for c, row in enumerate(rows):
        loops = mc.row_loops(row)
        assert sum(len(lp) - 2 for lp in loops) == len(row)
        for lp in loops:
            assert lp[0] == min(lp) and len(lp) <= 8, c              # a loop is listed from its lowest edge
            assert mc.valid_apices(lp), c
        new = mc.refan(row)
        assert new == tc.refan(row), c                               # the block-volume twin uses the same rule
        if new != list(row):
            changed.append(c)
            assert any(0 not in mc.valid_apices(lp) for lp in loops), c     # only where loop[0] is not valid
        if new != mc.first_valid_fan(row):
            differs.append(c)
            assert max(len(lp) for lp in loops) in (6, 7), c
    print(f"rows changed by the rule: {len(changed)}; different from the first valid apex: {differs}")
    assert len(changed) > 0 and len(differs) == 16


def _slow_mc(vol, level, origin, spacing):
    """Marching cubes in plain loops, one cell and one edge at a time."""
    nx, ny, nz = vol.shape
    lv = np.float32(level)
    vid, verts = {}, []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                for ax in range(3):
                    q = [i, j, k]
                    q[ax] += 1
                    if q[ax] >= vol.shape[ax]:
                        continue
                    a, b = vol[i, j, k], vol[tuple(q)]
                    if (a < lv) == (b < lv):
                        continue
                    t = np.float32(lv - a) / np.float32(b - a)
                    p = [float(i), float(j), float(k)]
                    p[ax] += float(t)
                    vid[(i, j, k, ax)] = len(verts)
                    verts.append([origin[c] + p[c] * spacing[c] for c in range(3)])
    faces = []
    table = [mc.refan(r) for r in mc.rows()]
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                cs = sum(1 << c for c in range(8) if vol[i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)] < lv)
                for tri in table[cs]:
                    ids = []
                    for e in tri:
                        ax, ea, eb = e >> 2, e & 1, (e >> 1) & 1
                        off = [0, 0, 0]
                        o1, o2 = [x for x in range(3) if x != ax]
                        off[o1], off[o2] = ea, eb
                        ids.append(vid[(i + off[0], j + off[1], k + off[2], ax)])
                    faces.append(ids)
    return np.array(verts).reshape(-1, 3), np.array(faces, dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("shape,seed,variant", [((5, 4, 6), 1, "plain"), ((4, 6, 5), 2, "hits"), ((2, 8, 7), 3, "placed")])
def test_reference_matches_plain_loops(shape, seed, variant):
    vol, level, origin, spacing = mc.variant_of(mc.random_field(shape, seed), variant)
    v, f = mc.reference_mc(vol, level, origin, spacing)
    sv, sf = _slow_mc(vol, level, origin, spacing)
    assert len(f) > 20 and v.tobytes() == sv.tobytes() and np.array_equal(f, sf)


def test_a_value_at_the_level_is_not_below_it():
    vol = np.full((3, 3, 3), -1.0, np.float32)
    vol[1, 1, 1] = 0.25
    v, f = mc.reference_mc(vol, 0.25)
    assert len(v) == 6 and len(f) == 8                # an octahedron shrunk to the point itself
    assert (v == 1.0).all() and (mc.face_areas(v, f) == 0).all()
    vol[1, 1, 1] = np.nextafter(np.float32(0.25), np.float32(0))
    assert len(mc.reference_mc(vol, 0.25)[0]) == 0


def test_gpu_fields_hold_the_edges_they_are_there_for():
    """Every random / plateau field of the GPU tests has a cell face with four crossings, at both levels and
    with level hits.  The exception is (3, 3, 3): it has one value inside its shell, and four crossings in a
    face need two differing diagonals; it is there for the smallest closed volume, and must have a surface."""
    fields = mc.gpu_fields()
    assert set(fields) == {"cases", "plateau_16x16x16"} | set(mc.RANDOM_SHAPES)
    for name, (vol, closed) in fields.items():
        assert vol.dtype == np.float32 and vol.size <= 16384 + 4 * 4 * 1024, name
        for variant in mc.VARIANTS:
            fv, level, _, _ = mc.variant_of(vol, variant)
            n_faces = len(mc.reference_mc(fv, level)[1])
            assert n_faces > 0, (name, variant)
            if name != "random_3x3x3":
                assert mc.has_four_crossing_face(fv, level), (name, variant)
            if mc.VARIANTS[variant][3] and name != "random_3x3x3":
                assert (fv == np.float32(level)).sum() > 0, name
        assert closed == (-1 if name == "cases" else int(mc.is_closed_shape(vol.shape))), name
    assert all(fields[n][0].size % 256 for n in mc.RANDOM_SHAPES)     # point counts off the workgroup size
    assert fields["random_2x3x257"][0].shape[2] > 256
    hits = mc.variant_of(fields["random_12x10x14"][0], "hits")[0]
    frac = (hits[1:-1, 1:-1, 1:-1] == np.float32(0.25)).mean()
    assert 0.03 < frac < 0.07
    v, f = mc.reference_mc(hits, 0.25)
    assert (mc.face_areas(v, f) == 0).any()                            # legitimate zero-area triangles


def test_pair_field_holds_all_256_cases():
    shape, seed = mc.PAIR_FIELD
    assert shape == (32, 32, 16)
    cnt = np.bincount(mc.cell_cases(mc.random_field(shape, seed), 0.0).reshape(-1), minlength=256)
    print(f"32 x 32 x 16: cells per case {cnt.min()} .. {cnt.max()}")
    assert cnt.min() > 0
    cnt = np.bincount(mc.cell_cases(mc.random_field((31, 31, 31), 1), 0.0).reshape(-1), minlength=256)
    print(f"31^3: at least {cnt.min()} cells per case")
    assert cnt.min() > 0


def test_plateau_field_has_plateaus_side_by_side():
    vol = mc.plateau_field(*mc.PLATEAU)
    inner = vol[1:-1, 1:-1, 1:-1]
    assert (inner == -100).mean() > 0.1 and (inner == 100).mean() > 0.1
    smooth = inner[np.abs(inner) < 100]
    assert smooth.size > 0.5 * inner.size and (smooth < 0).any() and (smooth > 0).any()
    assert ((vol[:-1] == -100) & (vol[1:] == 100)).any()              # -100 next to +100
    v, f = mc.reference_mc(vol, 0.0)
    assert mc.directed_edge_stats(f, len(v)) == {"doubled": 0, "unmatched": 0, "same_triple": 0}
    st = mc.directed_edge_stats(mc.reference_mc(vol, 0.0, fan_rule=mc.table_fan)[1], len(v))
    assert st["doubled"] > 0                                          # the defect on a mesher-like volume


def test_a_volume_without_a_cell_has_no_mesh():
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        vol = (np.random.default_rng(0).random(shape) - 0.5).astype(np.float32)
        v, f = mc.reference_mc(vol, 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32


def test_emit_refuses_counts_for_a_volume_without_a_cell(pkg):
    """nslam_mc_emit, before any device call: a volume with a dimension of 1 has no vertex and no face."""
    import ctypes
    L = pkg._lib.lib()
    three = (ctypes.c_double * 3)(0, 0, 0)
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        assert L.nslam_mc_emit(64, *dims, 0.0, three, three, 64, 64, 3, 0, 64, 64, None) == -1
        assert L.nslam_mc_emit(64, *dims, 0.0, three, three, 64, 64, 0, 0, None, None, None) == 0


def test_strip_mesh():
    m = mc.strip_mesh(5000, 5)
    v, f = m["vertices"], m["faces"]
    assert v.shape == (5005, 3) and f.shape == (5001, 3) and f.dtype == np.int32
    assert (f[-1, 0] == f[-1, 1]) and len(set(f[-1].tolist())) == 2   # the face that repeats a vertex
    assert not np.isin(m["isolated"], f).any() and np.array_equal(np.unique(f), m["strip"])
    label = mc.components(f, len(v))
    assert (label[m["strip"]] == m["strip"].min()).all()
    assert np.array_equal(label[m["isolated"]], m["isolated"])
    assert not np.array_equal(m["strip"], np.arange(5002))             # the ids are permuted
    assert (mc.face_areas(v, f)[:-1] > 0).all() and mc.face_areas(v, f)[-1] == 0
