"""CPU-side checks of the TSDF volume: the float32 twin against the float64 statement of the contract (the
float32 floors it prints are the ones DESIGN.md §7h quotes), the input conditions the GPU tests rely on, the
mesh conventions on a wall whose true plane is known, the topology of the reference extraction, argument
validation of the new entry points (no launch) and the Mesher's choice of hull method."""
import ctypes
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import tsdf_cases as tc
from conftest import GOLDEN

MAX_LEFT_OUT = 0.01


@pytest.fixture(scope="module")
def scenes():
    out = {}
    frames, plane = tc.wall_scene()
    for name, fr in (("wall", frames), ("corner", tc.corner_frames(3))):
        lo, hi, n_valid = tc.block_range(fr)
        out[name] = SimpleNamespace(frames=fr, lo=lo, hi=hi, n_valid=n_valid, ref=tc.fuse_ref(fr, lo, hi),
                                    f32=tc.fuse_f32(fr, lo, hi))
    out["wall"].plane = plane
    return out


@pytest.fixture(scope="module")
def meshes(scenes):
    return {k: tc.extract_ref(s.f32.tsdf, s.f32.weight, s.f32.color, s.f32.keys, s.lo, s.hi)
            for k, s in scenes.items()}


@pytest.mark.parametrize("name", ["wall", "corner"])
def test_f32_twin_matches_ref(scenes, name):
    s = scenes[name]
    ref, f32 = s.ref, s.f32
    assert min(s.lo) < 0 <= max(s.hi) - 1 and all(v < 0 for v in s.lo)       # negative block indices on every axis
    assert np.array_equal(ref.coords, f32.coords) and ref.coords.shape[0] > 8
    assert ref.n_outside == f32.n_outside == [0]
    cmp = ~(ref.margin | f32.margin)
    left_out = ref.margin_pairs / ref.updates
    print(f"{name}: blocks {ref.coords.shape[0]}, voxel-frame updates {ref.updates}, left out {left_out:.5f}")
    assert left_out <= MAX_LEFT_OUT and f32.margin_pairs / f32.updates <= MAX_LEFT_OUT
    assert np.array_equal(ref.weight[cmp], f32.weight[cmp].astype(np.float64))
    assert ref.weight.max() == len(s.frames)
    seen = cmp & (ref.weight > 0)
    dt = np.abs(ref.tsdf - f32.tsdf)[seen].max()
    dc = np.abs(ref.color - f32.color)[:, seen].max()
    print(f"{name}: float32 floor: max |tsdf| difference {dt:.3e}, max colour difference {dc:.3e}")
    assert dt < 1e-5 and dc < 1e-3          # a float32 running average of values <= 1 and <= 255


@pytest.mark.parametrize("name", ["wall", "corner"])
def test_samples_span_one_two_and_three_axes(scenes, name):
    spans = np.concatenate([(x["hi"] - x["lo"]).sum(1) for x in map(tc.frame_samples, scenes[name].frames)])
    assert spans.max() <= 3 and spans.min() >= 0
    for n_axes in (1, 2, 3):
        assert (spans == n_axes).any(), n_axes
    faces = np.concatenate([tc.frame_samples(fr)["face_dist"] for fr in scenes[name].frames])
    assert faces.min() > 1e-6               # no sample near a block face: the block sets are not in doubt


def test_a_block_touched_by_frame_0_only_is_seen_by_frame_1(scenes):
    s = scenes["corner"]
    only0 = tc.touched_by_0_only(s.ref, s.frames)
    assert only0 and s.ref.weight[only0[0]].max() == 1.0


def test_cells_cross_block_faces_edges_and_corners(scenes, meshes):
    s, m = scenes["corner"], meshes["corner"]
    at_end = ((m["cells"] % 16) == 15).sum(1)
    for n_axes in (1, 2, 3):
        assert (at_end == n_axes).any(), n_axes
    # a voxel with weight on the high face of its block whose neighbouring block is missing / outside the table
    f = s.f32
    w = f.weight.reshape(-1, 16, 16, 16)
    dims = np.asarray(s.hi) - np.asarray(s.lo)
    missing = border = False
    for pid, c in enumerate(f.coords):
        for ax in range(3):
            sl = [slice(None)] * 3
            sl[ax] = 15
            if not (w[pid][tuple(sl)] > 0).any():
                continue
            i = c - np.asarray(s.lo)
            i[ax] += 1
            if i[ax] >= dims[ax]:
                border = True
            elif f.table[(i[0] * dims[1] + i[1]) * dims[2] + i[2]] < 0:
                missing = True
    assert missing and border


def test_wall_vertices_lie_on_the_plane_and_face_the_camera(scenes, meshes):
    """Independent of the twins' agreement: the plane and the camera are known in closed form."""
    s, m = scenes["wall"], meshes["wall"]
    n, c = s.plane
    v, f = m["vertices"], m["faces"]
    assert v.shape[0] > 200 and f.shape[0] > 200
    dist = np.abs(v @ n - c)
    print(f"wall: V {v.shape[0]} F {f.shape[0]} max distance to the plane {dist.max():.3e}")
    assert dist.max() <= 1e-5
    eye = s.frames[0].c2w[:3, 3]
    fn = tc.face_normals(v, f)
    assert (np.einsum("ij,ij->i", fn, eye - v[f[:, 0]]) > 0).all()
    mr = tc.extract_ref(s.ref.tsdf.astype(np.float32), s.ref.weight.astype(np.float32), None, s.ref.keys, s.lo, s.hi)
    assert np.abs(mr["vertices"] @ n - c).max() <= 1e-5 and mr["colors"] is None


def _edge_face_counts(f, n_verts):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0).astype(np.int64), 1)
    return np.unique(e[:, 0] * n_verts + e[:, 1], return_counts=True)[1]


def test_extract_ref_vertices(meshes):
    m = meshes["corner"]
    v, f = m["vertices"], m["faces"]
    assert v.shape[0] > 500 and f.shape[0] > 500
    assert np.array_equal(np.unique(f), np.arange(v.shape[0]))              # every vertex is referenced
    assert np.unique(v, axis=0).shape[0] == v.shape[0]                      # no position twice
    assert m["colors"].shape == v.shape and m["colors"].dtype == np.uint8
    cnt = _edge_face_counts(f, v.shape[0])
    assert (cnt == 2).sum() > 10 * (cnt == 1).sum()                         # a surface with a boundary


def test_extract_ref_edges_belong_to_at_most_two_faces(meshes):
    """Frames that disagree at this resolution (0.1 m pixels on 0.04 m voxels) give cells with four crossings in
    a face.  The case table's fan from a loop's first vertex can put a diagonal, even a whole triangle, into such
    a face, where the neighbouring cell's fan puts the same one: with the table's own fans 4 of the corner
    scene's 45760 edges belong to 4 faces.  The volume fans every loop from a vertex whose diagonals cross the
    cell's interior (tsdf_cases.refan), and no edge has more than two."""
    for name in ("wall", "corner"):
        m = meshes[name]
        cnt = _edge_face_counts(m["faces"], m["vertices"].shape[0])
        print(f"{name}: edges by number of faces {np.bincount(cnt).tolist()}")
        assert cnt.max() <= 2, name
    assert (np.bincount(meshes["corner"]["cases"], minlength=256)[[159, 249]] > 0).all()   # the cases in question


def test_refan_keeps_the_loops_and_leaves_the_faces_free():
    """Every loop of every case has a vertex from which no diagonal lies in a face of the cell; fanned from
    it, a row keeps its loops, its triangle count and its winding."""
    rows = tc._mc_rows()
    moved = 0
    for case, row in enumerate(rows):
        new = tc.refan(row)
        assert len(new) == len(row), case
        pos = 0
        for loop in tc.row_loops(row):
            n = len(loop)
            tris = new[pos:pos + n - 2]
            pos += n - 2
            start = loop.index(tris[0][0])
            turned = loop[start:] + loop[:start]
            assert tris == [(turned[0], turned[i], turned[i + 1]) for i in range(1, n - 1)], case   # same cycle
            for t in tris:
                for u, v in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                    gap = (turned.index(v) - turned.index(u)) % n
                    if gap not in (1, n - 1):                                   # a diagonal of the loop
                        assert not (tc.edge_faces(u) & tc.edge_faces(v)), (case, t)
            moved += start != 0
        assert pos == len(row)
    assert moved > 0 and tc.refan(rows[159]) != rows[159]


# ------------------------------------------------------------------------------------------------
# the library and the Mesher, without a device
# ------------------------------------------------------------------------------------------------
TSDF_EXPORTS = ("nslam_tsdf_block_range", "nslam_tsdf_touch", "nslam_tsdf_integrate", "nslam_tsdf_mc_count",
                "nslam_tsdf_mc_emit")


def test_exports_exist(pkg):
    L = pkg._lib.lib()
    for name in TSDF_EXPORTS:
        assert name in pkg._lib.EXPORTS and hasattr(L, name), name
    assert hasattr(pkg, "tsdf") and hasattr(pkg.tsdf, "TSDFVolume")


def test_entry_points_validate_without_gpu(pkg):
    L = pkg._lib.lib()
    E, U = -1, -2
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)  # noqa: E731
    lo, hi, empty = i3(-2, -2, -2), i3(2, 2, 2), i3(2, -2, 2)
    P = 4096  # a fake, aligned, never dereferenced device pointer

    def rng(depth=P, c2w=P, K=2, stride=4, voxel=0.04, trunc=0.12, out=P, cnt=P):
        return L.nslam_tsdf_block_range(depth, c2w, K, 24, 32, 15.0, 15.0, 15.5, 11.5, stride, 1000.0, voxel, trunc,
                                        out, cnt, None)

    def tch(depth=P, c2w=P, K=2, stride=4, voxel=0.04, trunc=0.12, lo=lo, hi=hi, mask=P, cnt=P):
        return L.nslam_tsdf_touch(depth, c2w, K, 24, 32, 15.0, 15.0, 15.5, 11.5, stride, 1000.0, voxel, trunc, lo, hi,
                                  mask, cnt, None)

    def itg(depth=P, w2c=P, K=2, voxel=0.04, trunc=0.12, lo=lo, hi=hi, key=P, ids=P, mask=P, n_list=3, n_pool=5,
            tsdf=P, weight=P, cpool=None, color=None, cstride=0):
        return L.nslam_tsdf_integrate(depth, color, w2c, K, 24, 32, 15.0, 15.0, 15.5, 11.5, 1000.0, voxel, trunc, lo,
                                      hi, key, ids, mask, n_list, n_pool, tsdf, weight, cpool, cstride, None)

    def cnt(tsdf=P, weight=P, key=P, n_pool=5, table=P, lo=lo, hi=hi, flags=P, ntri=P):
        return L.nslam_tsdf_mc_count(tsdf, weight, key, n_pool, table, lo, hi, flags, ntri, None)

    def emt(tsdf=P, weight=P, key=P, n_pool=5, table=P, lo=lo, hi=hi, voxel=0.04, flags=P, voff=P, nv=7, nf=9,
            verts=P, faces=P):
        return L.nslam_tsdf_mc_emit(tsdf, weight, None, 0, key, n_pool, table, lo, hi, voxel, flags, P, voff, P, nv,
                                    nf, verts, None, faces, None)

    for call in (rng, tch, itg):
        assert call(depth=None) == E
        assert call(K=0) == E
        assert call(voxel=0.0) == E and call(voxel=-1.0) == E and call(trunc=0.0) == E
    assert rng(c2w=None) == E and rng(out=None) == E and rng(cnt=None) == E
    assert rng(stride=0) == E and tch(stride=0) == E
    assert rng(trunc=0.4) == E                                  # 2 trunc > 16 voxel
    assert tch(K=33) == E and itg(K=33) == E
    assert tch(mask=None) == E and tch(cnt=None) == E and tch(c2w=None) == E
    for call in (tch, itg, cnt, emt):
        assert call(lo=None) == E and call(hi=None) == E
        assert call(lo=hi, hi=lo) == E and call(hi=empty) == E  # an empty box
        assert call(lo=i3(0, 0, 0), hi=i3(1024, 1024, 1024)) == E   # more than 2^27 cells
    assert itg(w2c=None) == E and itg(key=None) == E and itg(ids=None) == E and itg(tsdf=None) == E
    assert itg(n_list=6) == E                                   # more listed blocks than pool blocks
    assert itg(cpool=P, color=None, cstride=5 * 4096) == E      # a colour pool without colour images
    assert itg(cpool=P, color=P, cstride=4096) == E             # colour planes closer than the pool is long
    assert itg(n_list=0, key=None, ids=None, mask=None) == 0    # nothing listed: no launch
    assert itg(n_pool=(1 << 31) // (3 * 4096) + 1) == U
    assert cnt(tsdf=None) == E and cnt(table=None) == E and cnt(flags=None) == E and cnt(n_pool=-1) == E
    assert cnt(n_pool=0, tsdf=None, weight=None, key=None, table=None, flags=None, ntri=None) == 0
    assert cnt(n_pool=(1 << 31) // (3 * 4096) + 1) == U
    assert emt(verts=None) == E and emt(voff=None) == E and emt(voxel=0.0) == E and emt(nv=-1) == E
    assert emt(nv=0, nf=0, verts=None, faces=None) == 0         # no crossing: no launch


def test_volume_checks_its_arguments_without_gpu(pkg):
    T = pkg.tsdf.TSDFVolume
    with pytest.raises(ValueError, match="empty"):
        T(0.04, 0.12, [0, 0, 0], [1, 0, 1], "cpu")
    with pytest.raises(ValueError, match=r"\[\[-600, 0, 0\], \[600, 600, 600\]\)"):
        T(0.04, 0.12, [-600, 0, 0], [600, 600, 600], "cpu")       # the message names the block range
    with pytest.raises(ValueError):
        T(0.04, 0.4, [0, 0, 0], [1, 1, 1], "cpu")
    with pytest.raises(ValueError):
        T(0.0, 0.12, [0, 0, 0], [1, 1, 1], "cpu")
    flipped = pkg.tsdf.opengl_to_cv(np.eye(4, dtype=np.float32))
    assert flipped.dtype == np.float32 and np.array_equal(np.diag(flipped), [1, -1, -1, 1])


def _mesher(pkg, **over):
    import torch
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import mesh_scene
    cfg = {"coarse": True, "scale": 1, "occupancy": True,
           "meshing": {"resolution": mesh_scene.GRID_RES, "level_set": 0, "clean_mesh_bound_scale": 1.02,
                       "remove_small_geometry_threshold": 0.2, "color_mesh_extraction_method": "direct_point_query",
                       "get_largest_components": False, "depth_test": True},
           "mapping": {"marching_cubes_bound": mesh_scene.MC_BOUND}}
    cfg["meshing"].update(over)
    slam = SimpleNamespace(renderer=None, bound=torch.tensor(mesh_scene.MC_BOUND, dtype=torch.float64), nice=True,
                           verbose=False, **mesh_scene.CAM)
    return pkg.Mesher(cfg, None, slam), mesh_scene


def test_bound_from_defaults_to_points(pkg):
    pytest.importorskip("scipy")
    import torch
    m, ms = _mesher(pkg)
    _, poses, depths = ms.mask_scene()
    kfs = [{"est_c2w": torch.from_numpy(p), "depth": torch.from_numpy(d)} for p, d in zip(poses, depths)]
    assert m.bound_from == "points"
    default = m.get_bound_from_frames(kfs, 1)
    assert default.tobytes() == m.get_bound_from_frames(kfs, 1, method="points").tobytes()
    assert default.tobytes() == _mesher(pkg, bound_from="points")[0].get_bound_from_frames(kfs, 1).tobytes()
    with pytest.raises(ValueError, match="voxels"):
        m.get_bound_from_frames(kfs, 1, method="voxels")
    with pytest.raises(ValueError, match="hull"):
        _mesher(pkg, bound_from="hull")[0].get_bound_from_frames(kfs, 1)
