"""CPU-side checks of the mesher: the generated marching-cubes table, argument validation of the new entry
points (no launch), the PLY writer / reader, get_grid_uniform against the reference's recording, and the
convex-hull bound (needs scipy)."""
import ctypes
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, REPO


def _gen():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(REPO, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _gen()


@pytest.fixture(scope="module")
def mesh_fix():
    with np.load(os.path.join(GOLDEN, "mesh_fixtures.npz")) as z:
        return {k: z[k] for k in z.files}


def _canon(loop):
    """A directed cycle as a tuple starting at its smallest element."""
    k = loop.index(min(loop))
    return tuple(loop[k:] + loop[:k])


def test_mc_table_loops(gen):
    rows, width = gen.build_table()
    assert len(rows) == 256 and width == max(len(r) for r in rows)
    for case in range(256):
        crossing = sorted(e for e, (a, b) in enumerate(gen.EDGES) if ((case >> a) & 1) != ((case >> b) & 1))
        loops = gen.case_loops(case)
        flat = sorted(e for lp in loops for e in lp)
        assert flat == crossing, case                     # every crossing edge lies in exactly one loop
        for lp in loops:
            assert len(lp) >= 3 and len(set(lp)) == len(lp), case
            # closed: consecutive loop vertices (cyclically) share a cube face
            for a, b in zip(lp, lp[1:] + lp[:1]):
                ca, cb = set(gen.EDGES[a]), set(gen.EDGES[b])
                assert any(ca <= set(ring) and cb <= set(ring) for _, ring in gen.FACES), (case, a, b)
        assert len(rows[case]) == sum(len(lp) - 2 for lp in loops), case
        # the opposite sign configuration: the same loops, reversed
        mine = sorted(_canon(lp) for lp in loops)
        other = sorted(_canon(lp[::-1]) for lp in gen.case_loops(255 - case))
        assert mine == other, case
    assert rows[0] == [] and rows[255] == []


def test_mc_table_single_corner_winding(gen):
    """Corner 0 below the level: one triangle whose right-hand normal points at corner 0 (toward lower values)."""
    (tri,) = gen.build_table()[0][1]
    p = [np.array(gen._mid(e)) for e in tri]
    n = np.cross(p[1] - p[0], p[2] - p[0])
    assert np.dot(n, np.zeros(3) - p[0]) > 0


def test_committed_table_is_the_generated_one(gen):
    with open(gen.header_path()) as f:
        assert f.read() == gen.render_header()


def test_mesh_entry_points_validate_without_gpu(pkg):
    L = pkg._lib.lib()
    E, U, WS = -1, -2, -3
    three = (ctypes.c_double * 3)(0, 0, 0)
    assert L.nslam_point_masks_workspace_size(4096, 3, 1024) >= 4 * 3 * 4
    assert L.nslam_point_masks_workspace_size(0, 3, 1024) == 0
    assert L.nslam_point_masks(None, 10, 64, 1, 64, 24, 32, 1.0, 1.0, 0.0, 0.0, 1, 0, 4, 64, 64, 64, 64, 1 << 20,
                               None) == E          # NULL points
    assert L.nslam_point_masks(64, 10, 64, 1, 64, 24, 32, 1.0, 1.0, 0.0, 0.0, 1, 0, 0, 64, 64, 64, 64, 1 << 20,
                               None) == E          # points_batch_size 0
    assert L.nslam_point_masks(64, 10, 64, 1, None, 24, 32, 1.0, 1.0, 0.0, 0.0, 1, 0, 4, 64, 64, 64, 64, 1 << 20,
                               None) == E          # depth needed
    assert L.nslam_point_masks(64, 10, 64, 1, 64, 24, 32, 1.0, 1.0, 0.0, 0.0, 1, 0, 4, 64, 64, 64, 64, 8,
                               None) == WS         # 3 chunks x 1 frame need more than 8 bytes
    assert L.nslam_point_masks(None, 0, None, 0, None, 24, 32, 1.0, 1.0, 0.0, 0.0, 1, 0, 4, None, None, None, None,
                               0, None) == 0       # empty: no launch
    assert L.nslam_mc_workspace_size(24, 20, 28) == 24 * 20 * 28 * 4
    assert L.nslam_mc_count(None, 4, 4, 4, 0.0, 64, 256, None) == E
    assert L.nslam_mc_count(64, 4, 0, 4, 0.0, 64, 256, None) == E
    assert L.nslam_mc_count(64, 4, 4, 4, 0.0, 64, 255, None) == WS
    assert L.nslam_mc_count(64, 1024, 1024, 1024, 0.0, 64, 1 << 40, None) == U   # int32 vertex ids
    assert L.nslam_mc_emit(64, 4, 4, 4, 0.0, None, three, 64, 64, 1, 1, 64, 64, None) == E
    assert L.nslam_mc_emit(64, 4, 4, 4, 0.0, three, three, 64, 64, 1, 1, None, 64, None) == E
    assert L.nslam_mc_emit(64, 4, 4, 4, 0.0, three, three, 64, 64, 0, 0, None, None, None) == 0
    assert L.nslam_points_in_hull(None, 0, 5, 64, 6, 64, None) == E
    assert L.nslam_points_in_hull(64, 0, 5, None, 6, 64, None) == E
    assert L.nslam_points_in_hull(None, 0, 0, None, 0, None, None) == 0
    assert L.nslam_mesh_face_cull(None, 5, 64, 9, 64, None) == E
    assert L.nslam_mesh_face_cull(64, 5, 64, 0, 64, None) == E
    assert L.nslam_mesh_face_cull(None, 0, None, 0, None, None) == 0
    assert L.nslam_mesh_components(None, 5, 64, 2, 64, 64, 64, None) == E
    assert L.nslam_mesh_components(64, 5, None, 2, 64, 64, 64, None) == E
    assert L.nslam_mesh_components(64, 5, 64, 2, 64, 64, None, None) == E
    assert L.nslam_mesh_select(None, 5, 64, 64, None, 0.0, 64, 64, None) == E
    assert L.nslam_mesh_select(None, 0, None, None, None, 0.0, None, None, None) == 0
    assert L.nslam_mesh_remap(64, 5, None, 64, None) == E
    assert L.nslam_mesh_remap(None, 0, None, None, None) == 0


def test_wrappers_check_tensors_before_any_pointer(pkg):
    import torch
    ops = pkg.ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.marching_cubes(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.points_in_hull(torch.zeros(4, 3), torch.zeros(6, 4, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.points_in_hull(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(6, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mesh_components(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int32))


def test_ply_round_trip(pkg, tmp_path):
    M = pkg.mesher
    rng = np.random.default_rng(0)
    v = rng.standard_normal((17, 3))
    f = rng.integers(0, 17, size=(9, 3)).astype(np.int32)
    c = rng.integers(0, 256, size=(17, 3), dtype=np.uint8)
    p = str(tmp_path / "m.ply")
    M.write_ply(p, v, f, c)
    got = M.read_ply(p)
    assert got["vertices"].dtype == np.float32 and (got["vertices"] == v.astype(np.float32)).all()
    assert got["faces"].dtype == np.int32 and (got["faces"] == f).all()
    assert (got["colors"][:, :3] == c).all() and (got["colors"][:, 3] == 255).all()
    head = open(p, "rb").read(400).split(b"end_header\n")[0].decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 17"]
    assert "property list uchar int vertex_indices" in head and "property uchar alpha" in head
    assert os.path.getsize(p) == len("\n".join(head)) + len("end_header\n") + 17 * 16 + 9 * 13
    M.write_ply(p, v, f)  # no colours
    got = M.read_ply(p)
    assert got["colors"] is None and (got["faces"] == f).all()
    M.write_ply(p, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    got = M.read_ply(p)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
    with pytest.raises(ValueError):
        M.write_ply(p, v, f, c.astype(np.float32))


def _mesher(pkg, **over):
    import torch
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import mesh_scene
    cam = dict(mesh_scene.CAM)
    cam.update(over.pop("cam", {}))
    cfg = {"coarse": True, "scale": 1, "occupancy": True,
           "meshing": {"resolution": mesh_scene.GRID_RES, "level_set": 0, "clean_mesh_bound_scale": 1.02,
                       "remove_small_geometry_threshold": 0.2, "color_mesh_extraction_method": "direct_point_query",
                       "get_largest_components": False, "depth_test": True},
           "mapping": {"marching_cubes_bound": mesh_scene.MC_BOUND}}
    cfg["meshing"].update(over)
    slam = SimpleNamespace(renderer=None, bound=torch.tensor(mesh_scene.MC_BOUND, dtype=torch.float64), nice=True,
                           verbose=False, **cam)
    return pkg.Mesher(cfg, None, slam), mesh_scene


def test_get_grid_uniform_matches_reference_bit_for_bit(pkg, mesh_fix):
    m, ms = _mesher(pkg)
    g = m.get_grid_uniform(ms.GRID_RES)
    assert str(g["grid_points"].dtype) == "torch.float32"
    assert g["grid_points"].numpy().tobytes() == mesh_fix["grid_points"].tobytes()
    for name, ax in zip("xyz", g["xyz"]):
        assert np.asarray(ax, dtype=np.float64).tobytes() == mesh_fix["grid_" + name].tobytes()
    # y is the slowest axis of the flattened list (np.meshgrid's default 'xy' order)
    R = ms.GRID_RES
    pts = g["grid_points"].numpy().reshape(R, R, R, 3)
    assert (pts[:, 0, 0, 1] == np.asarray(g["xyz"][1]).astype(np.float32)).all()
    assert (pts[0, :, 0, 0] == np.asarray(g["xyz"][0]).astype(np.float32)).all()


def test_render_ray_along_normal_is_not_implemented(pkg):
    m, _ = _mesher(pkg, color_mesh_extraction_method="render_ray_along_normal")
    with pytest.raises(NotImplementedError):
        m.get_mesh("unused.ply", None, None, [], None, 0)


def test_bound_from_frames_contains_its_points(pkg):
    pytest.importorskip("scipy")
    import torch
    m, ms = _mesher(pkg, clean_mesh_bound_scale=1.02)
    _, poses, depths = ms.mask_scene()
    kfs = [{"est_c2w": torch.from_numpy(p), "depth": torch.from_numpy(d)} for p, d in zip(poses, depths)]
    stride = 4
    planes = m.get_bound_from_frames(kfs, 1, stride=stride)
    assert planes.dtype == np.float64 and planes.shape[1] == 4 and planes.shape[0] >= 4
    cam = ms.CAM
    jj, ii = np.meshgrid(np.arange(0, cam["H"], stride), np.arange(0, cam["W"], stride), indexing="ij")
    n_pts = 0
    for p, d in zip(poses, depths):
        dd = d[::stride, ::stride].astype(np.float64)
        dirs = np.stack([(ii - cam["cx"]) / cam["fx"], -(jj - cam["cy"]) / cam["fy"], -np.ones(ii.shape)], -1)
        w = (dirs * dd[..., None]).reshape(-1, 3)[dd.reshape(-1) > 0] @ p[:3, :3].astype(np.float64).T + p[:3, 3]
        w = np.concatenate([w, p[None, :3, 3].astype(np.float64)], 0)
        assert (w @ planes[:, :3].T + planes[:, 3] <= 1e-9).all()
        n_pts += w.shape[0]
    assert n_pts > 100
    # the hull is grown, not shrunk: scale 1 is strictly inside scale 1.02
    m1, _ = _mesher(pkg, clean_mesh_bound_scale=1.0)
    p1 = m1.get_bound_from_frames(kfs, 1, stride=stride)
    assert (planes[:, 3] < p1[:, 3]).all()
