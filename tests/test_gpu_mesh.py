"""GPU tests of the mesher (csrc/nslam_mesh.hip, nice-slam_amd/mesher.py): point masks against the reference's
recording, marching cubes against topological and geometric invariants, cleaning, and get_mesh end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, grids_from, sd_from

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

DEV = "cuda:0"


@pytest.fixture(scope="module")
def mesh_fix():
    with np.load(os.path.join(GOLDEN, "mesh_fixtures.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def _mask_mesher(pkg, depth_test, batch):
    import torch

    import mesh_scene
    cfg = {"coarse": True, "scale": 1, "occupancy": True,
           "meshing": {"resolution": 8, "level_set": 0, "clean_mesh_bound_scale": 1.02,
                       "remove_small_geometry_threshold": 0.2, "color_mesh_extraction_method": "direct_point_query",
                       "get_largest_components": False, "depth_test": depth_test},
           "mapping": {"marching_cubes_bound": mesh_scene.MC_BOUND}}
    slam = SimpleNamespace(renderer=None, bound=torch.tensor(mesh_scene.MC_BOUND, dtype=torch.float64), nice=True,
                           verbose=False, **mesh_scene.CAM)
    return pkg.Mesher(cfg, None, slam, points_batch_size=batch)


@pytest.fixture(scope="module")
def mask_runs(pkg):
    """Our masks for the five recorded cases (computed once)."""
    import torch

    import mesh_scene
    pts, poses, depths = mesh_scene.mask_scene()
    kfs = [{"est_c2w": torch.from_numpy(p), "depth": torch.from_numpy(d)} for p, d in zip(poses, depths)]
    c2w_list = torch.from_numpy(np.stack(poses, 0))
    cases = {"dt1_b1024": (True, mesh_scene.BATCH, False), "dt1_b4096": (True, mesh_scene.N_POINTS, False),
             "dt0_b1024": (False, mesh_scene.BATCH, False), "dt0_b4096": (False, mesh_scene.N_POINTS, False),
             "all_b1024": (True, mesh_scene.BATCH, True)}
    out = {}
    for name, (dt, batch, use_all) in cases.items():
        m = _mask_mesher(pkg, dt, batch)
        s, f, u = m.point_masks(torch.from_numpy(pts), kfs, c2w_list, len(poses) - 1, DEV,
                                get_mask_use_all_frames=use_all)
        margin, _ = mesh_scene.mask_margins(pts, poses, depths, dt, use_all, batch)
        out[name] = (np.stack([s, f, u], 0), margin)
    return out


@pytest.mark.parametrize("case", ["dt1_b1024", "dt1_b4096", "dt0_b1024", "dt0_b4096", "all_b1024"])
def test_point_masks_match_reference(mask_runs, mesh_fix, case):
    import mesh_scene
    got, margin = mask_runs[case]
    ref = mesh_fix["masks." + case].astype(bool)
    cmp = margin >= mesh_scene.MARGIN
    left_out = 1.0 - cmp.mean()
    bad = (got != ref).any(0)
    print(f"{case}: left out {left_out:.4f}, mismatches {int(bad.sum())} (compared {int((bad & cmp).sum())}), "
          f"seen {int(got[0].sum())} forecast {int(got[1].sum())} unseen {int(got[2].sum())}")
    assert left_out <= mesh_scene.MAX_LEFT_OUT
    assert got.dtype == bool and got.shape == ref.shape
    assert (got.sum(0) == 1).all()                     # the three masks partition the points
    assert not (bad & cmp).any()


def test_point_masks_depend_on_the_chunking(mask_runs):
    """depth_test bounds the forecast depth by the largest sample of the point's own chunk (Mesher.py:166):
    one chunk of 4096 and four of 1024 must differ, which a kernel without the per-chunk pass could not show."""
    assert (mask_runs["dt1_b1024"][0] != mask_runs["dt1_b4096"][0]).any()
    assert (mask_runs["dt0_b1024"][0] == mask_runs["dt0_b4096"][0]).all()


# ------------------------------------------------------------------------------------------------
# marching cubes
# ------------------------------------------------------------------------------------------------
SHAPE = (24, 20, 28)  # non-cubic on purpose
ORIGIN = (0.5, -1.0, 2.0)
SPACING = (0.1, 0.15, 0.2)
SPHERES = (((7.3, 9.6, 8.4), 6.0), ((18.2, 9.4, 21.6), 3.0))


def _idx():
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE], indexing="ij")


def _sphere_field(spheres):
    i, j, k = _idx()
    f = np.full(SHAPE, -np.inf)
    for (cx, cy, cz), r in spheres:
        f = np.maximum(f, r - np.sqrt((i - cx) ** 2 + (j - cy) ** 2 + (k - cz) ** 2))
    return f.astype(np.float32)


def _torus_field():
    i, j, k = _idx()
    ring = np.sqrt((i - 11.4) ** 2 + (j - 9.6) ** 2) - 6.0
    return (2.5 - np.sqrt(ring ** 2 + (k - 13.3) ** 2)).astype(np.float32)


FIELDS = {"sphere": (lambda: _sphere_field((((11.3, 9.6, 13.4), 8.0),)), 2),
          "torus": (_torus_field, 0),
          "two_spheres": (lambda: _sphere_field(SPHERES), 4)}


def _mc(pkg, vol, level, origin=ORIGIN, spacing=SPACING):
    import torch
    v, f = pkg.ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level, origin, spacing)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


def _expected_vertices(vol, level, origin, spacing):
    """Owner-edge order: lattice points in C order, their +x, +y, +z edges; float64 interpolation."""
    lv = np.float32(level)
    below = vol < lv
    n = vol.size
    flags = np.zeros(vol.shape + (3,), dtype=bool)
    pos = np.zeros(vol.shape + (3, 3))
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in vol.shape], indexing="ij"), -1)
    for ax in range(3):
        a = vol.astype(np.float64)
        b = np.roll(a, -1, axis=ax)
        cross = below != np.roll(below, -1, axis=ax)
        sl = [slice(None)] * 3
        sl[ax] = -1
        cross[tuple(sl)] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (np.float64(lv) - a) / (b - a)
        p = idx.copy()
        p[..., ax] += np.where(cross, t, 0.0)
        flags[..., ax] = cross
        pos[..., ax, :] = np.asarray(origin) + p * np.asarray(spacing)
    flags = flags.reshape(n * 3)
    return pos.reshape(n * 3, 3)[flags], int(flags.sum())


def _directed(faces):
    f = faces.astype(np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def _signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def _canon_rows(f):
    k = np.argmin(f, 1)
    r = np.stack([np.roll(row, -s) for row, s in zip(f, k)], 0) if len(f) else f
    return r[np.lexsort(r.T[::-1])]


@pytest.fixture(scope="module")
def mc_runs(pkg):
    out = {}
    for name, (make, chi) in FIELDS.items():
        vol = make()
        out[name] = (vol, chi) + _mc(pkg, vol, 0.0)
    return out


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_cubes_surface(pkg, mc_runs, name):
    vol, chi, v, f = mc_runs[name]
    exp, n_exp = _expected_vertices(vol, 0.0, ORIGIN, SPACING)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert v.shape == (n_exp, 3) and n_exp > 100            # one vertex per straddling edge
    err = np.abs(v - exp) / np.asarray(SPACING)
    print(f"{name}: V {v.shape[0]} F {f.shape[0]} max vertex error {err.max():.2e} spacings")
    assert err.max() <= 1e-6
    assert f.min() == 0 and f.max() == n_exp - 1
    d = _directed(f)
    key = d[:, 0] * n_exp + d[:, 1]
    assert np.unique(key).size == key.size                    # no directed edge twice
    rev = d[:, 1] * n_exp + d[:, 0]
    assert np.array_equal(np.sort(key), np.sort(rev))         # every edge once in each direction: two faces
    n_edges = key.size // 2
    assert v.shape[0] - n_edges + f.shape[0] == chi           # Euler characteristic
    vol_signed = _signed_volume(v, f)
    inside = vol >= np.float32(0.0)
    cells_all = np.ones(tuple(s - 1 for s in SHAPE), dtype=bool)
    cells_any = np.zeros_like(cells_all)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = inside[dx:SHAPE[0] - 1 + dx, dy:SHAPE[1] - 1 + dy, dz:SHAPE[2] - 1 + dz]
                cells_all &= c
                cells_any |= c
    cell = float(np.prod(SPACING))
    print(f"{name}: signed volume {vol_signed:.6f} in [{cells_all.sum() * cell:.6f}, {cells_any.sum() * cell:.6f}]")
    assert vol_signed > 0                                      # normals point out of the high (occupied) side
    assert cells_all.sum() * cell <= vol_signed <= cells_any.sum() * cell
    # the negated field at the negated level: the same vertices, every face flipped
    v2, f2 = _mc(pkg, -vol, -0.0)
    assert np.array_equal(v2, v)
    assert np.array_equal(_canon_rows(f2[:, ::-1]), _canon_rows(f))


def test_marching_cubes_random_field_is_closed_and_deterministic(pkg):
    rng = np.random.default_rng(3)
    vol = np.full((12, 10, 14), -1.0, dtype=np.float32)
    vol[1:-1, 1:-1, 1:-1] = (rng.random((10, 8, 12)) - 0.5).astype(np.float32)
    v, f = _mc(pkg, vol, 0.0)
    exp, n_exp = _expected_vertices(vol, 0.0, ORIGIN, SPACING)
    assert v.shape[0] == n_exp and f.shape[0] > 500
    assert (np.abs(v - exp) / np.asarray(SPACING)).max() <= 1e-6
    d = _directed(f)
    key, rev = d[:, 0] * n_exp + d[:, 1], d[:, 1] * n_exp + d[:, 0]
    assert np.unique(key).size == key.size                    # no directed edge twice (ambiguous faces included)
    assert np.array_equal(np.sort(key), np.sort(rev))         # a -> b as often as b -> a: closed
    v2, f2 = _mc(pkg, vol, 0.0)
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()


def test_marching_cubes_no_crossing(pkg):
    v, f = _mc(pkg, np.ones((6, 5, 7), dtype=np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


# ------------------------------------------------------------------------------------------------
# cleaning
# ------------------------------------------------------------------------------------------------
def _areas(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)


def test_components_and_cull(pkg, mc_runs):
    import torch
    ops = pkg.ops
    _, _, v, f = mc_runs["two_spheres"]
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    split = ORIGIN[2] + 16.5 * SPACING[2]                      # between the two spheres along z
    big_v = v[:, 2] < split
    big_f = big_v[f[:, 0]]
    assert (big_v[f] == big_f[:, None]).all()
    fa = _areas(v, f)
    a_big, a_small = fa[big_f].sum(), fa[~big_f].sum()
    assert a_big > 3 * a_small > 0

    label, area = ops.mesh_components(tv, tf)
    label, area = label.cpu().numpy(), area.cpu().numpy()
    l_big, l_small = np.flatnonzero(big_v).min(), np.flatnonzero(~big_v).min()
    assert (label[big_v] == l_big).all() and (label[~big_v] == l_small).all()
    print(f"areas: {area[l_big]:.9f} vs {a_big:.9f}, {area[l_small]:.9f} vs {a_small:.9f}")
    assert abs(area[l_big] - a_big) <= 1e-9 * a_big and abs(area[l_small] - a_small) <= 1e-9 * a_small
    assert np.count_nonzero(area) == 2

    def check(kv, kf, ids, want_v, want_f):
        kv, kf, ids = kv.cpu().numpy(), kf.cpu().numpy(), ids.cpu().numpy()
        assert np.array_equal(ids, np.flatnonzero(want_v)) and np.array_equal(kv, v[want_v])
        assert kf.dtype == np.int32 and np.array_equal(kv[kf], v[f[want_f]])   # same triangles, same order

    thr = float(np.sqrt(a_big * a_small))                      # a factor > 1.7 from either area
    assert a_big > 1.7 * thr and thr > 1.7 * a_small
    check(*ops.mesh_keep_components(tv, tf, True), big_v, big_f)
    check(*ops.mesh_keep_components(tv, tf, False, thr), big_v, big_f)
    check(*ops.mesh_keep_components(tv, tf, False, a_small / 2), np.ones_like(big_v), np.ones_like(big_f))
    kv, kf, _ = ops.mesh_keep_components(tv, tf, False, 2 * a_big)
    assert kv.shape[0] == 0 and kf.shape[0] == 0

    # cull: faces with all three vertices masked go
    rng = np.random.default_rng(1)
    vmask = rng.random(v.shape[0]) < 0.6
    keep = ops.mesh_face_cull(tf, torch.from_numpy(vmask).to(DEV)).cpu().numpy()
    assert np.array_equal(keep, ~vmask[f].all(1)) and 0 < keep.sum() < keep.size
    keep = ops.mesh_face_cull(tf, torch.from_numpy(big_v).to(DEV)).cpu().numpy()
    assert np.array_equal(keep, ~big_f)
    # the small sphere alone is the largest component of what is left
    kv, kf, _ = ops.mesh_keep_components(tv, tf[torch.from_numpy(keep).to(DEV)].contiguous(), True)
    assert np.array_equal(kv.cpu().numpy(), v[~big_v]) and kf.shape[0] == int((~big_f).sum())


def test_points_in_hull(pkg):
    import torch
    rng = np.random.default_rng(2)
    planes = pkg.mesher.box_planes((0.0, -1.0, 0.5), (2.0, 1.0, 3.0))
    extra = np.array([[1.0, 1.0, 1.0, -3.5]]) / np.sqrt(3.0)   # one oblique cut
    planes = np.concatenate([planes, extra], 0)
    for dtype in (np.float32, np.float64):
        p = (rng.random((5000, 3)) * 4.0 - 1.0).astype(dtype)
        q = p.astype(np.float64)
        want = np.ones(p.shape[0], dtype=bool)
        for pl in planes:
            want &= ((pl[0] * q[:, 0] + pl[1] * q[:, 1]) + pl[2] * q[:, 2]) + pl[3] <= 0.0
        got = pkg.ops.points_in_hull(torch.from_numpy(p).to(DEV), torch.from_numpy(planes).to(DEV)).cpu().numpy()
        assert np.array_equal(got, want) and 0 < want.sum() < want.size


# ------------------------------------------------------------------------------------------------
# get_mesh end to end on the tiny scene
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_mesher(pkg, tiny):
    import torch

    import scenes
    dev = torch.device(DEV)
    scale = 0.5
    bound = torch.from_numpy(tiny["bound"])
    nice = pkg.NICE(c_dim=32, coarse_grid_len=2.0, middle_grid_len=0.64, fine_grid_len=0.32, color_grid_len=0.32,
                    hidden_size=32, coarse=True)
    nice.load_state_dict(sd_from(tiny))
    nice.set_bound(bound)
    nice = nice.to(dev)
    c = {k: v.to(dev).contiguous(memory_format=torch.channels_last_3d) for k, v in grids_from(tiny).items()}
    cam = scenes.TINY_CAM
    cfg = {"rendering": {"N_samples": 32, "N_surface": 16, "N_importance": 0, "lindisp": False, "perturb": 0.0},
           "occupancy": True, "coarse": True, "scale": scale,
           "meshing": {"resolution": 32, "level_set": 0.0, "clean_mesh_bound_scale": 1.02,
                       "remove_small_geometry_threshold": 0.002, "color_mesh_extraction_method": "direct_point_query",
                       "get_largest_components": False, "depth_test": True},
           # multiplied by scale inside the mesher: the lattice covers the tiny bound itself
           "mapping": {"marching_cubes_bound": (np.array(scenes.TINY_BOUND) / scale).tolist()}}
    slam = SimpleNamespace(nice=True, bound=bound, verbose=False, **cam)
    slam.renderer = pkg.Renderer(cfg, None, slam)
    m = pkg.Mesher(cfg, None, slam, points_batch_size=8192)
    b, poses, _ = scenes.tiny_window(3)
    kfs = [{"est_c2w": torch.from_numpy(p), "depth": torch.from_numpy(scenes.box_depth(p, cam, b, seed=40 + k))}
           for k, p in enumerate(poses)]
    c2w_list = torch.from_numpy(np.stack(poses, 0))
    tb = np.array(scenes.TINY_BOUND)
    planes = pkg.mesher.box_planes(tb[:, 0] + 0.25, tb[:, 1] - 0.25)
    # a level that the fine field crosses inside the box: its median there
    pts = m.get_grid_uniform(32)["grid_points"].to(dev).contiguous()
    inside = pkg.ops.points_in_hull(pts, torch.from_numpy(planes).to(dev))
    with torch.no_grad():
        m.level_set = float(m.eval_points(pts[inside], nice, c, "fine", dev)[:, -1].median())
    return SimpleNamespace(m=m, nice=nice, c=c, kfs=kfs, c2w_list=c2w_list, planes=planes, scale=scale, dev=dev)


@pytest.mark.parametrize("show_forecast", [False, True])
def test_get_mesh_end_to_end(pkg, tiny_mesher, tmp_path, show_forecast):
    import torch
    t = tiny_mesher
    m = t.m
    m.get_largest_components = not show_forecast          # one branch each: largest / area threshold
    path = str(tmp_path / f"mesh_{int(show_forecast)}.ply")
    m.get_mesh(path, t.c, t.nice, t.kfs, t.c2w_list, 2, t.dev, show_forecast=show_forecast, mesh_bound=t.planes)
    assert os.path.exists(path)
    got = pkg.mesher.read_ply(path)
    last = m.last_mesh
    lv, faces = last["lattice_vertices"], last["faces"]
    print(f"show_forecast={show_forecast}: level {m.level_set:.4f} V {lv.shape[0]} F {faces.shape[0]}")
    assert faces.shape[0] > 0 and got["faces"].shape == tuple(faces.shape)
    assert np.array_equal(got["faces"], faces.cpu().numpy())
    assert np.array_equal(np.unique(got["faces"]), np.arange(lv.shape[0]))      # compacted: every vertex used
    # vertices: the lattice-space vertices divided by scale, stored as float32
    assert np.array_equal(got["vertices"], (lv.cpu().numpy() / t.scale).astype(np.float32))
    f64 = faces.long()
    if show_forecast:
        ok = pkg.ops.points_in_hull(lv.contiguous(), torch.from_numpy(t.planes).to(t.dev))
    else:
        ok = m.point_masks_device(lv, t.kfs, t.c2w_list, 2, t.dev)[0]
    assert bool(ok[f64].any(1).all())                      # every kept face has a contained / seen vertex
    print(f"vertices contained / seen: {int(ok.sum())} of {ok.shape[0]}")
    # colours: clip(0, 1) * 255 of the colour stage at the written (lattice-space) vertices
    with torch.no_grad():
        rgb = t.m.renderer.eval_points(lv.float(), t.nice, t.c, "color", t.dev)[:, :3]
        want = (torch.clamp(rgb, 0, 1) * 255).cpu().numpy()
    col = got["colors"].astype(np.float64)
    assert (col[:, 3] == 255).all()
    plain = np.ones(lv.shape[0], dtype=bool)
    if show_forecast:
        fc = m.point_masks_device(lv, t.kfs, t.c2w_list, 2, t.dev)[1].cpu().numpy()
        assert (got["colors"][fc, :3] == np.array([0, 255, 255])).all()
        plain = ~fc
    assert plain.any()
    assert (np.abs(col[plain, :3] - np.floor(want[plain])) <= 1).all()


def test_get_mesh_without_a_crossing_writes_nothing(pkg, tiny_mesher, tmp_path, capsys):
    t = tiny_mesher
    level = t.m.level_set
    try:
        t.m.level_set = 1e6                                # above every logit (outside the hull is 100)
        path = str(tmp_path / "none.ply")
        assert t.m.get_mesh(path, t.c, t.nice, t.kfs, t.c2w_list, 2, t.dev, mesh_bound=t.planes) is None
        assert not os.path.exists(path)
        assert "no surface" in capsys.readouterr().out.lower()
    finally:
        t.m.level_set = level
