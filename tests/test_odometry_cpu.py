"""CPU checks of the depth odometry's twins (tests/odometry_cases.py), of its host-side code (twists, the
trajectory log, tools/prep_own_data.py on a folder that already has a mesh) and of the three entry points'
argument checks.  No GPU.  The float32 floors and the twin's drift are printed (pytest -s shows them)."""
import ctypes
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import odometry_cases as oc
import tsdf_cases as tc
from conftest import GOLDEN, REPO


def _tool():
    spec = importlib.util.spec_from_file_location("prep_own_data", os.path.join(REPO, "tools", "prep_own_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def frs():
    return oc.frames()


@pytest.fixture(scope="module")
def corner(frs):
    """Three frames of the trajectory fused by tsdf_cases.fuse_f32 at the true poses."""
    lo, hi = oc.box()
    est = [SimpleNamespace(depth=f.depth, color=f.color, c2w=f.c2w) for f in frs[:3]]
    with oc.camera():
        v = tc.fuse_f32(est, lo, hi, calls=[[0], [1], [2]], color=False)
    return oc.volume_arrays(v.table, lo, hi, v.tsdf, v.weight)


def _outside(a, b, margin):
    """max |a - b| over the pixels outside the margin, which must agree on validity there."""
    va, vb = ~np.isnan(a).any(-1), ~np.isnan(b).any(-1)
    assert ((va == vb) | margin).all()
    keep = va & vb & ~margin
    return float(np.abs(a[keep].astype(np.float64) - b[keep]).max()) if keep.any() else 0.0


def test_depth_map_twins_agree_and_their_floors(frs):
    for name, depth in (("frame", frs[0].depth), ("holes", oc.holes(frs[5].depth)), ("5x7", oc.holes(frs[0].depth[:5, :7])),
                        ("1x1", frs[0].depth[:1, :1])):
        ref, f32 = oc.depth_maps_ref(depth), oc.depth_maps_f32(depth)
        assert ref.margin.mean() <= oc.MARGIN_CAP, name
        fv, fn = _outside(f32.vertex, ref.vertex, ref.margin), _outside(f32.normal, ref.normal, ref.margin)
        print(f"depth_maps {name}: float32 floor vertex {fv:.3e} normal {fn:.3e}, "
              f"{int((~np.isnan(ref.normal).any(-1)).sum())} normals, {int(ref.margin.sum())} margin pixels")
        assert fv < 1e-6 and fn < 1e-4, name
        assert np.isnan(ref.normal[-1]).all() and np.isnan(ref.normal[:, -1]).all()
    h = oc.depth_maps_ref(oc.holes(frs[5].depth))
    assert np.isnan(h.vertex[1, 2]).all() and np.isnan(h.vertex[2, 4]).all() and np.isnan(h.vertex[3, 1]).all()
    assert np.isnan(h.normal[0, 4]).all() and not np.isnan(h.normal[4, 2]).any()   # just over / just under max_jump


def test_raycast_twins_agree_and_their_floors(frs, corner):
    for k in (0, 2, 7):
        ref, f32 = oc.raycast_ref(corner, frs[k].c2w), oc.raycast_f32(corner, frs[k].c2w)
        assert ref.margin.mean() <= oc.MARGIN_CAP
        assert ((ref.hit == f32.hit) | ref.margin).all()
        fv, fn = _outside(f32.vertex, ref.vertex, ref.margin), _outside(f32.normal, ref.normal, ref.margin)
        print(f"raycast from pose {k}: float32 floor vertex {fv:.3e} normal {fn:.3e}, {int(ref.hit.sum())} hits, "
              f"{int(ref.margin.sum())} margin pixels, {ref.samples} samples")
        assert ref.hit.sum() > 2000 and fv < 1e-4 and fn < 1e-2
        assert np.abs(np.linalg.norm(ref.normal[ref.hit], axis=-1) - 1.0).max() < 1e-12


def test_raycast_hits_the_wall_and_the_corner(frs, corner):
    frames, (n, c) = tc.wall_scene()
    lo, hi, _ = tc.block_range(frames)
    v = tc.fuse_ref(frames, lo, hi)
    r = oc.raycast_ref(oc.volume_arrays(v.table, lo, hi, v.tsdf, v.weight), frames[0].c2w, cam=tc.CAM)
    off = np.abs(r.vertex[r.hit] @ n - c)
    print(f"wall: {int(r.hit.sum())} hits, median distance to the plane {np.median(off):.3e}")
    assert r.hit.sum() > 0.5 * r.hit.size and np.median(off) < oc.L
    assert (r.normal[r.hit] @ n < -0.9).all()          # toward the camera: the free side
    # the corner against the analytic depth
    k = 2
    r = oc.raycast_ref(corner, frs[k].c2w)
    w2c = np.linalg.inv(frs[k].c2w)
    z = (r.vertex @ w2c[:3, :3].T + w2c[:3, 3])[..., 2]
    truth = oc.cast(oc.trajectory()[k])
    err = np.abs(z - truth)[r.hit]
    print(f"corner: {int(r.hit.sum())} hits, median |z - analytic| {np.median(err):.3e}")
    assert np.median(err) < oc.L


def test_raycast_misses(frs, corner):
    away = frs[0].c2w @ np.diag([-1.0, 1.0, -1.0, 1.0])        # turned about its y axis: the room behind it
    assert not oc.raycast_ref(corner, away).hit.any()
    far_off = frs[0].c2w.copy()
    far_off[:3, 3] += 40.0                                       # outside the table
    assert not oc.raycast_ref(corner, far_off).hit.any()
    lo, hi = oc.box()
    empty = oc.volume_arrays(np.full(int(np.prod(np.subtract(hi, lo))), -1), lo, hi, np.zeros((0, 4096)),
                             np.zeros((0, 4096)))
    assert not oc.raycast_f32(empty, frs[0].c2w).hit.any()
    bad = frs[0].c2w.copy()
    bad[0, 3] = np.nan
    assert not oc.raycast_f32(corner, bad).hit.any()


def test_icp_sums_twin(frs, corner):
    src = oc.depth_maps_f32(frs[3].depth)
    model = oc.raycast_f32(corner, frs[2].c2w)
    w2c = np.linalg.inv(frs[2].c2w)
    od = oc._od()
    for stride in (1, 2, 4):
        s = oc.icp_sums_ref(src.vertex, src.normal, frs[3].c2w, model.vertex, model.normal, w2c, stride)
        assert s.margin.sum() <= oc.MARGIN_CAP * s.n_terms
        assert s.sums[28] == s.accept.sum() > 0.7 * (~np.isnan(src.normal[::stride, ::stride]).any(-1)).sum()
        A, b, rr, n = od.normal_equations(s.sums)
        assert np.allclose(A, A.T) and np.linalg.eigvalsh(A).min() > 0 and n == s.accept.sum()
    moved = od.se3_exp([0.012, 0.0, 0.0, 0.02, 0.0, 0.0]) @ frs[3].c2w      # 0.7 degrees and 2 cm
    t = oc.icp_sums_ref(src.vertex, src.normal, moved, model.vertex, model.normal, w2c, 1)
    assert (t.accept != s.accept).any()
    none = oc.icp_sums_ref(np.full_like(src.vertex, np.nan), src.normal, frs[3].c2w, model.vertex, model.normal, w2c, 1)
    assert (none.sums == 0).all()


def test_track_ref_converges(frs):
    res = oc.track_ref(frs)
    for k, r in enumerate(res[1:], 1):
        dt, dr = oc.pose_error(r["c2w"], frs[k].c2w)
        print(f"track_ref frame {k}: inliers {r['inliers']} of {r['valid']} ({100.0 * r['inliers'] / r['valid']:.1f} %), "
              f"cond {r['cond']:.1f}, rms {r['rms']:.2e}, drift {1e3 * dt:.2f} mm {dr:.3f} deg")
        assert not r["lost"] and r["cond"] < 100.0 and r["inliers"] > 0.8 * r["valid"], k
    dt, dr = oc.pose_error(res[-1]["c2w"], frs[-1].c2w)
    assert dt < 0.02 and dr < 1.0      # a step of the trajectory: the tracker follows it


def test_twist_round_trip():
    od = oc._od()
    rng = np.random.default_rng(5)
    for xi in [np.zeros(6), oc.twist(3), np.array([1e-10, 0, 0, 0.3, -0.2, 0.1]), *rng.uniform(-1.0, 1.0, (6, 6))]:
        T = od.se3_exp(xi)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14) and np.linalg.det(T[:3, :3]) > 0
        assert np.allclose(od.se3_log(T), xi, atol=1e-12)
        assert np.allclose(od.se3_exp(-np.asarray(xi)) @ T, np.eye(4), atol=1e-14)
    poses = [np.eye(4), od.se3_exp(oc.twist(1))]
    assert np.allclose(od.predict(poses), od.se3_exp(oc.twist(1)) @ od.se3_exp(oc.twist(1)))
    assert np.allclose(od.predict(poses[:1]), np.eye(4))


def test_trajectory_log_is_what_the_azure_loader_reads(pkg, tmp_path):
    poses = oc.relative(oc.trajectory(4))
    path = tmp_path / "trajectory.log"
    pkg.odometry.write_trajectory_log(str(path), poses)
    assert len(path.read_text().splitlines()) == 5 * len(poses)
    ds = SimpleNamespace(n_img=len(poses))
    pkg.datasets.Azure.load_poses(ds, str(path))
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    assert len(ds.poses) == len(poses)
    for got, want in zip(ds.poses, poses):
        assert np.allclose(got.numpy(), (want @ flip).astype(np.float32), atol=1e-7)
    assert np.array_equal(ds.poses[0].numpy(), flip.astype(np.float32))


def _scene_with_ply(pkg, folder):
    os.makedirs(folder / "scene")
    (folder / "intrinsic.json").write_text(json.dumps(
        {"width": 64, "height": 48, "intrinsic_matrix": [30.0, 0.0, 0.0, 0.0, 31.0, 0.0, 31.5, 23.5, 1.0]}))
    v = np.array([[-1.25, 0.5, 2.0], [0.75, -0.5, 3.5], [0.25, 1.5, 0.00001]], dtype=np.float32)
    pkg.mesher.write_ply(str(folder / "scene" / "integrated.ply"), v, np.array([[0, 1, 2]], dtype=np.int32))
    return v.astype(np.float64)


def test_prep_own_data_with_an_existing_mesh(pkg, tmp_path):
    folder = tmp_path / "my scene"
    v = _scene_with_ply(pkg, folder)
    before = {f: (folder / "scene" / f).read_bytes() for f in os.listdir(folder / "scene")}
    base = os.path.join(GOLDEN, "configs", "own.yaml")
    tool = _tool()
    for flag in ("--output_config", "--ouput_config"):
        out = tmp_path / f"cfg{flag[3]}.yaml"
        assert tool.main(["--scene_folder", str(folder), flag, str(out), "--base", base]) == 0
        assert "\t" not in out.read_text()
        cfg = pkg.config.load_config(str(out), os.path.join(GOLDEN, "configs", "nice_slam.yaml"))
        want = np.stack([v.min(0) - 1.0, v.max(0) + 1.0], 1)
        for key in ("bound", "marching_cubes_bound"):
            assert np.allclose(np.array(cfg["mapping"][key], dtype=np.float64), want, atol=1e-12), key
        assert cfg["cam"]["H"] == 48 and cfg["cam"]["W"] == 64
        assert (cfg["cam"]["fx"], cfg["cam"]["fy"], cfg["cam"]["cx"], cfg["cam"]["cy"]) == (30.0, 31.0, 31.5, 23.5)
        assert cfg["cam"]["png_depth_scale"] == 1000.0 and cfg["dataset"] == "azure"      # from the base
        assert cfg["mapping"]["every_frame"] == 5 and cfg["inherit_from"] == base
        assert cfg["data"]["input_folder"] == str(folder) and cfg["data"]["output"] == "output/Own/my scene"
    assert {f: (folder / "scene" / f).read_bytes() for f in os.listdir(folder / "scene")} == before
    # the default base is the reference's path
    out = tmp_path / "default.yaml"
    assert tool.main(["--scene_folder", str(folder), "--output_config", str(out)]) == 0
    import yaml
    assert yaml.safe_load(out.read_text())["inherit_from"] == "configs/Own/own.yaml"


def test_prep_own_data_does_not_overwrite_a_log(pkg, tmp_path):
    folder = tmp_path / "s"
    _scene_with_ply(pkg, folder)
    os.remove(folder / "scene" / "integrated.ply")
    (folder / "scene" / "trajectory.log").write_text("0 0 1\n")
    with pytest.raises(SystemExit, match="--force"):
        _tool().main(["--scene_folder", str(folder), "--output_config", str(tmp_path / "c.yaml")])
    assert (folder / "scene" / "trajectory.log").read_text() == "0 0 1\n"


def test_odometry_entry_points_validate_without_gpu(pkg):
    """nslam_depth_maps, nslam_tsdf_raycast and nslam_icp_sums return their documented codes before any device
    call (fake aligned pointers, never dereferenced)."""
    L = pkg._lib.lib()
    P = 4096
    assert L.nslam_depth_maps(None, 4, 4, 1.0, 1.0, 0.0, 0.0, 5.0, 0.1, P, P, None) == -1        # no depth
    assert L.nslam_depth_maps(P, 4, 4, 1.0, 1.0, 0.0, 0.0, 5.0, 0.1, P, None, None) == -1        # no normal map
    assert L.nslam_depth_maps(P, 0, 4, 1.0, 1.0, 0.0, 0.0, 5.0, 0.1, P, P, None) == -1           # empty image
    assert L.nslam_depth_maps(P, 4, 4, 0.0, 1.0, 0.0, 0.0, 5.0, 0.1, P, P, None) == -1           # fx == 0
    assert L.nslam_depth_maps(P, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.0, 0.1, P, P, None) == -1           # depth_trunc
    assert L.nslam_depth_maps(P, 4, 4, 1.0, 1.0, 0.0, 0.0, 5.0, float("nan"), P, P, None) == -1  # max_jump
    assert L.nslam_depth_maps(P, 1 << 15, 1 << 15, 1.0, 1.0, 0.0, 0.0, 5.0, 0.1, P, P, None) == -2
    lo, hi = (ctypes.c_int32 * 3)(-2, -2, -2), (ctypes.c_int32 * 3)(2, 2, 2)
    eye = (ctypes.c_double * 16)(*np.eye(4).ravel())

    def cast(**k):
        a = dict(table=P, key=P, tsdf=P, weight=P, n=3, lo=lo, hi=hi, voxel=0.04, trunc=0.12, c2w=eye, H=4, W=4,
                 fx=1.0, near=0.0, far=5.0, vertex=P)
        a.update(k)
        return L.nslam_tsdf_raycast(a["table"], a["key"], a["tsdf"], a["weight"], a["n"], a["lo"], a["hi"], a["voxel"],
                                    a["trunc"], a["c2w"], a["H"], a["W"], a["fx"], 1.0, 0.0, 0.0, a["near"], a["far"],
                                    a["vertex"], P, None)
    assert cast(table=None) == -1
    assert cast(tsdf=None) == -1                     # a pool without its arrays
    assert cast(c2w=None) == -1
    assert cast(vertex=None) == -1
    assert cast(n=-1) == -1
    assert cast(H=0) == -1
    assert cast(fx=0.0) == -1
    assert cast(voxel=0.0) == -1
    assert cast(trunc=0.5) == -1                     # 2 trunc > 16 voxel
    assert cast(near=-1.0) == -1
    assert cast(far=0.0) == -1                       # far <= near
    assert cast(far=float("inf")) == -1
    assert cast(hi=(ctypes.c_int32 * 3)(2, -2, 2)) == -1   # an empty box
    assert cast(n=1 << 18) == -2                     # 3 * 4096 * n_pool >= 2^31
    assert cast(H=1 << 15, W=1 << 15) == -2

    def icp(**k):
        a = dict(sv=P, sn=P, Hs=8, Ws=8, stride=2, T=eye, mv=P, mn=P, Hm=8, Wm=8, w2c=eye, fx=1.0, dist=0.1, cos=0.8,
                 partial=P, n_partial=1, out=P)
        a.update(k)
        return L.nslam_icp_sums(a["sv"], a["sn"], a["Hs"], a["Ws"], a["stride"], a["T"], a["mv"], a["mn"], a["Hm"],
                                a["Wm"], a["w2c"], a["fx"], 1.0, 0.0, 0.0, a["dist"], a["cos"], a["partial"],
                                a["n_partial"], a["out"], None, None)
    assert L.nslam_icp_partials(8, 8, 2) == 1 and L.nslam_icp_partials(47, 63, 1) == 12
    assert L.nslam_icp_partials(720, 1280, 1) == 1024 and L.nslam_icp_partials(0, 8, 1) == 0
    for name in ("sv", "sn", "mv", "mn", "T", "w2c", "out", "partial"):
        assert icp(**{name: None}) == -1, name
    assert icp(stride=0) == -1
    assert icp(Hm=0) == -1
    assert icp(fx=0.0) == -1
    assert icp(dist=-1.0) == -1
    assert icp(cos=1.5) == -1
    nan = (ctypes.c_double * 16)(*([float("nan")] + [0.0] * 15))
    assert icp(T=nan) == -1                          # an estimate that is not finite
    assert icp(n_partial=0) == -3
    assert icp(Hs=1 << 15, Ws=1 << 15, n_partial=1 << 20) == -2
    import torch
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.depth_maps(torch.zeros(4, 4), 1.0, 1.0, 0.0, 0.0, 5.0, 0.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.icp_sums(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3), np.eye(4), torch.zeros(4, 4, 3),
                         torch.zeros(4, 4, 3), np.eye(4), 1.0, 1.0, 0.0, 0.0, 1, 0.1, 0.8)
