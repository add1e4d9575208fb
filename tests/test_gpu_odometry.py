"""GPU tests of the depth odometry (csrc/nslam_odometry.hip, nice-slam_amd/odometry.py) against the numpy twins of
tests/odometry_cases.py: depth maps, the volume's ray cast, the ICP sums, the tracker on the 13-frame trajectory,
its failure handling, and tools/prep_own_data.py end to end.  Floors are the float32 twin's own distance to the
float64 twin on the same input; the device is held to twice that."""
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import odometry_cases as oc
import tsdf_cases as tc
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = oc.CAM
INTR = (K["fx"], K["fy"], K["cx"], K["cy"])
FAR = 8.0


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _valid(a):
    return ~np.isnan(a).any(-1)


def _floor(f32, ref, margin):
    keep = _valid(f32) & _valid(ref) & ~margin
    return float(np.abs(f32[keep].astype(np.float64) - ref[keep]).max()) if keep.any() else 0.0


def _within(got, ref, margin, floor, what):
    assert ((_valid(got) == _valid(ref)) | margin).all(), what
    keep = _valid(got) & _valid(ref) & ~margin
    err = float(np.abs(got[keep].astype(np.float64) - ref[keep]).max()) if keep.any() else 0.0
    print(f"{what}: device - float64 twin {err:.3e}, float32 floor {floor:.3e}")
    assert err <= 2.0 * floor, what


@pytest.fixture(scope="module")
def frs():
    return oc.frames()


def gpu_volume(pkg, frames, lo, hi, cam=K):
    import torch
    vol = pkg.tsdf.TSDFVolume(oc.L, oc.TRUNC, lo, hi, DEV, color=False, depth_stride=tc.STRIDE,
                              depth_trunc=oc.DEPTH_TRUNC)
    for f in frames:
        vol.integrate(_dev(f.depth[None]), None, f.c2w[None], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    torch.cuda.synchronize()
    arrays = oc.volume_arrays(vol.table.cpu().numpy(), lo, hi, vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy())
    return vol, arrays


@pytest.fixture(scope="module")
def volumes(pkg, frs):
    lo, hi = oc.box()
    return {n: gpu_volume(pkg, frs[:n], lo, hi) for n in (3, 13)}


# ------------------------------------------------------------------------------------------------
# depth maps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["48x64", "holes", "5x7", "1x1"])
def test_depth_maps_match_the_twins(pkg, frs, case):
    depth = {"48x64": frs[0].depth, "holes": oc.holes(frs[5].depth), "5x7": oc.holes(frs[0].depth[:5, :7]),
             "1x1": frs[0].depth[:1, :1]}[case]
    ref, f32 = oc.depth_maps_ref(depth), oc.depth_maps_f32(depth)
    v, n = pkg.ops.depth_maps(_dev(depth), *INTR, oc.DEPTH_TRUNC, oc.MAX_JUMP)
    v, n = v.cpu().numpy(), n.cpu().numpy()
    assert v.shape == depth.shape + (3,) and np.array_equal(v, f32.vertex, equal_nan=True)
    _within(n, ref.normal, ref.margin, _floor(f32.normal, ref.normal, ref.margin), f"depth_maps {case} normal")
    assert np.isnan(n[-1]).all() and np.isnan(n[:, -1]).all()
    if case == "1x1":
        assert np.isnan(n).all() and not np.isnan(v).any()


# ------------------------------------------------------------------------------------------------
# ray cast
# ------------------------------------------------------------------------------------------------
def _check_cast(pkg, vol, arrays, c2w, cam, what):
    v, n = vol.raycast(c2w, cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], oc.NEAR, FAR)
    v2, n2 = vol.raycast(c2w, cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], oc.NEAR, FAR)
    v, n = v.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(v, v2.cpu().numpy(), equal_nan=True) and np.array_equal(n, n2.cpu().numpy(), equal_nan=True)
    ref = oc.raycast_ref(arrays, c2w, cam=cam, far=FAR)
    f32 = oc.raycast_f32(arrays, c2w, cam=cam, far=FAR)
    assert ref.margin.mean() <= oc.MARGIN_CAP and ref.hit.sum() > 0.5 * ref.hit.size
    assert ((_valid(v) == ref.hit) | ref.margin).all(), what
    _within(v, ref.vertex, ref.margin, _floor(f32.vertex, ref.vertex, ref.margin), what + " vertex")
    _within(n, ref.normal, ref.margin, _floor(f32.normal, ref.normal, ref.margin), what + " normal")


@pytest.mark.parametrize("n_frames,pose", [(3, 2), (13, 12), (13, 5)])
def test_raycast_of_the_corner_matches_the_twins(pkg, frs, volumes, n_frames, pose):
    vol, arrays = volumes[n_frames]
    _check_cast(pkg, vol, arrays, frs[pose].c2w, K, f"raycast corner {n_frames} frames, pose {pose}")


def test_raycast_of_the_wall_matches_the_twins(pkg):
    frames, (nrm, c) = tc.wall_scene()
    lo, hi, _ = tc.block_range(frames)
    vol, arrays = gpu_volume(pkg, frames, lo, hi, cam=tc.CAM)
    _check_cast(pkg, vol, arrays, frames[0].c2w, tc.CAM, "raycast wall")
    v, _ = vol.raycast(frames[0].c2w, tc.CAM["H"], tc.CAM["W"], tc.CAM["fx"], tc.CAM["fy"], tc.CAM["cx"], tc.CAM["cy"],
                       oc.NEAR, FAR)
    v = v.cpu().numpy()
    assert np.median(np.abs(v[_valid(v)] @ nrm - c)) < oc.L


def test_raycast_without_a_hit_returns(pkg, frs, volumes):
    import torch
    vol, _ = volumes[3]
    args = (K["H"], K["W"], *INTR, oc.NEAR, FAR)
    away = frs[0].c2w @ np.diag([-1.0, 1.0, -1.0, 1.0])          # the room behind the camera
    outside = frs[0].c2w.copy()
    outside[:3, 3] += 40.0                                         # far outside the table
    hole = away.copy()
    hole[:3, 3] = [0.0, 0.0, -2.0]                                 # inside the table, among unallocated blocks
    bad = frs[0].c2w.copy()
    bad[1, 3] = np.nan
    for name, pose in (("away", away), ("outside", outside), ("unallocated", hole), ("nan", bad)):
        v, n = vol.raycast(pose, *args)
        assert torch.isnan(v).all() and torch.isnan(n).all(), name
    lo, hi = oc.box()
    empty = pkg.tsdf.TSDFVolume(oc.L, oc.TRUNC, lo, hi, DEV, color=False)
    v, n = empty.raycast(frs[0].c2w, *args)
    assert v.shape == (K["H"], K["W"], 3) and torch.isnan(v).all() and torch.isnan(n).all()


# ------------------------------------------------------------------------------------------------
# ICP sums
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps(frs, volumes):
    """Source maps of frame 3 and model maps from pose 2 of the 3-frame volume (float32 twins)."""
    src = oc.depth_maps_f32(oc.holes(frs[3].depth))
    model = oc.raycast_f32(volumes[3][1], frs[2].c2w, far=FAR)
    return SimpleNamespace(sv=src.vertex, sn=src.normal, mv=model.vertex, mn=model.normal, w2c=np.linalg.inv(frs[2].c2w))


def _check_sums(pkg, sv, sn, T, m, stride):
    ref = oc.icp_sums_ref(sv, sn, T, m.mv, m.mn, m.w2c, stride)
    args = (_dev(sv), _dev(sn), T, _dev(m.mv), _dev(m.mn), m.w2c, *INTR, stride, oc.DIST_TH, oc.COS_TH)
    got, mask = pkg.ops.icp_sums(*args, return_mask=True)
    again = pkg.ops.icp_sums(*args)
    got, mask = got.cpu().numpy(), mask.cpu().numpy().astype(bool)
    assert np.array_equal(got.view(np.int64), again.cpu().numpy().view(np.int64))       # the same bits
    assert ref.margin.sum() <= oc.MARGIN_CAP * max(ref.n_terms, 100)
    same = bool((mask == ref.accept).all())
    assert same or ((mask == ref.accept) | ref.margin).all()
    assert abs(got[28] - ref.sums[28]) <= ref.margin.sum() and got[28] == mask.sum()
    print(f"icp_sums stride {stride}: {int(got[28])} inliers, {int(ref.margin.sum())} margin pixels, same set: {same}")
    if same:      # the same terms: only the order of the float64 additions differs
        bound = ref.n_terms * 2.0 ** -52 * ref.abs_sums[:28]
        assert (np.abs(got[:28] - ref.sums[:28]) <= bound).all(), np.abs(got[:28] - ref.sums[:28]) / np.maximum(bound, 1e-300)
    return ref, got


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_icp_sums_match_the_twin(pkg, frs, maps, stride):
    ref, got = _check_sums(pkg, maps.sv, maps.sn, frs[3].c2w, maps, stride)
    assert got[28] > 0.5 * _valid(maps.sn[::stride, ::stride]).sum()


@pytest.mark.parametrize("case", ["47x63", "one pixel", "no valid pixel"])
def test_icp_sums_at_the_launch_edges(pkg, frs, maps, case):
    sv, sn = maps.sv, maps.sn
    if case == "47x63":           # 2961 pixels: no multiple of a wave or a workgroup, 12 workgroups
        sv, sn = np.ascontiguousarray(sv[:47, :63]), np.ascontiguousarray(sn[:47, :63])
    elif case == "one pixel":
        sv, sn = np.ascontiguousarray(sv[20:21, 30:31]), np.ascontiguousarray(sn[20:21, 30:31])
        assert _valid(sn).all()
    else:
        sv = np.full_like(sv, np.nan)
    ref, got = _check_sums(pkg, sv, sn, frs[3].c2w, maps, 1)
    if case == "no valid pixel":
        assert (got == 0).all()
    if case == "47x63":
        assert got[28] > 1000


def test_icp_sums_reject_what_the_twin_rejects(pkg, frs, maps):
    moved = oc._od().se3_exp([0.012, 0.0, 0.0, 0.02, 0.0, 0.0]) @ frs[3].c2w        # 0.7 degrees and 2 cm
    ref, got = _check_sums(pkg, maps.sv, maps.sn, moved, maps, 1)
    base = oc.icp_sums_ref(maps.sv, maps.sn, frs[3].c2w, maps.mv, maps.mn, maps.w2c, 1)
    assert (ref.accept != base.accept).sum() > 10


def _random_maps(H, W, level, seed):
    """Seeded maps that pass every gate with thresholds wide open: a source vertex map whose pixels project onto
    themselves under identity poses, the same map with noise as the model / reference, random unit normals, random
    grey levels.  -> (camera intrinsics, a dict of device tensors)."""
    rng = np.random.default_rng([seed, H, W, level])
    fx = fy = 100.0
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    z = 1.0 + rng.random((H, W))
    v, u = np.mgrid[0:H, 0:W]
    sv = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)

    def normals():
        n = rng.standard_normal((H, W, 3))
        return n / np.linalg.norm(n, axis=-1, keepdims=True)

    S = 1 << level
    gray = (-(-H // S), -(-W // S))
    m = dict(sv=sv, sn=normals(), mv=sv + 0.01 * rng.standard_normal(sv.shape), mn=normals(),
             sg=rng.random(gray), rg=rng.random(gray))
    return (fx, fy, cx, cy), {k: _dev(a) for k, a in m.items()}


@pytest.mark.parametrize("H,W,level", [(16, 16, 0), (128, 128, 0), (130, 130, 0), (130, 130, 1)])
@pytest.mark.parametrize("entry", ["nslam_icp_sums", "nslam_photo_sums"])
def test_final_sums_are_the_partials_in_index_order(pkg, entry, H, W, level):
    """out[j] is, bit for bit, the sequential chain over partial[0..groups-1][j] for all 29 values: 1, 64, 67 and
    (at stride 2) 17 workgroups.  The terms and the workgroup stage are the twin comparisons' business."""
    import ctypes

    import ordered_sum_ref as osr
    import torch
    L, ptr = pkg._lib.lib(), pkg._lib.ptr
    intr, m = _random_maps(H, W, level, seed=3)
    stride = 1 << level
    groups = int(L.nslam_icp_partials(H, W, stride))
    assert groups == {(16, 0): 1, (128, 0): 64, (130, 0): 67, (130, 1): 17}[(H, level)]
    partial = torch.full((groups, 29), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((29,), float("nan"), dtype=torch.float64, device=DEV)
    eye = (ctypes.c_double * 16)(*np.eye(4).ravel())
    stream = pkg._lib.stream_ptr(DEV)
    if entry == "nslam_icp_sums":
        rc = L.nslam_icp_sums(ptr(m["sv"]), ptr(m["sn"]), H, W, stride, eye, ptr(m["mv"]), ptr(m["mn"]), H, W, eye,
                              *intr, 1.0e3, -1.0, ptr(partial), groups, ptr(out), None, stream)
    else:
        sh, sw = m["sg"].shape
        rc = L.nslam_photo_sums(ptr(m["sv"]), H, W, ptr(m["sg"]), sh, sw, ptr(m["rg"]), sh, sw, level, ptr(m["mv"]),
                                H, W, eye, eye, *intr, 1.0e3, 1.0e3, ptr(partial), groups, ptr(out), None, stream)
    assert rc == 0
    got, rows = out.cpu().numpy(), partial.cpu().numpy()
    print(f"{entry} {H}x{W} level {level}: {groups} workgroups, {int(got[28])} accepted pixels")
    assert got[28] > 0 and np.isfinite(rows).all()               # a row of zeros cannot pass
    assert np.array_equal(osr.bits(got), osr.bits(osr.ordered_sum(rows))), got - osr.ordered_sum(rows)


# ------------------------------------------------------------------------------------------------
# the tracker
# ------------------------------------------------------------------------------------------------
def _odometry(pkg, extent=oc.EXTENT, **kw):
    return pkg.odometry.DepthOdometry(K["H"], K["W"], *INTR, oc.L, oc.TRUNC, extent, DEV, oc.DEPTH_TRUNC, oc.MAX_JUMP,
                                      dist_th=oc.DIST_TH, angle_deg=oc.ANGLE_DEG, near=oc.NEAR, **kw)


def test_depth_odometry_follows_the_trajectory(pkg, frs):
    twin = oc.track_ref(frs)
    od = _odometry(pkg)
    res = [od.track(f.depth) for f in frs]
    assert np.array_equal(res[0]["c2w"], np.eye(4)) and not any(r["lost"] for r in res)
    assert od.fused == list(range(len(frs))) and od.lost == []
    for k in (1, 6, 12):
        dt, dr = oc.pose_error(res[k]["c2w"], twin[k]["c2w"])
        print(f"frame {k}: device - twin {1e3 * dt:.3f} mm {dr:.4f} deg, inliers {res[k]['inliers']} / "
              f"{twin[k]['inliers']}, rms {res[k]['rms']:.2e} / {twin[k]['rms']:.2e}")
    dt, dr = oc.pose_error(res[-1]["c2w"], frs[-1].c2w)
    tt, tr = oc.pose_error(twin[-1]["c2w"], frs[-1].c2w)
    print(f"final error: device {1e3 * dt:.3f} mm {dr:.4f} deg, twin {1e3 * tt:.3f} mm {tr:.4f} deg")
    assert dt <= 2.0 * tt and dr <= 2.0 * tr


def test_a_blank_frame_is_lost_and_the_next_one_tracks(pkg, frs):
    od = _odometry(pkg)
    for f in frs[:3]:
        od.track(f.depth)
    blocks = od.volume.n_blocks
    weight = od.volume.weight.sum().item()
    r = od.track(np.zeros_like(frs[3].depth))
    assert r["lost"] and r["inliers"] == 0 and od.lost == [3] and od.fused == [0, 1, 2]
    assert od.volume.n_blocks == blocks and od.volume.weight.sum().item() == weight
    assert np.allclose(r["c2w"], oc._od().predict(od.poses[:3]))
    r = od.track(frs[4].depth)
    dt, dr = oc.pose_error(r["c2w"], frs[4].c2w)
    assert not r["lost"] and dt < 0.01 and dr < 0.5 and od.fused == [0, 1, 2, 4]


def test_a_small_extent_raises_with_its_name(pkg, frs):
    od = _odometry(pkg, extent=0.5)
    with pytest.raises(ValueError, match="extent"):
        od.track(frs[0].depth)


# ------------------------------------------------------------------------------------------------
# tools/prep_own_data.py
# ------------------------------------------------------------------------------------------------
def test_prep_own_data_end_to_end(pkg, frs, tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("prep_own_data", os.path.join(REPO, "tools", "prep_own_data.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    folder = tmp_path / "scene0"
    os.makedirs(folder / "color")
    os.makedirs(folder / "depth")
    for i, f in enumerate(frs):
        Image.fromarray(f.color).save(str(folder / "color" / f"{i:05d}.jpg"))
        Image.fromarray(np.round(f.depth * 1000.0).astype(np.uint16)).save(str(folder / "depth" / f"{i:05d}.png"))
    (folder / "intrinsic.json").write_text(json.dumps(
        {"width": K["W"], "height": K["H"], "intrinsic_matrix": [K["fx"], 0, 0, 0, K["fy"], 0, K["cx"], K["cy"], 1]}))
    base = os.path.join(GOLDEN, "configs", "own.yaml")
    out = tmp_path / "own.yaml"
    argv = ["--scene_folder", str(folder), "--output_config", str(out), "--base", base, "--voxel", str(oc.L),
            "--trunc", str(oc.TRUNC), "--extent", str(oc.EXTENT), "--fuse_every", "2", "--depth_trunc", "20"]
    assert tool.main(argv) == 0
    log, ply = folder / "scene" / "trajectory.log", folder / "scene" / "integrated.ply"
    verts = pkg.evaluation.load_mesh(str(ply))["vertices"]
    assert verts.shape[0] > 1000
    cfg = pkg.config.load_config(str(out), os.path.join(GOLDEN, "configs", "nice_slam.yaml"))
    for key in ("bound", "marching_cubes_bound"):
        b = np.array(cfg["mapping"][key], dtype=np.float64)
        assert np.allclose(b[:, 0], verts.min(0) - 1.0, atol=1e-9) and np.allclose(b[:, 1], verts.max(0) + 1.0, atol=1e-9)
    ds = pkg.get_dataset(cfg, SimpleNamespace(input_folder=None), 1, device="cpu")
    assert len(ds) == len(frs)
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    for k in (0, 12):
        logged = ds.poses[k].numpy().astype(np.float64) @ flip
        dt, dr = oc.pose_error(logged, frs[k].c2w)
        assert dt < 0.02 and dr < 1.0, k
    assert np.array_equal(ds.poses[0].numpy(), flip.astype(np.float32))
    # again without --force: the mesh is used as it is, the log keeps its bytes
    before = log.read_bytes(), ply.read_bytes()
    assert tool.main(argv[:4]) == 0
    assert (log.read_bytes(), ply.read_bytes()) == before
