"""GPU tests of the TSDF volume (csrc/nslam_tsdf.hip, nice-slam_amd/tsdf.py) against the numpy twins of
tests/tsdf_cases.py: sample passes, integration, extraction, determinism, the Mesher's 'tsdf' hull bound and
tools/fuse_tsdf.py end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import tsdf_cases as tc
from conftest import GOLDEN, REPO, grids_from, sd_from

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

DEV = "cuda:0"
K = tc.CAM


def _intr():
    return K["fx"], K["fy"], K["cx"], K["cy"]


def upload(frames):
    import torch
    depth = torch.from_numpy(np.stack([f.depth for f in frames], 0)).to(DEV)
    color = torch.from_numpy(np.stack([f.color for f in frames], 0)).to(DEV)
    return depth, color, np.stack([f.c2w for f in frames], 0)


def gpu_fuse(pkg, frames, lo, hi, calls=None, color=True):
    """A TSDFVolume after one integrate call per entry of `calls` (default: one call with every frame)."""
    vol = pkg.tsdf.TSDFVolume(tc.L, tc.TRUNC, lo, hi, DEV, color=color, depth_stride=tc.STRIDE,
                              depth_trunc=tc.DEPTH_TRUNC)
    rets = []
    for call in calls or [list(range(len(frames)))]:
        d, c, p = upload([frames[i] for i in call])
        rets.append(vol.integrate(d, c if color else None, p, *_intr()))
    return vol, rets


def download(vol):
    import torch
    torch.cuda.synchronize()
    return SimpleNamespace(coords=vol.block_coords().cpu().numpy(), keys=vol.block_keys.cpu().numpy().astype(np.int64),
                           tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(),
                           color=None if vol.color is None else vol.color.cpu().numpy(),
                           table=vol.table.cpu().numpy())


@pytest.fixture(scope="module")
def corner(pkg):
    frames = tc.corner_frames(3)
    lo, hi, n_valid = tc.block_range(frames)
    vol, rets = gpu_fuse(pkg, frames, lo, hi)
    return SimpleNamespace(frames=frames, lo=lo, hi=hi, n_valid=n_valid, ref=tc.fuse_ref(frames, lo, hi),
                           f32=tc.fuse_f32(frames, lo, hi), vol=vol, rets=rets, got=download(vol))


@pytest.fixture(scope="module")
def wall(pkg):
    frames, plane = tc.wall_scene()
    lo, hi, _ = tc.block_range(frames)
    vol, _ = gpu_fuse(pkg, frames, lo, hi)
    return SimpleNamespace(frames=frames, plane=plane, lo=lo, hi=hi, ref=tc.fuse_ref(frames, lo, hi),
                           f32=tc.fuse_f32(frames, lo, hi), vol=vol, got=download(vol))


@pytest.fixture(scope="module")
def frames32():
    return tc.corner_frames(33)


# ------------------------------------------------------------------------------------------------
# range and touch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["full", "crop", "many"])
def test_block_range_matches_reference(pkg, frames32, case):
    frames = {"full": frames32[:3], "crop": tc.corner_frames(3, H=23, W=30), "many": frames32}[case]
    H, W = frames[0].depth.shape
    invalid = sum(int((~(f.depth[::tc.STRIDE, ::tc.STRIDE] > 0)).sum()
                      + (f.depth[::tc.STRIDE, ::tc.STRIDE] > tc.DEPTH_TRUNC).sum()) for f in frames)
    assert invalid >= 2 * len(frames)             # zero, NaN and over-range depths sit on strided pixels
    want = tc.block_range(frames)
    d, _, p = upload(frames)
    got = pkg.tsdf.TSDFVolume.block_range(d, p, H, W, *_intr(), tc.L, tc.TRUNC, tc.STRIDE, tc.DEPTH_TRUNC)
    print(f"{case}: {got}")
    assert got == want and want[2] > 20 * len(frames)


def test_block_range_without_a_valid_sample(pkg):
    import torch
    depth = torch.zeros(2, K["H"], K["W"], device=DEV)
    depth[0, 1, 1] = 1.0                          # valid, but not on the stride
    depth[1, 4, 4] = float("nan")
    depth[1, 8, 8] = 2000.0
    got = pkg.tsdf.TSDFVolume.block_range(depth, np.stack([np.eye(4)] * 2), K["H"], K["W"], *_intr(), tc.L, tc.TRUNC)
    assert got == (None, None, 0)


def _touch(pkg, frames, lo, hi):
    d, _, p = upload(frames)
    import torch
    mask, n_out = pkg.ops.tsdf_touch(d, torch.from_numpy(p).to(DEV), K["H"], K["W"], *_intr(), tc.STRIDE,
                                     tc.DEPTH_TRUNC, tc.L, tc.TRUNC, lo, hi)
    return mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, int(n_out)


@pytest.mark.parametrize("n", [1, 31, 32])
def test_touch_masks_match_reference(pkg, frames32, n):
    frames = frames32[:n]
    lo, hi, _ = tc.block_range(frames)
    want, n_out, _ = tc.touch(frames, lo, hi)
    got, got_out = _touch(pkg, frames, lo, hi)
    assert np.array_equal(got, want) and got_out == n_out == 0
    assert int(want.max()) >> (n - 1) == 1        # the last frame's bit is in use


@pytest.mark.parametrize("side", range(6))
def test_touch_counts_samples_outside_a_small_table(pkg, corner, side):
    lo, hi = list(corner.lo), list(corner.hi)
    if side < 3:
        lo[side] += 1
    else:
        hi[side - 3] -= 1
    want, n_out, _ = tc.touch(corner.frames, lo, hi)
    got, got_out = _touch(pkg, corner.frames, lo, hi)
    assert n_out > 0 and got_out == n_out
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------
# integrate
# ------------------------------------------------------------------------------------------------
def _compare(name, got, ref, f32, n_frames):
    """Pool order, weights, tsdf and colour bit-equal to the float32 twin outside the margins (the kernel runs
    the twin's float32 operations in the twin's order, and division and square root are correctly rounded on
    both sides), which puts them within the twin's own float32 floor of the float64 reference; both figures are
    printed, and the bound of twice that floor is asserted too."""
    assert np.array_equal(got.coords, f32.coords)
    cmp = ~(ref.margin | f32.margin)
    assert cmp.mean() > 0.98
    assert np.array_equal(got.weight[cmp], f32.weight[cmp])
    seen = cmp & (ref.weight > 0)
    floor_t = np.abs(ref.tsdf - f32.tsdf)[seen].max()
    err_t = np.abs(ref.tsdf - got.tsdf)[seen].max()
    bits = got.tsdf[cmp].tobytes() == f32.tsdf[cmp].tobytes()
    bits_all = got.tsdf.tobytes() == f32.tsdf.tobytes() and got.weight.tobytes() == f32.weight.tobytes()
    print(f"{name}: tsdf error {err_t:.3e} (float32 floor {floor_t:.3e}); bit-equal to the float32 twin: "
          f"{bits} outside the margins, {bits_all} everywhere")
    assert err_t <= 2 * floor_t
    assert bits
    if got.color is not None:
        floor_c = np.abs(ref.color - f32.color)[:, seen].max()
        err_c = np.abs(ref.color - got.color)[:, seen].max()
        bits_c = got.color[:, cmp].tobytes() == f32.color[:, cmp].tobytes()
        print(f"{name}: colour error {err_c:.3e} (float32 floor {floor_c:.3e}); bit-equal: {bits_c}")
        assert err_c <= 2 * floor_c
        assert bits_c
    return bits


def test_integrate_matches_the_twins(corner, wall):
    for name, s in (("wall", wall), ("corner", corner)):
        _compare(name, s.got, s.ref, s.f32, len(s.frames))
    assert corner.rets == [{"n_new_blocks": corner.f32.coords.shape[0], "n_outside": 0}]
    assert corner.vol.n_blocks == corner.f32.coords.shape[0]
    # a block only frame 0 touched holds weight 1 although frame 1 sees it
    only0 = tc.touched_by_0_only(corner.ref, corner.frames)
    assert only0
    for pid in only0:
        assert corner.got.weight[pid].max() == 1.0


def test_integrate_skips_voxels_behind_the_camera_and_off_the_image(pkg, corner):
    frames = corner.frames + [tc.close_frame()]
    lo, hi, _ = tc.block_range(frames)
    ref, f32 = tc.fuse_ref(frames, lo, hi), tc.fuse_f32(frames, lo, hi)
    assert ref.behind > 1000 and ref.off_image > 1000
    vol, _ = gpu_fuse(pkg, frames, lo, hi)
    _compare("with the close frame", download(vol), ref, f32, len(frames))


def test_integrate_splits_33_frames(pkg, frames32):
    lo, hi, _ = tc.block_range(frames32)
    ref = tc.fuse_ref(frames32, lo, hi, color=False)          # calls of 32 and 1
    f32 = tc.fuse_f32(frames32, lo, hi, color=False)
    vol, rets = gpu_fuse(pkg, frames32, lo, hi, color=False)
    assert len(f32.new_blocks) == 2 and f32.weight.max() > 16
    assert rets == [{"n_new_blocks": sum(f32.new_blocks), "n_outside": sum(f32.n_outside)}]
    _compare("33 frames", download(vol), ref, f32, 33)


def test_second_call_appends_blocks_in_key_order(pkg, corner):
    calls = [[0, 1], [2]]
    f32 = tc.fuse_f32(corner.frames, corner.lo, corner.hi, calls=calls)
    vol, rets = gpu_fuse(pkg, corner.frames, corner.lo, corner.hi, calls=calls)
    got = download(vol)
    assert [r["n_new_blocks"] for r in rets] == f32.new_blocks and min(f32.new_blocks) > 0
    assert np.array_equal(got.coords, f32.coords)
    n0 = f32.new_blocks[0]
    assert (np.diff(got.keys[:n0]) > 0).all() and (np.diff(got.keys[n0:]) > 0).all()
    assert got.keys[n0:].min() < got.keys[:n0].max()          # appended, not merged into the key order
    assert np.array_equal(got.table[got.keys], np.arange(got.keys.shape[0]))
    cmp = ~f32.margin
    assert np.array_equal(got.weight[cmp], f32.weight[cmp])
    assert (got.weight[:n0].max(1) > 2).any()                 # old blocks were updated by the second call


def _by_block(g):
    order = np.lexsort(g.coords.T[::-1])
    return g.coords[order], g.tsdf[order], g.weight[order], None if g.color is None else g.color[:, order]


def test_one_call_equals_two_calls_bit_for_bit(pkg, corner):
    fr = corner.frames[:2]
    one = download(gpu_fuse(pkg, fr, corner.lo, corner.hi)[0])
    two = download(gpu_fuse(pkg, fr, corner.lo, corner.hi, calls=[[0], [1]])[0])
    assert not np.array_equal(one.coords, two.coords)         # the pool orders differ: (call, key)
    for a, b in zip(_by_block(one), _by_block(two)):
        assert a.tobytes() == b.tobytes()


def test_volume_without_colour(pkg, corner):
    vol, _ = gpu_fuse(pkg, corner.frames, corner.lo, corner.hi, color=False)
    got = download(vol)
    assert got.color is None and vol.extract_mesh()["colors"] is None
    assert got.tsdf.tobytes() == corner.got.tsdf.tobytes() and got.weight.tobytes() == corner.got.weight.tobytes()


# ------------------------------------------------------------------------------------------------
# extract
# ------------------------------------------------------------------------------------------------
def _mesh(vol):
    import torch
    m = vol.extract_mesh()
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in m.items()}


@pytest.mark.parametrize("name", ["wall", "corner"])
def test_extract_matches_reference_on_the_downloaded_volume(corner, wall, name):
    s = {"wall": wall, "corner": corner}[name]
    got = _mesh(s.vol)
    want = tc.extract_ref(s.got.tsdf, s.got.weight, s.got.color, s.got.keys, s.lo, s.hi)
    print(f"{name}: blocks {s.vol.n_blocks} V {got['vertices'].shape[0]} F {got['faces'].shape[0]}")
    assert got["vertices"].dtype == np.float64 and got["faces"].dtype == np.int32 and got["colors"].dtype == np.uint8
    assert got["faces"].shape == want["faces"].shape and got["faces"].shape[0] > 500
    assert np.array_equal(got["faces"], want["faces"])
    assert got["vertices"].tobytes() == want["vertices"].tobytes()
    assert np.array_equal(got["colors"], want["colors"])


def test_wall_normals_face_the_camera(wall):
    m = _mesh(wall.vol)
    n, c = wall.plane
    v, f = m["vertices"], m["faces"]
    assert np.abs(v @ n - c).max() <= 1e-5
    eye = wall.frames[0].c2w[:3, 3]
    assert (np.einsum("ij,ij->i", tc.face_normals(v, f), eye - v[f[:, 0]]) > 0).all()


def test_empty_volume_and_volume_without_a_crossing(pkg, wall):
    vol = pkg.tsdf.TSDFVolume(tc.L, tc.TRUNC, wall.lo, wall.hi, DEV)
    m = _mesh(vol)
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["colors"].shape == (0, 3)
    # the table ends in front of the wall: every fused voxel is on the free side
    hi = [0, wall.hi[1], wall.hi[2]]
    vol, rets = gpu_fuse(pkg, wall.frames, wall.lo, hi)
    assert vol.n_blocks > 0 and rets[0]["n_outside"] > 0
    got = download(vol)
    assert (got.weight > 0).any() and (got.tsdf[got.weight > 0] > 0).all()
    m = _mesh(vol)
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["colors"].shape == (0, 3)


def test_two_runs_are_bit_identical(pkg, corner):
    vol, _ = gpu_fuse(pkg, corner.frames, corner.lo, corner.hi)
    got = download(vol)
    assert np.array_equal(got.keys, corner.got.keys)
    for k in ("tsdf", "weight", "color"):
        assert getattr(got, k).tobytes() == getattr(corner.got, k).tobytes(), k
    a, b = _mesh(vol), _mesh(corner.vol)
    for k in ("vertices", "faces", "colors"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------
# Mesher
# ------------------------------------------------------------------------------------------------
SCALE = 4.0     # the reference's sizes at this scale: voxel 1/32, truncation 0.16, blocks of 0.5


def _mesher(pkg, **over):
    import torch

    import mesh_scene
    cfg = {"coarse": True, "scale": SCALE, "occupancy": True,
           "meshing": {"resolution": 8, "level_set": 0, "clean_mesh_bound_scale": 1.02,
                       "remove_small_geometry_threshold": 0.2, "color_mesh_extraction_method": "direct_point_query",
                       "get_largest_components": False, "depth_test": True},
           "mapping": {"marching_cubes_bound": mesh_scene.MC_BOUND}}
    cfg["meshing"].update(over)
    slam = SimpleNamespace(renderer=None, bound=torch.tensor(mesh_scene.MC_BOUND, dtype=torch.float64), nice=True,
                           verbose=False, **mesh_scene.CAM)
    return pkg.Mesher(cfg, None, slam)


def _keyframes(frames):
    """The frames as the package keeps keyframes: est_c2w in its own convention (y and z flipped), float32."""
    import torch
    kfs = []
    for f in frames:
        c2w = f.c2w.copy()
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        kfs.append({"est_c2w": torch.from_numpy(c2w.astype(np.float32)), "depth": torch.from_numpy(f.depth.copy()),
                    "color": torch.from_numpy(f.color.astype(np.float32) / np.float32(255.0))})
    return kfs


def _scaled_hull(pts, s):
    from scipy.spatial import ConvexHull
    hull = ConvexHull(pts)
    eq = np.array(hull.equations, dtype=np.float64)
    centre = pts[hull.vertices].mean(0)
    nc = eq[:, :3] @ centre
    eq[:, 3] = s * (nc + eq[:, 3]) - nc
    return eq


def test_mesher_tsdf_bound(pkg):
    pytest.importorskip("scipy")
    frames = tc.corner_frames(3, holes=False)
    kfs = _keyframes(frames)
    before = [kf["est_c2w"].clone() for kf in kfs]
    m = _mesher(pkg)
    planes = m.get_bound_from_frames(kfs, SCALE, method="tsdf")
    for kf, b in zip(kfs, before):
        assert kf["est_c2w"].numpy().tobytes() == b.numpy().tobytes()          # the poses are not edited
    voxel, trunc = 4.0 * SCALE / 512.0, 0.04 * SCALE
    # the volume the Mesher fused, block for block the reference's at these sizes (float32 poses, as kept)
    vol = m.fuse_keyframes(kfs, SCALE)
    got = download(vol)
    as_kept = [SimpleNamespace(depth=f.depth, color=f.color, c2w=pkg.tsdf.opengl_to_cv(kf["est_c2w"]).astype(np.float64))
               for f, kf in zip(frames, kfs)]
    lo, hi, _ = tc.block_range(as_kept, trunc=trunc, block=16.0 * voxel)
    assert (vol.block_lo, vol.block_hi) == (lo, hi)
    # (the twin inverts float64 poses; the Mesher inverts the kept float32 ones: compare block sets and weights)
    f32 = tc.fuse_f32(as_kept, lo, hi, voxel=voxel, trunc=trunc)
    assert np.array_equal(got.coords, f32.coords)
    assert (got.weight != f32.weight).mean() < 0.01
    want = tc.extract_ref(got.tsdf, got.weight, got.color, got.keys, lo, hi, voxel=voxel)
    centres = np.stack([kf["est_c2w"].numpy().astype(np.float64)[:3, 3] for kf in kfs], 0)
    ref = _scaled_hull(np.concatenate([centres, want["vertices"]], 0), 1.02)
    assert planes.shape == ref.shape and planes.shape[0] >= 4
    order = lambda p: p[np.lexsort(np.round(p, 6).T[::-1])]  # noqa: E731
    print(f"tsdf hull: {planes.shape[0]} planes, V {want['vertices'].shape[0]}, "
          f"max plane difference {np.abs(order(planes) - order(ref)).max():.2e}")
    assert np.abs(order(planes) - order(ref)).max() <= 1e-9
    # the fused surface stays near the back-projected depths
    m1 = _mesher(pkg, clean_mesh_bound_scale=1.0)
    pts_hull = m1.get_bound_from_frames(kfs, SCALE, stride=1, method="points")
    dist = (want["vertices"] @ pts_hull[:, :3].T + pts_hull[:, 3]).max(1)
    print(f"largest distance of a TSDF vertex outside the 'points' hull: {dist.max():.4f}")
    assert dist.max() <= trunc + np.sqrt(3.0) * voxel
    # the configured default
    m2 = _mesher(pkg, bound_from="tsdf")
    assert m2.get_bound_from_frames(kfs, SCALE).tobytes() == planes.tobytes()


def test_get_mesh_with_the_tsdf_bound_writes_a_ply(pkg, tiny, tmp_path):
    pytest.importorskip("scipy")
    import torch

    import scenes
    dev = torch.device(DEV)
    scale = 2.0
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
           "meshing": {"resolution": 32, "level_set": 0.0, "clean_mesh_bound_scale": 1.02, "bound_from": "tsdf",
                       "remove_small_geometry_threshold": 0.002, "color_mesh_extraction_method": "direct_point_query",
                       "get_largest_components": False, "depth_test": True},
           "mapping": {"marching_cubes_bound": (np.array(scenes.TINY_BOUND) / scale).tolist()}}
    slam = SimpleNamespace(nice=True, bound=bound, verbose=False, **cam)
    slam.renderer = pkg.Renderer(cfg, None, slam)
    m = pkg.Mesher(cfg, None, slam, points_batch_size=8192)
    b, poses, _ = scenes.tiny_window(3)
    kfs = [{"est_c2w": torch.from_numpy(p), "depth": torch.from_numpy(scenes.box_depth(p, cam, b, seed=40 + k)),
            "color": torch.from_numpy(scenes.color_image(cam, seed=60 + k))} for k, p in enumerate(poses)]
    c2w_list = torch.from_numpy(np.stack(poses, 0))
    planes = m.get_bound_from_frames(kfs, scale)
    pts = m.get_grid_uniform(32)["grid_points"].to(dev).contiguous()
    inside = pkg.ops.points_in_hull(pts, torch.from_numpy(planes).to(dev))
    assert 0 < int(inside.sum()) < pts.shape[0]
    with torch.no_grad():
        m.level_set = float(m.eval_points(pts[inside], nice, c, "fine", dev)[:, -1].median())
    path = str(tmp_path / "mesh.ply")
    m.get_mesh(path, c, nice, kfs, c2w_list, 2, dev, clean_mesh=True)
    got = pkg.mesher.read_ply(path)
    print(f"get_mesh with bound_from tsdf: V {got['vertices'].shape[0]} F {got['faces'].shape[0]}")
    assert got["faces"].shape[0] > 0 and got["colors"] is not None


# ------------------------------------------------------------------------------------------------
# tools/fuse_tsdf.py
# ------------------------------------------------------------------------------------------------
def _write_run(root, frames):
    """A Replica-layout folder and an output folder with one checkpoint: est = the frames' poses, gt = the same
    poses moved by 5 cm, frame 3's estimate NaN."""
    import torch
    import yaml
    from PIL import Image
    data, out = os.path.join(root, "data"), os.path.join(root, "out")
    os.makedirs(os.path.join(data, "results"))
    os.makedirs(os.path.join(out, "ckpts"))
    est, gt = [], []
    with open(os.path.join(data, "traj.txt"), "w") as f:
        for i, fr in enumerate(frames):
            Image.fromarray(fr.color).save(os.path.join(data, f"results/frame{i:06d}.jpg"), quality=95)
            d = np.nan_to_num(fr.depth, nan=0.0)
            Image.fromarray(np.clip(np.rint(d * 1000.0), 0, 65535).astype(np.uint16)).save(
                os.path.join(data, f"results/depth{i:06d}.png"))
            f.write(" ".join(f"{v:.17g}" for v in fr.c2w.ravel()) + "\n")       # the loader flips y and z
            gl = fr.c2w.copy()
            gl[:3, 1] *= -1
            gl[:3, 2] *= -1
            est.append(torch.from_numpy(gl.astype(np.float32)))
            moved = gl.copy()
            moved[:3, 3] += 0.05
            gt.append(torch.from_numpy(moved.astype(np.float32)))
    est = torch.stack(est, 0)
    est[3] = float("nan")
    torch.save({"c": {}, "decoder_state_dict": {}, "gt_c2w_list": torch.stack(gt, 0), "estimate_c2w_list": est,
                "keyframe_list": [0], "selected_keyframes": None, "idx": torch.tensor(len(frames) - 1)},
               os.path.join(out, "ckpts", "00005.tar"), _use_new_zipfile_serialization=False)
    cfg = {"dataset": "replica", "scale": 1, "data": {"input_folder": data, "output": out},
           "cam": dict(tc.CAM, png_depth_scale=1000.0, crop_edge=0),
           "mapping": {"bound": [[-1.5, 1.8], [-1.3, 1.5], [-1.2, 1.6]]}}
    path = os.path.join(root, "run.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path, data, out


def test_fuse_tsdf_tool(pkg, tmp_path, capsys):
    import torch
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import fuse_tsdf
    finally:
        sys.path.pop(0)
    frames = tc.corner_frames(6, holes=False)
    cfg_path, data, out = _write_run(str(tmp_path), frames)
    args = [cfg_path, "--voxel", str(tc.L), "--trunc", str(tc.TRUNC)]
    res = fuse_tsdf.main(args + ["--every", "1"])
    text = capsys.readouterr().out
    assert res["frames"] == 5 and res["skipped"] == 1 and res["mesh"] == os.path.join(out, "mesh", "tsdf_mesh.ply")
    assert f"frames 5 (skipped 1) blocks {res['blocks']} V {res['V']} F {res['F']} n_outside {res['n_outside']}" in text
    mesh = pkg.evaluation.load_mesh(res["mesh"])
    assert mesh["vertices"].shape == (res["V"], 3) and mesh["faces"].shape == (res["F"], 3) and res["F"] > 500
    assert mesh["colors"] is not None and mesh["colors"].shape[0] == res["V"]

    # the same volume in process: the frames as the reader decodes them, the estimate's poses
    ds = pkg.get_dataset(fuse_tsdf.load_config(cfg_path), SimpleNamespace(input_folder=None), 1, device=DEV)
    ck = pkg.datasets.load_checkpoint(os.path.join(out, "ckpts", "00005.tar"), device="cpu")

    def in_process(poses, idx):
        lo = [int(np.floor((b - tc.TRUNC) / tc.B)) for b in (-1.5, -1.3, -1.2)]
        hi = [int(np.floor((b + tc.TRUNC) / tc.B)) + 1 for b in (1.8, 1.5, 1.6)]
        vol = pkg.tsdf.TSDFVolume(tc.L, tc.TRUNC, lo, hi, DEV)
        items = [ds[i] for i in idx]
        r = vol.integrate(torch.stack([it[2].float() for it in items], 0),
                          torch.stack([(it[1].float() * 255).to(torch.uint8) for it in items], 0),
                          np.stack([pkg.tsdf.opengl_to_cv(poses[i]) for i in idx], 0), *_intr())
        m = vol.extract_mesh()
        return vol.n_blocks, int(m["vertices"].shape[0]), int(m["faces"].shape[0]), r["n_outside"], m

    nb, nv, nf, n_out, m = in_process(ck["estimate_c2w_list"], [0, 1, 2, 4, 5])
    assert (res["blocks"], res["V"], res["F"], res["n_outside"]) == (nb, nv, nf, n_out)
    assert np.array_equal(mesh["vertices"].astype(np.float32), m["vertices"].cpu().numpy().astype(np.float32))
    assert np.array_equal(mesh["faces"], m["faces"].cpu().numpy())

    # --traj gt --every 2: frames 0, 2, 4 along the moved trajectory, into the file asked for
    other = str(tmp_path / "gt.ply")
    res2 = fuse_tsdf.main(args + ["--traj", "gt", "--every", "2", "--mesh", other, "--input_folder", data])
    assert res2["frames"] == 3 and res2["skipped"] == 0 and os.path.exists(other)
    nb, nv, nf, n_out, _ = in_process(ck["gt_c2w_list"], [0, 2, 4])
    assert (res2["blocks"], res2["V"], res2["F"], res2["n_outside"]) == (nb, nv, nf, n_out)
    assert (res2["V"], res2["F"]) != (res["V"], res["F"])
