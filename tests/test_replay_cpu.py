"""Host-side checks of the replay (no GPU calls): the camera actor and the viewer's pose against viz.py's table and
rule, the Motion-JPEG AVI writer, the command line of the root visualizer.py, the argument checks of
nslam_scene_render, and the input conditions of tests/replay_cases.py on its numpy twins alone."""
import importlib.util
import io
import os
import struct

import numpy as np
import pytest

from conftest import REPO

import replay_cases as C

P = 4096  # a fake aligned device pointer, never dereferenced


def _cli():
    spec = importlib.util.spec_from_file_location("replay_cli", os.path.join(REPO, "visualizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------
# the actor, the viewer, the frontend's state
# ------------------------------------------------------------------------------------------------
def test_camera_actor_is_the_reference_table(pkg):
    # viz.py:15-26, restated
    cam_points = np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5],
                           [0.5, 1, 1.5], [0, 1.2, 1.5]])
    cam_lines = [[1, 2], [2, 3], [3, 4], [4, 1], [1, 3], [2, 4], [1, 0], [0, 2], [3, 0], [0, 4], [5, 7], [7, 6]]
    for is_gt, scale, colour in ((False, 0.3, (255, 0, 0)), (True, 0.005, (0, 0, 0))):
        pts, col = pkg.replay.camera_actor(is_gt, scale)
        assert pts.shape == (1200, 3) and pts.dtype == np.float64
        assert col.dtype == np.uint8 and tuple(col) == colour
        seg = pts.reshape(12, 100, 3)
        for k, (a, b) in enumerate(cam_lines):
            assert np.array_equal(seg[k, 0], scale * cam_points[a]) and np.array_equal(seg[k, -1], scale * cam_points[b])
            t = np.linspace(0.0, 1.0, 100)
            want = scale * cam_points[a][None] * (1.0 - t)[:, None] + scale * cam_points[b][None] * t[:, None]
            assert np.array_equal(seg[k], want)
    assert np.array_equal(C.actor_points(0.3), pkg.replay.camera_actor(False, 0.3)[0])


def test_viewer_extrinsic_closed_form(pkg):
    for pos, direction, up in (((1.0, 1.5, 1.2), (1.0, 0.1, -0.05), (0.0, 0.0, -1.0)),
                               ((-0.3, 2.0, 0.4), (0.2, -0.7, 0.4), (0.0, 1.0, 0.0))):
        pose = C.R.look(pos, direction, up)
        keep = pose.copy()
        got = pkg.replay.viewer_extrinsic(pose)
        assert np.array_equal(pose, keep)                              # computed on a copy
        # for a rigid pose: the viewer sits at t + 2 z with the pose's y and z axes negated; its inverse is the transpose form
        r = np.stack([pose[:3, 0], -pose[:3, 1], -pose[:3, 2]], 1)
        t = pose[:3, 3] + 2.0 * pose[:3, 2]
        want = np.eye(4)
        want[:3, :3], want[:3, 3] = r.T, -r.T @ t
        assert np.abs(got - want).max() <= 1e-12
    fx, fy, cx, cy = pkg.replay.intrinsics(1080, 1920, 60.0)
    assert fx == fy and abs(fx - 540.0 / np.tan(np.pi / 6)) < 1e-9 and (cx, cy) == (959.5, 539.5)


def test_frontend_state_without_a_device(pkg):
    import torch
    est = np.tile(np.eye(4), (12, 1, 1))
    est[:, 0, 3] = np.arange(12)
    gt = est.copy()
    gt[:, 1, 3] = 1.0
    r = pkg.replay.Replay("out", est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt)
    for pose in (C.R.look((1.0, 1.5, 1.2), (1.0, 0.1, -0.05), (0.0, 0.0, -1.0)),
                 torch.from_numpy(C.R.look((1.0, 1.5, 1.2), (1.0, 0.1, -0.05), (0.0, 0.0, -1.0)))):
        keep = pose.clone() if isinstance(pose, torch.Tensor) else pose.copy()
        r.update_pose(1, pose, gt=False)
        r.update_pose(1, pose, gt=True)
        assert (pose == keep).all()                                    # the reference flips the caller's array
        flipped = keep.numpy().copy() if isinstance(keep, torch.Tensor) else keep.copy()
        flipped[:3, 2] *= -1
        assert sorted(r.cameras) == [1, 100001]
        assert np.array_equal(r.cameras[1][1], flipped) and r.cameras[100001][0] is True
    p, c = r.point_set()
    assert p.shape == (2400, 3) and c.dtype == np.uint8
    assert (c[:1200] == (255, 0, 0)).all() and (c[1200:] == 0).all()
    want = pkg.replay.camera_actor(False, 0.3)[0] @ flipped[:3, :3].T + flipped[:3, 3]
    assert np.array_equal(p[:1200], want)
    r.update_cam_trajectory(0, gt=False)                               # list[1:0]: nothing yet
    assert r.point_set()[0].shape == (2400, 3)
    r.update_cam_trajectory(10, gt=False)
    r.update_cam_trajectory(10, gt=True)
    p, c = r.point_set()
    assert p.shape == (2400 + 18, 3) and np.array_equal(p[2400:2409], est[1:10, :3, 3])
    assert np.array_equal(p[2409:], gt[1:10, :3, 3]) and (c[2400:2409] == (255, 0, 0)).all() and (c[2409:] == 0).all()
    r.reset()
    assert r.cameras == {} and r.point_set()[0].shape == (18, 3)
    with pytest.raises(ValueError, match="cull"):
        pkg.replay.Replay("out", est[0], cull="both")


# ------------------------------------------------------------------------------------------------
# the AVI writer
# ------------------------------------------------------------------------------------------------
def test_mjpeg_avi(pkg, tmp_path):
    from PIL import Image
    g = np.random.default_rng(1)
    W, H = 20, 14
    jpegs = [pkg.visualizer.encode_jpeg(g.integers(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(5)]
    jpegs[2] = jpegs[2] + (b"" if len(jpegs[2]) & 1 else b"\0")        # one odd-sized chunk: it needs a pad byte
    path = str(tmp_path / "v.avi")
    pkg.replay.write_mjpeg_avi(path, jpegs, 30, W, H)
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    got = pkg.replay.read_mjpeg_avi(path)                              # walks every chunk: the sizes add up
    assert got["fps"] == 30.0 and got["usec"] == 33333 and got["fourcc"] == b"MJPG"
    assert (got["W"], got["H"], got["n"]) == (W, H, 5)
    assert got["frames"] == jpegs and len(got["index"]) == 5
    for (off, size), j in zip(got["index"], jpegs):                    # idx1 points at each frame's chunk
        at = got["movi"] + off
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == size == len(j)
        assert data[at + 8:at + 8 + size] == j
    for j in got["frames"]:
        assert Image.open(io.BytesIO(j)).size == (W, H)
    pkg.replay.write_mjpeg_avi(path, [], 30, W, H)
    assert pkg.replay.read_mjpeg_avi(path)["frames"] == []
    with pytest.raises(ValueError):
        pkg.replay.write_mjpeg_avi(path, jpegs, 0, W, H)


# ------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------
def test_cli_takes_the_reference_arguments():
    cli = _cli()
    a = cli.parse_args(["cfg.yaml", "--input_folder", "in", "--output", "out", "--imap", "--save_rendering",
                        "--vis_input_frame", "--no_gt_traj"])
    assert (a.config, a.input_folder, a.output, a.nice) == ("cfg.yaml", "in", "out", False)
    assert a.save_rendering and a.vis_input_frame and a.no_gt_traj
    d = cli.parse_args(["cfg.yaml"])
    assert d.nice and not d.save_rendering and not d.vis_input_frame and not d.no_gt_traj
    assert (d.width, d.height, d.fov, d.every, d.cull, d.point_size) == (1920, 1080, 60.0, 1, "none", 4)
    assert cli.parse_args(["cfg.yaml", "--nice"]).nice
    with pytest.raises(SystemExit):
        cli.parse_args(["cfg.yaml", "--nice", "--imap"])
    with pytest.raises(NotImplementedError, match="vis_input_frame"):
        cli.main(["cfg.yaml", "--vis_input_frame"])


# ------------------------------------------------------------------------------------------------
# nslam_scene_render's argument checks
# ------------------------------------------------------------------------------------------------
def _scene(L, **kw):
    import ctypes
    a = dict(verts=P, nv=8, faces=P, nf=12, vcol=P, nrm=P, f64=1, grey=(ctypes.c_uint8 * 3)(1, 2, 3), pts=P, pcol=P,
             np=5, size=4.0, w2c=P, nb=2, H=48, W=64, fx=40.0, fy=40.0, cx=31.5, cy=23.5, zn=0.0, zf=3.0, cull=0,
             bg=(ctypes.c_uint8 * 3)(255, 255, 255), ambient=0.3, small=64, passes=31, color=P, depth=None, ids=None,
             ws=P, wsb=L.nslam_scene_workspace_size(16, 2, 48, 64))
    a.update(kw)
    return L.nslam_scene_render(a["verts"], a["nv"], a["faces"], a["nf"], a["vcol"], a["nrm"], a["f64"], a["grey"],
                                a["pts"], a["pcol"], a["np"], a["size"], a["w2c"], a["nb"], a["H"], a["W"], a["fx"],
                                a["fy"], a["cx"], a["cy"], a["zn"], a["zf"], a["cull"], a["bg"], a["ambient"],
                                a["small"], a["passes"], a["color"], a["depth"], a["ids"], a["ws"], a["wsb"], None)


def test_scene_entry_point_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    assert L.nslam_scene_workspace_size(1, 2, 48, 64) == 24 + 8 * 2 * 48 * 64
    assert L.nslam_scene_workspace_size(0, 0, 48, 64) == 24
    assert L.nslam_scene_workspace_size(1000, 1, 1080, 1920) == 16 + 8000 + 8 * 1080 * 1920
    for k in ("verts", "faces", "nrm", "pts", "pcol", "w2c", "color", "ws", "bg"):
        assert _scene(L, **{k: None}) == -1, k
    assert _scene(L, vcol=None, grey=None) == -1                       # neither vertex colours nor a grey
    for k in ("nv", "nf", "np", "nb", "small"):
        assert _scene(L, **{k: -1}) == -1, k
    assert _scene(L, nv=0) == -1
    for k in ("H", "W"):
        assert _scene(L, **{k: 0}) == -1, k
    for k in ("fx", "fy"):
        for bad in (0.0, -40.0, float("nan"), float("inf")):
            assert _scene(L, **{k: bad}) == -1, (k, bad)
    assert _scene(L, cx=float("nan")) == -1 and _scene(L, cy=float("inf")) == -1
    assert _scene(L, zn=3.0, zf=3.0) == -1 and _scene(L, zn=-0.1) == -1 and _scene(L, zf=float("nan")) == -1
    assert _scene(L, cull=3) == -1 and _scene(L, cull=-1) == -1
    assert _scene(L, passes=32) == -1 and _scene(L, passes=-1) == -1
    assert _scene(L, ambient=1.5) == -1 and _scene(L, ambient=float("nan")) == -1 and _scene(L, ambient=-0.1) == -1
    assert _scene(L, size=0.0) == -1 and _scene(L, size=float("nan")) == -1
    assert _scene(L, size=64.5) == -2 and _scene(L, size=1e9) == -2    # NSLAM_EUNSUPPORTED
    assert _scene(L, wsb=L.nslam_scene_workspace_size(1, 2, 48, 64) - 1) == -1
    assert _scene(L, wsb=L.nslam_raster_workspace_size(16)) == -1      # the depth rasteriser's workspace: no keys
    assert _scene(L, nb=70000, wsb=1 << 40) == -2
    assert _scene(L, nb=0, w2c=None, color=None, ws=None, wsb=0) == 0  # no views: no launch


def test_render_scene_has_no_cpu_fallback(pkg):
    import torch
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    w2c = torch.eye(4, dtype=torch.float64)[None, :3].contiguous()
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.render_scene(v, f, None, v, None, None, w2c, 48, 64, 40., 40., 31.5, 23.5, 0.0, 3.0)


# ------------------------------------------------------------------------------------------------
# the references alone: the scenes put the renderer where the tests need it
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins():
    ms, (p, pc) = C.meshes(), C.point_set()
    return {name: [C.expected(m, c2w, p, pc, 4) for c2w in C.views()] for name, m in ms.items()}, p


def test_scenes_are_the_ones_described(twins):
    ms = C.meshes()
    assert ms["scene"][1].shape == (122, 3) and ms["two_spheres"][1].shape == (122 + 352, 3)
    for v, f, col, n in ms.values():
        assert col.shape == v.shape and col.dtype == np.uint8 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
    exp, p = twins
    assert p.shape == (1200 + 9 + 2, 3) and np.isnan(p[-1]).any() and np.array_equal(p[-2], C.TIE_POINT)
    assert (p[1200:1209, 1].min() < 0 < p[1200:1209, 1].max())         # the trajectory crosses the y = 0 wall
    npx = C.CAM["H"] * C.CAM["W"]
    for name, per_view in exp.items():
        for b, e in enumerate(per_view):
            und = int((~e["decided"]).sum())
            print(f"{name} view {b}: undecided {und}, point pixels winning {int(e['point_wins'].sum())}, losing "
                  f"{int(e['point_loses'].sum())}, tying {int(e['tie'].sum())}, points drawn {len(e['boxes'])}")
            assert und <= C.MAX_UNDECIDED * npx
            assert len(p) - 1 not in e["boxes"]                        # the NaN point is never drawn
        assert any(e["point_wins"].any() for e in per_view) and any(e["point_loses"].any() for e in per_view)
        assert any(0 < len(e["boxes"]) < len(p) - 1 for e in per_view)  # a view with points behind the camera
        assert any(k[4] for e in per_view for k in e["boxes"].values())  # a sprite that straddles the border
        tie = per_view[6]["tie"]
        assert tie.any() and (per_view[6]["ids_lo"][tie] >= 0).all() and per_view[6]["decided"][tie].all()
        assert len(p) - 2 in per_view[6]["boxes"]


def test_cull_scene(pkg):
    v, f, col, n = C.outward_box()
    c2w = C.R.look(*C.CULL_VIEW)
    e = {k: C.expected((v, f, col, n), c2w, cull=k) for k in ("none", "back", "front")}
    assert np.array_equal(e["none"]["ids_lo"], e["back"]["ids_lo"]) and e["none"]["decided"].all()
    box = (e["none"]["ids_lo"] >= 0) & (e["none"]["ids_lo"] < 12)
    assert box.sum() > 100 and (e["front"]["ids_lo"][box] >= 0).all() and (e["front"]["ids_lo"][box] < 12).all()
    assert (e["front"]["z_lo"][box] > e["none"]["z_lo"][box]).all()     # the far side of the box
    assert (e["front"]["ids_lo"][~box] == -1).all()                    # the floor is a front: culled
