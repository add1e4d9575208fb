"""Host-side checks of the depth-L1 metric (no GPU calls): the argument checks of nslam_raster_depth,
nslam_views_see_any and nslam_depth_l1, the oriented bounds, the view sampler's stream, and the refusal of CPU
tensors and of a missing unseen-point file."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

P = 4096  # a fake aligned device pointer, never dereferenced


def _raster(L, **kw):
    a = dict(verts=P, nv=8, faces=P, nf=12, w2c=P, nb=2, H=48, W=64, fx=40.0, fy=40.0, cx=31.5, cy=23.5, zn=0.1,
             zf=3.0, small=64, passes=15, depth=P, ws=P, wsb=L.nslam_raster_workspace_size(16))
    a.update(kw)
    return L.nslam_raster_depth(a["verts"], a["nv"], a["faces"], a["nf"], a["w2c"], a["nb"], a["H"], a["W"], a["fx"],
                                a["fy"], a["cx"], a["cy"], a["zn"], a["zf"], a["small"], a["passes"], a["depth"],
                                a["ws"], a["wsb"], None)


def test_raster_entry_point_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    one = L.nslam_raster_workspace_size(1)
    assert one == 24 and L.nslam_raster_workspace_size(0) == one and L.nslam_raster_workspace_size(-3) == one
    assert L.nslam_raster_workspace_size(1000) == 16 + 8 * 1000
    for k in ("verts", "faces", "w2c", "depth", "ws"):
        assert _raster(L, **{k: None}) == -1, k
    for k in ("nv", "nf", "nb", "small"):
        assert _raster(L, **{k: -1}) == -1, k
    assert _raster(L, nv=0) == -1                                   # faces of no vertices
    for k in ("H", "W"):
        assert _raster(L, **{k: 0}) == -1 and _raster(L, **{k: -4}) == -1, k
    for k in ("fx", "fy"):
        for bad in (0.0, -40.0, float("nan"), float("inf")):
            assert _raster(L, **{k: bad}) == -1, (k, bad)
    assert _raster(L, cx=float("nan")) == -1 and _raster(L, cy=float("inf")) == -1
    assert _raster(L, zn=3.0, zf=3.0) == -1 and _raster(L, zn=4.0, zf=3.0) == -1
    assert _raster(L, zn=float("nan")) == -1 and _raster(L, zf=float("nan")) == -1 and _raster(L, zn=-0.1) == -1
    assert _raster(L, wsb=one - 1) == -1 and _raster(L, wsb=0) == -1    # a short workspace
    assert _raster(L, passes=16) == -1 and _raster(L, passes=-1) == -1
    assert _raster(L, nb=70000) != 0                                # more views than one launch takes
    # empty work: no launch, whatever the pointers
    assert _raster(L, nb=0, w2c=None, depth=None, ws=None, wsb=0) == 0
    assert _raster(L, nf=0, faces=None, ws=None, wsb=0) == 0
    assert _raster(L, nf=0, nv=0, verts=None, faces=None) == 0


def test_views_see_any_and_depth_l1_validate_without_gpu(pkg):
    L = pkg._lib.lib()
    cam = (48, 64, 40.0, 40.0, 31.5, 23.5)
    assert L.nslam_views_see_any(None, 10, P, 2, *cam, P, None) == -1
    assert L.nslam_views_see_any(P, 10, None, 2, *cam, P, None) == -1
    assert L.nslam_views_see_any(P, 10, P, 2, *cam, None, None) == -1
    assert L.nslam_views_see_any(P, -1, P, 2, *cam, P, None) == -1
    assert L.nslam_views_see_any(P, 10, P, -2, *cam, P, None) == -1
    assert L.nslam_views_see_any(P, 10, P, 2, 0, 64, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_views_see_any(P, 10, P, 2, 48, -1, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_views_see_any(P, 10, P, 70000, *cam, P, None) != 0
    assert L.nslam_views_see_any(None, 0, P, 2, *cam, P, None) == 0          # no points: no launch
    assert L.nslam_views_see_any(P, 10, None, 0, *cam, None, None) == 0      # no views

    assert L.nslam_depth_l1(None, P, 3, 100, P, None) == -1
    assert L.nslam_depth_l1(P, None, 3, 100, P, None) == -1
    assert L.nslam_depth_l1(P, P, 3, 100, None, None) == -1
    assert L.nslam_depth_l1(P, P, -3, 100, P, None) == -1
    assert L.nslam_depth_l1(P, P, 3, -100, P, None) == -1
    assert L.nslam_depth_l1(P, P, 3, 0, P, None) == -1                        # the mean of no pixels
    assert L.nslam_depth_l1(None, None, 0, 100, None, None) == 0


def test_oriented_bounds_of_a_rotated_box(pkg):
    pytest.importorskip("scipy")
    E = pkg.evaluation
    ext = np.array([3.0, 1.0, 2.0])
    a, b, c = 0.7, -0.4, 1.1
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1.0, 0], [-np.sin(b), 0, np.cos(b)]])
    rx = np.array([[1.0, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    rot, shift = rz @ ry @ rx, np.array([0.5, -2.0, 1.5])
    g = np.random.default_rng(2)
    corners = np.array([[(k >> d) & 1 for d in range(3)] for k in range(8)], dtype=np.float64) - 0.5
    inside = g.random((200, 3)) - 0.5
    pts = (np.concatenate([corners, inside], 0) * ext) @ rot.T + shift
    to_origin, got = E.oriented_bounds(pts)
    assert np.abs(got - np.sort(ext)).max() <= 1e-9
    assert (np.diff(got) >= 0).all()
    r = to_origin[:3, :3]
    assert abs(np.linalg.det(r) - 1.0) <= 1e-12 and np.abs(r @ r.T - np.eye(3)).max() <= 1e-12
    assert np.array_equal(to_origin[3], [0.0, 0.0, 0.0, 1.0])
    local = pts @ r.T + to_origin[:3, 3]
    assert (np.abs(local) <= got / 2 + 1e-9).all()
    # get_cam_position: the shrunk extents, the inverse transform, 0.4 up
    e2, tr = E.get_cam_position(pts)
    assert np.abs(e2 - got * np.array([0.3, 0.7, 0.7])).max() <= 1e-12
    want = np.linalg.inv(to_origin)
    want[2, 3] += 0.4
    assert np.abs(tr - want).max() <= 1e-12
    assert np.abs(tr[:3, 3] - (shift + np.array([0.0, 0.0, 0.4]))).max() <= 1e-9


def test_view_stream_is_the_package_stream(pkg):
    import eval_scene
    E = pkg.evaluation
    for k in (0, 5):
        assert np.array_equal(E._uniforms(7, 0, 50, k), eval_scene.uniforms(7, 50, k))
        assert np.array_equal(E._uniforms(7, 20, 30, k), eval_scene.uniforms(7, 50, k)[20:])
    # no unseen points: no kernel is called, so the sampler itself runs here
    ext, tr = np.array([0.6, 1.5, 2.0]), np.eye(4)
    v = E.sample_views(4, ext, tr, np.zeros((0, 3)), 1)
    assert v.shape == (4, 4, 4) and np.array_equal(v, E.sample_views(9, ext, tr, None, 1, batch=2)[:4])
    assert (np.abs(v[:, :3, 3]) <= ext / 2).all()
    assert E.sample_views(0, ext, tr, None, 1).shape == (0, 4, 4)


def test_depth_l1_has_no_cpu_fallback(pkg, tmp_path):
    import torch
    E = pkg.evaluation
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    w2c = torch.eye(4, dtype=torch.float64)[None, :3].contiguous()
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.render_depth(v, f, w2c, 48, 64, 40., 40., 31.5, 23.5, 0.1, 3.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.depth_l1(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.views_see_any(v, torch.eye(4)[None], 48, 64, 40., 40., 31.5, 23.5)
    ply = str(tmp_path / "gt.ply")
    pkg.mesher.write_ply(ply, v.numpy(), f.numpy())
    with pytest.raises(FileNotFoundError, match="gt_pc_unseen.npy"):
        E.calc_depth_l1(ply, ply)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.calc_depth_l1(ply, ply, align=False, n_imgs=2, unseen_pc=np.zeros((0, 3)),
                        cam_box=(np.ones(3), np.eye(4)), device="cpu")
    with pytest.raises(NotImplementedError, match="calc_depth_l1"):
        E.calc_2d_metric(ply, ply)
