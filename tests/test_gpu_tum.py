"""TUM-RGBD on the device: nslam_undistort_u8 against the numpy restatement, device frames against host
frames, and the fused camera tail with separate learning rates (nslam_cam_grad_step_lr2) against the
reference's seperate_LR loop (tests/golden/tum_fixtures.npz `track2`, tests/golden/make_golden_tum.py:
Tracker.py:202-247 over Tracker.optimize_cam_in_batch), against nslam_cam_grad_step, and through
Tracker.track_frame (fused vs the autograd loop; the captured graph vs the eager engine loop).

Tolerances: the undistortion is exact integer arithmetic after one rounding step, so every pixel is bit-equal
except where 32·map lies within 1e-6 of a half-integer (a last-bit difference of the float64 map may pick the
other 1/32 cell): those are left out, at most 0.01 % of the image.  The loop bars are those of
tests/test_gpu_loop.py::test_tracker_loop_matches_reference (losses rtol 2e-4, camera displacement rel-L2 1e-2)
and tests/test_gpu_fused.py::test_tracker_track_frame_fused_matches_loop (atol 5e-4).
"""
import copy
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, FixedPixels, rel_l2
from test_gpu_dropins import Scene, base_cfg
from test_gpu_loop import loop_cfg, tiny_slam
from test_tum_cpu import rebuild_tum

sys.path.insert(0, GOLDEN)
import scenes  # noqa: E402
import tum_scene  # noqa: E402

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
DIST = tum_scene.FREIBURG1_DIST


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "tum_fixtures.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _undistort_case(H, W, C, scale):
    """(image, restatement's output, left-out mask), computed once."""
    img = tum_scene.random_u8(H, W, C, seed=H + C)
    intr = tum_scene.intrinsics(scale)
    want = tum_scene.undistort_u8(img, *intr, DIST)
    skip = tum_scene.near_half(*tum_scene.undistort_map(H, W, *intr, DIST), tol=1e-6)
    return img, intr, want, skip


@pytest.mark.parametrize("H,W,C,scale", [(48, 64, 3, 0.1), (37, 53, 3, 0.085), (48, 64, 1, 1.0), (480, 640, 3, 1.0)])
def test_undistort_u8_matches_restatement(H, W, C, scale):
    img, intr, want, skip = _undistort_case(H, W, C, scale)
    got = P.ops.undistort_u8(torch.from_numpy(img).to(DEV), *intr, DIST).cpu().numpy()
    share = float(skip.mean())
    print(f"undistort {H}x{W}x{C}: {int(skip.sum())} of {skip.size} pixels left out ({share:.2e})")
    assert share <= 1e-4
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got[~skip], want[~skip])
    assert not np.array_equal(got, img)


def test_undistort_u8_identity_and_2d():
    img, intr, want, skip = _undistort_case(48, 64, 3, 0.1)
    assert int(skip.sum()) == 0  # (nearest margin 5e-5 at this shape: nothing is left out)
    src = torch.from_numpy(img).to(DEV)
    assert torch.equal(P.ops.undistort_u8(src, *intr, [0.0] * 5), src)
    # the zero border is exercised: 257 of the 3072 pixels have a tap outside the image
    assert tum_scene.taps_outside(48, 64, *intr, DIST) == 257
    # a [H, W] image, and `out`
    g = src[:, :, 1].contiguous()
    out = torch.empty_like(g)
    assert P.ops.undistort_u8(g, *intr, DIST, out=out) is out
    assert np.array_equal(out.cpu().numpy(), tum_scene.undistort_u8(img[:, :, 1].copy(), *intr, DIST))
    with pytest.raises(ValueError):
        P.ops.undistort_u8(src, *intr, DIST[:4])
    with pytest.raises(ValueError):
        P.ops.undistort_u8(src, *intr, DIST, out=src)


def test_tum_device_frames_equal_host_frames(fx, tmp_path):
    cfg = rebuild_tum(fx, tmp_path)
    scale = float(fx["tumrgbd.scale"])
    host = P.get_dataset(cfg, None, scale, device="cpu")
    dev = P.get_dataset(cfg, None, scale, device="cuda:0")
    assert len(host) == len(dev) == int(fx["tumrgbd.n"])
    intr = (host.fx, host.fy, host.cx, host.cy)
    for k in range(len(host)):
        u8, _ = host._load_host(k)
        und = P.ops.undistort_u8(u8.to(DEV), *intr, host.distortion)
        assert np.array_equal(und.cpu().numpy(), P.datasets.undistort_u8(u8.numpy(), *intr, host.distortion)), k
        _, c0, d0, p0 = host[k]
        _, c1, d1, p1 = dev[k]
        assert c1.is_cuda and d1.is_cuda and p1.is_cuda
        assert torch.equal(d1.cpu(), d0) and torch.equal(p1.cpu(), p0), k
        assert float((c1.cpu() - c0).abs().max()) < 1e-12, k
        assert float((c1.cpu() - torch.from_numpy(fx[f"tumrgbd.{k}.color"])).abs().max()) < 1e-12, k


def test_tum_prefetch_yields_getitem_on_device(fx, tmp_path):
    """The undistortion runs on prefetch's side stream: the same tuples as dataset[i], in the requested order."""
    cfg = rebuild_tum(fx, tmp_path)
    a = P.get_dataset(cfg, None, 0.5, device="cuda:0")
    b = P.get_dataset(cfg, None, 0.5, device="cuda:0")
    order = [2, 0, 3, 1]
    got = list(a.prefetch(order, workers=2, ahead=3))
    assert [g[0] for g in got] == order
    for g in got:
        e = b[g[0]]
        for x, y in zip(g[1:], e[1:]):
            assert x.device == y.device and x.dtype == y.dtype and torch.equal(x, y)


# ------------------------------------------------------------------------------------------------
# separate learning rates on the fused camera tail
# ------------------------------------------------------------------------------------------------
def _tiny_tracker(tiny, cfg):
    cam = scenes.TINY_CAM
    tr = P.Tracker(cfg, None, tiny_slam(tiny, cfg, cam))
    tr.update_para_from_mapping()
    return tr


def test_engine_lr2_matches_reference_loop(tiny, fx):
    """TrackingEngine.iteration(lr_quat, best_before_step) against the reference's seperate_LR loop on the
    fixture's draws, 4 iterations: the losses, the camera after every step, and the kept best camera — the one
    at the top of the reference's best iteration, not the one after that iteration's step."""
    cam = scenes.TINY_CAM
    b, _, cur = scenes.tiny_window()
    depth = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=int(fx["track2.depth_seed"]))).to(DEV)
    color = torch.from_numpy(scenes.color_image(cam, seed=int(fx["track2.color_seed"]))).to(DEV)
    eng = _tiny_tracker(tiny, loop_cfg()).engine()
    fp = FixedPixels(int(fx["track2.draw_seed"]))
    cam0 = torch.from_numpy(fx["track2.cam0"])
    lr, lr_quat, n = float(fx["track2.lr"]), float(fx["track2.lr_quat"]), int(fx["track2.pixels"])
    assert (lr, lr_quat) == (0.001, 0.0002)
    tops, final = fx["track2.tops"], fx["track2.final"]
    iters = tops.shape[0]
    assert iters == 4
    after_ref = [tops[k + 1] for k in range(iters - 1)] + [final]
    camf = cam0.to(DEV).clone().requires_grad_(True)
    opt = P.ops.FusedAdam([{"params": [camf], "lr": lr}])
    best = (torch.full((), float("inf"), dtype=torch.float64, device=DEV), torch.zeros(7, device=DEV))
    losses, after = [], []
    for k in range(iters):
        pix = fp.draw(eng.n_window(), n).to(DEV)
        losses.append(float(eng.iteration(camf, depth, color, pix, opt, best=best, lr_quat=lr_quat,
                                          best_before_step=True)))
        after.append(camf.detach().cpu().clone())
        d = rel_l2(after[k] - cam0, after_ref[k] - cam0.numpy())
        print(f"iteration {k}: loss {losses[k]:.6f} (reference {fx['track2.losses'][k]:.6f}), displacement rel-L2 {d:.2e}")
        assert d < 1e-2, k
    np.testing.assert_allclose(losses, fx["track2.losses"], rtol=2e-4)
    kb = int(fx["track2.best_iter"])
    assert np.array_equal(fx["track2.candidate"], tops[kb]) and int(np.argmin(losses)) == kb
    assert abs(float(best[0]) - losses[kb]) == 0.0
    got = best[1].cpu()
    assert rel_l2(got - cam0, tops[kb] - cam0.numpy()) < 1e-2
    # the camera before that iteration's step (ours, bit for bit), not the one after it
    before = cam0 if kb == 0 else after[kb - 1]
    assert torch.equal(got, before) and not torch.equal(got, after[kb])
    # the quaternion moved with its own, smaller rate: Adam's first step is lr·sign(g) per element
    step0 = (after[0] - cam0).abs()
    assert float(step0[:4].max()) < 1.01 * lr_quat < 0.5 * float(step0[4:].max())


def _engine_trace(tiny, pixs, cam0, **kw):
    scn = Scene(tiny)
    slam = scn.slam(base_cfg())
    te = P.engine.TrackingEngine(copy.deepcopy(slam.shared_decoders), slam.shared_c, scn.bound, 32, 16,
                                 (scn.H, scn.W), (scn.fx, scn.fy, scn.cx, scn.cy), ignore_edge=(20, 20),
                                 w_color=0.5, handle_dynamic=True, use_color=True, device=DEV)
    cam = cam0.clone().requires_grad_(True)
    opt = P.ops.FusedAdam([{"params": [cam], "lr": 0.003}])
    best = (torch.full((), float("inf"), dtype=torch.float64, device=DEV), cam0.clone())
    trace = []
    for pix in pixs:
        loss = te.iteration(cam, scn.depth.cuda(), scn.color.cuda(), (pix % te.n_window()).cuda(), opt, best=best,
                            **kw)
        trace.append(torch.cat([cam.detach(), cam.grad.detach(), *opt.state_of(cam)]).clone())
        trace.append(loss.detach().clone().view(1))
    return trace + [best[0].clone().view(1), best[1].clone()]


def test_cam_grad_step_lr2_reduces_to_cam_grad_step(tiny):
    """nslam_cam_grad_step_lr2 with lr_quat == lr and best_before_step = 0 gives nslam_cam_grad_step's bits (200
    rays × 48 samples, 6 iterations): the camera, the gradient, the Adam moments and step count, the loss, the
    best pose and the best loss.  With best_before_step the best pose alone changes."""
    cam0 = P.common.get_tensor_from_camera(Scene(tiny).c2w).cuda()
    cam0[4:] += torch.tensor([0.02, -0.01, 0.015], device=DEV)
    gen = torch.Generator().manual_seed(9)
    pixs = [torch.randint(400, (200,), generator=gen) for _ in range(6)]
    old = _engine_trace(tiny, pixs, cam0)
    new = _engine_trace(tiny, pixs, cam0, lr_quat=0.003, best_before_step=False)
    assert float(old[0][7:14].abs().sum()) > 0 and not torch.equal(old[0][:7], cam0)  # a gradient; the camera moved
    assert len(old) == len(new)
    for a, b in zip(old, new):
        assert torch.equal(a, b), (a - b).abs().max()
    before = _engine_trace(tiny, pixs, cam0, lr_quat=0.003, best_before_step=True)
    for a, b in zip(old[:-1], before[:-1]):
        assert torch.equal(a, b)
    assert not torch.equal(old[-1], before[-1])
    losses = torch.cat(old[1:-2:2])
    kb = int(torch.argmin(losses))
    assert torch.equal(before[-1], cam0 if kb == 0 else old[2 * (kb - 1)][:7]) and torch.equal(old[-1], old[2 * kb][:7])


def test_engine_lr2_needs_the_fused_tail(tiny):
    scn = Scene(tiny)
    slam = scn.slam(base_cfg())
    cam0 = P.common.get_tensor_from_camera(scn.c2w).cuda()
    pix = torch.randint(400, (200,), generator=torch.Generator().manual_seed(9)).cuda()
    for knob in ("cam_tail", "cam_parts"):
        te = P.engine.TrackingEngine(copy.deepcopy(slam.shared_decoders), slam.shared_c, scn.bound, 32, 16,
                                     (scn.H, scn.W), (scn.fx, scn.fy, scn.cx, scn.cy), ignore_edge=(20, 20),
                                     w_color=0.5, handle_dynamic=True, use_color=True, device=DEV)
        setattr(te, knob, False)
        cam = cam0.clone().requires_grad_(True)
        opt = P.ops.FusedAdam([{"params": [cam], "lr": 0.001}])
        with pytest.raises(RuntimeError, match="fused camera tail"):
            te.iteration(cam, scn.depth.cuda(), scn.color.cuda(), pix, opt, lr_quat=0.0002)
        with pytest.raises(RuntimeError, match="fused camera tail"):
            te.iteration(cam, scn.depth.cuda(), scn.color.cuda(), pix, opt, best_before_step=True)
        assert torch.equal(cam.detach(), cam0)  # nothing stepped


def _sep_cfg():
    cfg = base_cfg()
    cfg["tracking"]["seperate_LR"] = True
    return cfg


def test_track_frame_seperate_lr_fused_matches_loop(tiny):
    """Tracker.track_frame with seperate_LR on the TrackingEngine == the autograd loop (fused = False: two Adam
    groups, the candidate before the step), same generator ⇒ same pixel draws."""
    cfg = _sep_cfg()
    sc = Scene(tiny)
    outs = []
    for fused in (False, True):
        tr = P.Tracker(cfg, None, sc.slam(cfg), generator=torch.Generator(device=DEV).manual_seed(4))
        tr.fused = fused
        c2w = torch.cat([sc.c2w, torch.tensor([[0, 0, 0, 1.0]])], 0).cuda()
        pre = c2w.clone()
        pre[:3, 3] += 0.02
        outs.append(tr.track_frame(1, sc.color.cuda(), sc.depth.cuda(), c2w, pre_c2w=pre))
        assert len(tr._graphs) == 0
    print("fused vs loop, max abs", float((outs[0] - outs[1]).abs().max()))
    assert torch.allclose(outs[0], outs[1], atol=5e-4), (outs[0] - outs[1]).abs().max()
    assert not torch.equal(outs[1][:3, 3], pre[:3, 3])  # the loop moved the pose


def test_track_frame_seperate_lr_graph_matches_eager(tiny):
    """seperate_LR without a generator: the camera loop is one captured hipGraph (device draws), equal bit for bit
    to the same engine calls run eagerly on the same draw stream, on the capturing frame and on a replay; the
    eager replica keeps the pre-step camera as the best."""
    cfg = _sep_cfg()
    sc = Scene(tiny)
    c2w = torch.cat([sc.c2w[:3], torch.tensor([[0, 0, 0, 1.0]])], 0).cuda()
    pres = []
    for d in (0.02, -0.015):
        pre = c2w.clone()
        pre[:3, 3] += d
        pres.append(pre)
    tr = P.Tracker(cfg, None, sc.slam(cfg))
    assert tr.seperate_LR and tr.fused and tr.graphs
    tr._draw_seed = 77
    got = [tr.track_frame(k + 1, sc.color.cuda(), sc.depth.cuda(), c2w, pre_c2w=pre) for k, pre in enumerate(pres)]
    assert len(tr._graphs) == 1
    tr2 = P.Tracker(cfg, None, sc.slam(cfg))
    tr2.update_para_from_mapping()
    eng = tr2.engine()
    lr = cfg["tracking"]["lr"]
    ref = []
    for pre in pres:
        cam = P.ops.cam_vector_batch(pre[None].contiguous(), torch.empty(1, 7, device="cuda"))[0]
        start = cam.clone()
        cam = cam.clone().requires_grad_(True)
        opt = P.ops.FusedAdam([{"params": [cam], "lr": lr}])
        best, best_loss = cam.detach().clone(), torch.full((), float("inf"), dtype=torch.float64, device="cuda")
        for it in range(cfg["tracking"]["iters"]):
            before = cam.detach().clone()
            loss = eng.iteration(cam, sc.depth.cuda(), sc.color.cuda(), None, opt, n=cfg["tracking"]["pixels"], seed=77,
                                 lr_quat=lr * 0.2)
            if it == 0:  # Adam's first step is rate·sign(g): the quaternion's is a fifth of the translation's
                step0 = (cam.detach() - start).abs()
                assert float(step0[:4].max()) < 1.01 * lr * 0.2 < 0.5 * float(step0[4:].max())
            better = loss < best_loss
            best_loss = torch.where(better, loss, best_loss)
            best = torch.where(better, before, best)
        pose = torch.eye(4, device="cuda")
        P.ops.cam_pose(best.contiguous(), pose[:3])
        ref.append(pose)
    for a, b in zip(got, ref):
        assert torch.equal(a, b), (a - b).abs().max()
    assert not torch.equal(got[0], pres[0])
