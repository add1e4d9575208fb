"""GPU parity of the loop-level pieces against vectors the REFERENCE's own code produced
(tests/golden/loop_fixtures.npz, tests/golden/make_golden_loop.py):

  nslam_cam_pose / nslam_cam_grad      vs get_camera_from_tensor + get_rays_from_uv + pts (a2, a3)
  nslam_render_loss TRACKER / MAPPER   vs Tracker.py:110-125 / Mapper.py:487-503 (a13, a14)
  Tracker.optimize_cam_in_batch        vs Tracker.py:71-128, 3 iterations (drop-in and TrackingEngine)
  Mapper.optimize_map                  vs Mapper.py:230-540: frustum selection, overlap keyframe
                                       selection, BA over a 5-frame window (a16, a17, f3)
  mapper.frustum_mask / overlap scores vs Mapper.py:93-228 at room0 shapes, on the device

Tolerances: forward quantities as tests/test_gpu_parity.py; multi-iteration loops (Adam
normalises every gradient, so fp32-level differences in tiny gradient entries become lr-sized
steps) as tests/test_gpu_dropins.py: losses rtol 2e-3 (mapper) / 2e-4 (tracker), parameter
updates rel-L2 1e-3 (mapper, BA window: measured <= 8e-5 on MI355X) / 1e-2 (tracker).
"""
import importlib
import json
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, FixedPixels, rel_l2

sys.path.insert(0, GOLDEN)
import scenes  # noqa: E402

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")


def test_cam_pose_matches_reference(loop):
    cams = torch.from_numpy(loop["camera.cam"]).to(DEV)
    ref = torch.from_numpy(loop["camera.c2w"])
    out = torch.empty(3, 4, device=DEV)
    exact, worst = 0, 0.0
    for b in range(cams.shape[0]):
        P.ops.cam_pose(cams[b].contiguous(), out)
        got = out.cpu()
        exact += bool(torch.equal(got, ref[b]))
        worst = max(worst, float((got - ref[b]).abs().max() / ref[b].abs().max()))
    print(f"cam_pose vs reference: {exact}/{cams.shape[0]} bit-identical, worst rel {worst:.2e}")
    assert worst < 1e-6


def test_cam_grad_matches_reference(loop):
    """d loss/d cam for fixed d loss/d pts through the reference's rays + pts chain."""
    B = loop["camera.cam"].shape[0]
    out = torch.empty(7, device=DEV)
    c2w = torch.empty(3, 4, device=DEV)
    worst = 0.0
    for b in range(B):
        cam = torch.from_numpy(loop["camera.cam"][b]).to(DEV)
        P.ops.cam_pose(cam, c2w)
        z = torch.from_numpy(loop["camera.z"][b]).to(DEV).contiguous()
        gp = torch.from_numpy(loop["camera.g_pts"][b]).to(DEV).reshape(-1, 3).contiguous()
        rd = torch.from_numpy(loop["camera.rays_d"][b]).to(DEV).contiguous()
        P.ops.cam_grad(cam, c2w, gp, z, rd, out)
        worst = max(worst, rel_l2(out, loop["camera.grad_cam"][b]))
    print(f"cam_grad vs reference: worst rel-L2 {worst:.2e}")
    assert worst < 1e-5


@pytest.mark.parametrize("case,mode,hd,use_color,w", [("tloss_hd", "tracker", True, True, 0.5),
                                                       ("tloss_nohd", "tracker", False, True, 0.5),
                                                       ("mloss_color", "mapper", False, True, 0.2),
                                                       ("mloss_middle", "mapper", False, False, 0.2)])
def test_render_loss_matches_reference(loop, case, mode, hd, use_color, w):
    raw = torch.from_numpy(loop[case + ".raw"]).to(DEV)
    z = torch.from_numpy(loop[case + ".z"]).to(DEV)
    gd = torch.from_numpy(loop[case + ".gt_depth"]).to(DEV)
    gc = torch.from_numpy(loop[case + ".gt_color"]).to(DEV)
    _, _, _, ray_loss, g_raw = P.ops.render_loss(raw, z, gd, gc, None, mode=mode, use_color=use_color,
                                                 handle_dynamic=hd, w_color=w)
    ref = float(loop[case + ".loss"])
    got = float(ray_loss.sum())
    assert abs(got - ref) <= 1e-6 * abs(ref), (got, ref)
    gref = torch.from_numpy(loop[case + ".g_raw"])
    assert float((g_raw.cpu() - gref).abs().max()) <= 1e-6 * max(1.0, float(gref.abs().max()))


# ------------------------------------------------------------------------------------------------
# drop-in loops on the tiny scene
# ------------------------------------------------------------------------------------------------
def tiny_slam(tiny, cfg, cam):
    bound = torch.from_numpy(tiny["bound"])
    sd = {k[3:]: torch.from_numpy(v) for k, v in tiny.items() if k.startswith("sd.") and not k.startswith("sd.coarse")}
    nice = P.NICE(c_dim=32, coarse=False, middle_grid_len=0.64, fine_grid_len=0.32, color_grid_len=0.32)
    nice.load_state_dict(sd)
    nice.set_bound(bound)
    grids = {k: torch.from_numpy(tiny[k]).to(DEV).contiguous(memory_format=torch.channels_last_3d)
             for k in ("grid_middle", "grid_fine", "grid_color")}
    s = SimpleNamespace(nice=True, bound=bound, H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"],
                        cy=cam["cy"], shared_decoders=nice.to(DEV), shared_c=grids,
                        estimate_c2w_list=torch.zeros(4, 4, 4), gt_c2w_list=torch.zeros(4, 4, 4),
                        mapping_idx=torch.zeros(1).int())
    s.renderer = P.Renderer(cfg, None, s)
    return s


def loop_cfg(frustum=True, pixels=1000, window=5):
    from test_gpu_dropins import base_cfg
    cfg = base_cfg()
    m = cfg["mapping"]
    m.update(pixels=pixels, mapping_window_size=window, frustum_feature_selection=frustum)
    return cfg


def test_tracker_loop_matches_reference(tiny, loop, monkeypatch):
    cam = scenes.TINY_CAM
    b, _, cur = scenes.tiny_window()
    depth = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=int(loop["track.depth_seed"]))).to(DEV)
    color = torch.from_numpy(scenes.color_image(cam, seed=int(loop["track.color_seed"]))).to(DEV)
    cfg = loop_cfg()
    cam0 = torch.from_numpy(loop["track.cam0"])
    # (1) the autograd drop-in, Tracker.optimize_cam_in_batch
    monkeypatch.setattr(P.common, "select_uv", FixedPixels(int(loop["track.draw_seed"])))
    tr = P.Tracker(cfg, None, tiny_slam(tiny, cfg, cam))
    tr.update_para_from_mapping()
    camt = cam0.to(DEV).clone().requires_grad_(True)
    opt = torch.optim.Adam([camt], lr=0.001)
    grads, cams, losses = [], [], []
    step = opt.step

    def step_rec(*a, **k):
        grads.append(camt.grad.detach().cpu().clone())
        return step(*a, **k)

    opt.step = step_rec
    for _ in range(3):
        losses.append(tr.optimize_cam_in_batch(camt, color, depth, 200, opt))
        cams.append(camt.detach().cpu().clone())
    ref_l, ref_g, ref_c = loop["track.losses"], loop["track.grads"], loop["track.cams"]
    np.testing.assert_allclose(losses, ref_l, rtol=2e-4)
    assert rel_l2(grads[0], ref_g[0]) < 1e-3
    for k in range(3):
        assert rel_l2(cams[k] - cam0, ref_c[k] - cam0.numpy()) < 1e-2, k
    # (2) the fused TrackingEngine on the same draws (select_uv indices into the cropped window)
    fp = FixedPixels(int(loop["track.draw_seed"]))
    eng = P.engine.TrackingEngine(tr.decoders, {k: v for k, v in tr.c.items()}, tr.bound, 32, 16,
                                  (cam["H"], cam["W"]), (cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                                  ignore_edge=(20, 20), w_color=0.5, handle_dynamic=True, use_color=True, device=DEV)
    camf = cam0.to(DEV).clone().requires_grad_(True)
    fopt = P.ops.FusedAdam([{"params": [camf], "lr": 0.001}])
    flosses = []
    for k in range(3):
        pix = fp.draw(eng.n_window(), 200).to(DEV)
        flosses.append(float(eng.iteration(camf, depth, color, pix, fopt)))
        assert rel_l2(camf.detach().cpu() - cam0, ref_c[k] - cam0.numpy()) < 1e-2, k
    np.testing.assert_allclose(flosses, ref_l, rtol=2e-4)


def test_mapper_loop_matches_reference(tiny, loop, monkeypatch):
    """optimize_map with frustum feature selection, overlap keyframe selection and BA over a
    5-frame window (4 cameras optimised, the oldest fixed): losses of all 8 iterations (middle →
    fine → colour), the selected keyframes, the updated grids / colour decoder / poses."""
    cam = scenes.TINY_CAM
    b, poses, cur = scenes.tiny_window()
    cfg = loop_cfg(frustum=True, pixels=1000, window=5)
    slam = tiny_slam(tiny, cfg, cam)
    g0 = {k: v.detach().cpu().clone() for k, v in slam.shared_c.items()}
    mp = P.Mapper(cfg, None, slam)
    mp.BA = True
    mp.loss_history = []
    sel = []
    orig_sel = mp.keyframe_selection_overlap

    def sel_rec(*a, **k):
        out = orig_sel(*a, **k)
        sel.append([int(x) for x in out])
        return out

    mp.keyframe_selection_overlap = sel_rec
    kf = []
    for k, p in enumerate(poses):
        kf.append({"gt_c2w": torch.from_numpy(p), "idx": 5 * k, "est_c2w": torch.from_numpy(p).clone(),
                   "depth": torch.from_numpy(scenes.box_depth(p, cam, b, seed=100 + k)),
                   "color": torch.from_numpy(scenes.color_image(cam, seed=200 + k))})
    cur_depth = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=150))
    cur_color = torch.from_numpy(scenes.color_image(cam, seed=250))
    monkeypatch.setattr(P.common, "select_uv", FixedPixels(int(loop["map.draw_seed"])))
    np.random.seed(int(loop["map.np_seed"]))
    n = int(loop["map.n_iters"])
    out = mp.optimize_map(n, 1.0, 30, cur_color, cur_depth, torch.from_numpy(cur), kf, [5 * k for k in range(5)],
                          torch.from_numpy(cur).clone())
    torch.cuda.synchronize()
    assert sel[0] == [int(x) for x in loop["map.selected"]]
    losses = [float(x) for x in mp.loss_history]
    np.testing.assert_allclose(losses, loop["map.losses"], rtol=2e-3)
    report = {}
    for k in ("grid_middle", "grid_fine", "grid_color"):
        d_got = slam.shared_c[k].detach().cpu() - g0[k]
        d_ref = torch.from_numpy(loop["map.grid_out." + k]) - g0[k]
        report[k] = rel_l2(d_got, d_ref)
        # frustum selection: voxels outside the reference's mask are untouched
        mask = torch.from_numpy(loop["map.mask." + k]).permute(2, 1, 0)[None, None].expand_as(d_got)
        assert float(d_got[~mask].abs().max()) == 0.0, k
    sd = mp.decoders.color_decoder.state_dict()
    d_got = torch.cat([sd[k].detach().cpu().reshape(-1) for k in sd])
    d_ref = torch.cat([torch.from_numpy(loop["map.color_decoder_out." + k]).reshape(-1) for k in sd])
    d0 = torch.cat([torch.from_numpy(tiny["sd.color_decoder." + k]).reshape(-1) for k in sd])
    report["color_decoder"] = rel_l2(d_got - d0, d_ref - d0)
    # poses: the 4 optimised cameras moved as the reference's did, the oldest did not move
    oldest = min(int(x) for x in loop["map.selected"])
    for k in range(5):
        got = kf[k]["est_c2w"].detach().cpu()
        ref = torch.from_numpy(loop[f"map.est_c2w_out.{k}"])
        start = torch.from_numpy(poses[k])
        if k == oldest or (k not in [int(x) for x in loop["map.selected"]] and k != 4):
            assert torch.equal(got, start), k
            continue
        report[f"pose{k}"] = rel_l2(got - start, ref - start)
    report["cur"] = rel_l2(out.detach().cpu() - torch.from_numpy(cur), loop["map.cur_c2w_out"] - cur)
    print(json.dumps(report, indent=1))
    # (measured on MI355X: grids <= 1.9e-5, colour decoder 5.8e-7, poses <= 4.5e-6)
    assert all(v < 1e-3 for v in report.values()), report


def test_frustum_mask_device_matches_reference(loop):
    b, _, cur = scenes.room0_window()
    cam = scenes.ROOM0_CAM
    depth = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=int(loop["frustum.depth_seed"]))).to(DEV)
    for key in ("grid_middle", "grid_fine", "grid_color"):
        shp = tuple(int(v) for v in loop["frustum.shape." + key])
        m = P.mapper.frustum_mask(torch.from_numpy(cur).to(DEV), key, shp, depth, torch.from_numpy(b), cam["H"],
                                  cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        ref = loop["frustum.mask." + key]
        bad = int((m.cpu().numpy() != ref).sum())
        print(f"frustum {key}: {bad} of {ref.size} voxels differ ({int(ref.sum())} selected)")
        assert bad == 0, key


def test_keyframe_overlap_device_matches_reference(loop, monkeypatch):
    b, poses, cur = scenes.room0_window()
    cam = scenes.ROOM0_CAM
    depth = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=int(loop["overlap.depth_seed"]))).to(DEV)
    color = torch.from_numpy(scenes.color_image(cam, seed=int(loop["overlap.color_seed"]))).to(DEV)
    kf = [{"est_c2w": torch.from_numpy(p).to(DEV)} for p in poses]
    from test_loop_golden import overlap_mapper
    mp = overlap_mapper(P, DEV)
    monkeypatch.setattr(P.common, "select_uv", FixedPixels(int(loop["overlap.draw_seed"])))
    scores = mp.keyframe_overlap_scores(color, depth, torch.from_numpy(cur).to(DEV), kf)
    # 1600 samples per keyframe: one sample flipping across an image edge moves a score by 1/1600
    np.testing.assert_allclose(scores, loop["overlap.scores"], atol=1.5 / 1600)
    monkeypatch.setattr(P.common, "select_uv", FixedPixels(int(loop["overlap.draw_seed"])))
    np.random.seed(int(loop["overlap.np_seed"]))
    sel = mp.keyframe_selection_overlap(color, depth, torch.from_numpy(cur).to(DEV), kf, int(loop["overlap.k"]))
    assert [int(s) for s in sel] == [int(s) for s in loop["overlap.selected"]]


def test_frustum_rows_kernel_matches_mask(loop):
    """ABI v20 nslam_frustum_rows (the remap, depth tests and compaction in one kernel sequence) at room0
    shapes: its mask equals the reference's get_mask_from_c2w fixture and mapper.frustum_mask (torch) bit
    for bit, on the fixture's pose and on 6 more (random look directions, a zero-depth patch); rows are the
    ascending channels-last nonzeros of that mask, slot their inverse, n_live their count."""
    b, poses, cur = scenes.room0_window()
    cam = scenes.ROOM0_CAM
    bound = torch.from_numpy(b)
    depth0 = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=int(loop["frustum.depth_seed"]))).to(DEV)
    cases = [(torch.from_numpy(cur), depth0, "fixture")]
    g = np.random.default_rng(3)
    ctr = b.mean(1)
    for k in range(6):
        c2w = scenes.look_pose(ctr, float(g.uniform(0, 6.28)), float(g.uniform(-0.4, 0.4)),
                               tuple(float(v) for v in g.uniform(-0.6, 0.6, 3)))
        d = torch.from_numpy(scenes.box_depth(c2w, cam, b, seed=40 + k)).to(DEV)
        if k % 2:
            d[100:200, 300:500] = 0  # zero depths take the maximum over all grid points
        cases.append((torch.from_numpy(c2w), d, f"pose{k}"))
    for key in ("grid_middle", "grid_fine"):
        shp = tuple(int(v) for v in loop["frustum.shape." + key])
        nz, ny, nx = shp
        n = nx * ny * nz
        for c2w, d, name in cases:
            slot = torch.full((n,), -7, dtype=torch.int32, device=DEV)
            rows = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
            n_live = torch.zeros(1, dtype=torch.int64, device=DEV)
            mref = torch.zeros(n, dtype=torch.uint8, device=DEV)
            P.mapper.frustum_rows_device(c2w.to(DEV), shp, d, bound, cam["H"], cam["W"], cam["fx"], cam["fy"],
                                         cam["cx"], cam["cy"], slot, rows, n_live, mask_ref=mref)
            m = P.mapper.frustum_mask(c2w.to(DEV), key, shp, d, bound, cam["H"], cam["W"], cam["fx"], cam["fy"],
                                      cam["cx"], cam["cy"])
            assert torch.equal(mref.bool().reshape(nx, ny, nz), m), (key, name)
            if name == "fixture":
                assert np.array_equal(mref.bool().reshape(nx, ny, nz).cpu().numpy(), loop["frustum.mask." + key])
            want = P.engine.frustum_rows(m)
            k = int(n_live)
            assert k == want.numel() > 0, (key, name)
            assert torch.equal(rows[:k], want), (key, name)
            inv = torch.full((n,), -1, dtype=torch.int32, device=DEV)
            inv[want.long()] = torch.arange(k, dtype=torch.int32, device=DEV)
            assert torch.equal(slot, inv), (key, name)


def _tiny_frustum_case(tiny):
    """frustum_rows_device's arguments on the tiny scene's fine grid, with fresh output buffers."""
    cam = scenes.TINY_CAM
    b, _, cur = scenes.tiny_window()
    depth = torch.from_numpy(scenes.box_depth(cur, cam, b, seed=150)).to(DEV)
    shp = tuple(int(v) for v in tiny["grid_fine"].shape[2:])
    n = shp[0] * shp[1] * shp[2]
    args = (shp, depth, torch.from_numpy(b), cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])

    def buffers():
        slot, rows = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
        return slot, rows, torch.zeros(1, dtype=torch.int64, device=DEV)

    return torch.from_numpy(cur).to(DEV), args, n, buffers


def test_frustum_rows_device_accepts_a_3x4_pose(tiny):
    c2w, args, n, buffers = _tiny_frustum_case(tiny)
    assert c2w.shape == (4, 4)
    out = []
    for pose in (c2w, c2w[:3]):
        slot, rows, n_live = buffers()
        P.mapper.frustum_rows_device(pose, *args, slot, rows, n_live)
        out.append((slot, rows, n_live))
    (s4, r4, n4), (s3, r3, n3) = out
    k = int(n4)
    assert 0 < k < n
    assert torch.equal(n3, n4) and torch.equal(s3, s4) and torch.equal(r3[:k], r4[:k])


@pytest.mark.parametrize("bad", ["short slot", "float rows", "int32 n_live"])
def test_frustum_rows_device_refuses_bad_buffers(tiny, bad):
    """A buffer the kernels would overrun or misread is refused on the host: nothing is launched, nothing written."""
    c2w, args, n, buffers = _tiny_frustum_case(tiny)
    slot, rows, n_live = buffers()
    if bad == "short slot":
        slot = slot[:n - 1]
    elif bad == "float rows":
        rows = rows.float()
    else:
        n_live = n_live.int()
    with pytest.raises(ValueError):
        P.mapper.frustum_rows_device(c2w, *args, slot, rows, n_live)
    torch.cuda.synchronize()
    assert bool((slot == -7).all()) and bool((rows == -7).all()) and int(n_live) == 0


@pytest.mark.parametrize("n", [0, 1, 200, 1000, 5000])
def test_loss_sum_best_matches_torch_and_keeps_the_best_pose(n):
    """ABI v21 nslam_loss_sum_best (the tracker's per-iteration loss and Tracker.py:245-247's best-pose
    bookkeeping in one launch): the sum equals torch's float64 sum to rounding and is the same value on
    every call (fixed order); a lower loss replaces best_loss and the best pose, an equal, higher or NaN
    loss leaves both as they were (torch's comparison)."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5 + n)
    rl = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * 3.0
    out = torch.empty((), dtype=torch.float64, device=dev)
    s1 = float(P.ops.loss_sum_best(rl, out))
    s2 = float(P.ops.loss_sum_best(rl, out))
    ref = float(rl.sum())
    assert s1 == s2
    assert abs(s1 - ref) <= 1e-12 * max(1.0, abs(ref))
    cam = torch.arange(7, dtype=torch.float32, device=dev)
    for best_before, expect_update in ((s1 + 1.0, True), (s1, False), (s1 - 1.0, False), (float("inf"), True)):
        best_loss = torch.full((), best_before, dtype=torch.float64, device=dev)
        best = torch.full((7,), -1.0, dtype=torch.float32, device=dev)
        P.ops.loss_sum_best(rl, out, best_loss, cam, best)
        torch.cuda.synchronize()
        if expect_update:
            assert float(best_loss) == s1 and torch.equal(best, cam)
        else:
            assert float(best_loss) == best_before and bool((best == -1.0).all())
    if n:  # a NaN loss is never better
        rl[0] = float("nan")
        best_loss = torch.full((), float("inf"), dtype=torch.float64, device=dev)
        best = torch.full((7,), -1.0, dtype=torch.float32, device=dev)
        P.ops.loss_sum_best(rl, out, best_loss, cam, best)
        torch.cuda.synchronize()
        assert float(best_loss) == float("inf") and bool((best == -1.0).all())


def _rotations(n, gen):
    """Random rotations, a quarter of them rotated by pi about x / y / z so every branch of the
    trace / largest-diagonal rule is taken (trace <= 0 with r00, r11 or r22 the largest)."""
    q = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    R = P.common.quad2rotation(q)
    flips = [torch.diag(torch.tensor(d, dtype=torch.float64)) for d in ((1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    small = P.common.quad2rotation(q * torch.tensor([1.0, 0.05, 0.05, 0.05], dtype=torch.float64))
    for k in range(n):
        if k % 4:
            R[k] = flips[k % 4 - 1] @ small[k]
    return R


@pytest.mark.parametrize("rows", [3, 4])
def test_cam_vector_batch_matches_camera_tensors(rows):
    """nslam_cam_vector_batch (ABI v22) == common.camera_tensors (the device restatement of the reference's
    get_tensor_from_camera, common.py:179-201) on poses taking every branch, for [n,3,4] and [n,4,4] slots;
    the optional copy equals the output; and cam_pose(cam_vector(c2w)) gives c2w back.  Tolerance: 1 float32
    ulp per entry (|q|² is summed in a fixed order, torch's reduction order is not pinned)."""
    gen = torch.Generator().manual_seed(5)
    n = 64
    R = _rotations(n, gen)
    c2w = torch.zeros(n, rows, 4, dtype=torch.float64)
    c2w[:, :3, :3] = R
    c2w[:, :3, 3] = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    if rows == 4:
        c2w[:, 3, 3] = 1.0
    c2w = c2w.float().to(DEV)
    tr = c2w[:, 0, 0] + c2w[:, 1, 1] + c2w[:, 2, 2]
    assert bool((tr > 0).any()) and bool((tr <= 0).any())
    out = torch.full((n, 7), -9.0, device=DEV)
    cp = torch.full((n, 7), -9.0, device=DEV)
    P.ops.cam_vector_batch(c2w, out, cp)
    ref = P.common.camera_tensors(c2w)
    assert torch.equal(out, cp)
    exact = int((out == ref).all(dim=1).sum())
    print(f"cam_vector_batch: {exact}/{n} bit-identical to camera_tensors")
    assert float((out - ref).abs().max()) <= 2 ** -23
    assert bool((out[:, 0] >= 0).all())
    back = torch.empty(3, 4, device=DEV)
    for k in range(n):
        P.ops.cam_pose(out[k].contiguous(), back)
        assert float((back - c2w[k, :3]).abs().max()) < 1e-5
    # one camera, no copy
    one = torch.empty(1, 7, device=DEV)
    P.ops.cam_vector_batch(c2w[:1].contiguous(), one)
    assert torch.equal(one[0], out[0])
