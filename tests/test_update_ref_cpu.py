"""The update chain's float64 restatements (tests/update_ref.py) against each other, the floors the GPU tests
(test_gpu_update_edges.py) use, and the conditions those tests rely on — all on the references alone, no GPU.
Run with -s to see the floors."""
import numpy as np
import pytest
import torch

import update_ref as ur


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def _cpu_inputs(c):
    """float32 pose and rays_d of a camera case, as the GPU tests hand them to the kernel."""
    c2w = ur.camera_pose(c["cam"])
    return c2w, ur.rays_of(c2w, c["dirs"])


@pytest.mark.parametrize("n,S", [(1, 1), (21, 48), (683, 3), (1025, 32)])
@pytest.mark.parametrize("quat", sorted(ur.QUATS))
def test_cam_grad_ref_matches_chain_autograd(quat, n, S):
    """cam_grad_ref on the float32 pose and rays_d == float64 autograd through the whole chain, to the project's
    1e-5 rel-L2 (the float32 inputs differ from float64 by rounding; measured <= 8.7e-7).  Also prints the
    camera floor: the chain in float32 against float64."""
    q = ur.QUATS[quat]
    qq = float((q.float().double() ** 2).sum())
    assert {"tiny": 0.5e-4 < qq < 2e-4, "unit": qq == 1.0, "big": 7 < qq < 9, "negw": float(q[0]) < 0}[quat]
    c = ur.cam_case(n, S, 2, quat)
    gp = c["g_pts"][0] + c["g_pts"][1]
    chain64, _, _ = ur.camera_chain_autograd(c["cam"], c["dirs"], c["z"], gp, torch.float64)
    chain32, c2w, rd = ur.camera_chain_autograd(c["cam"], c["dirs"], c["z"], gp, torch.float32)
    ref = ur.cam_grad_ref(c["cam"], c2w, c["g_pts"], c["z"], rd)
    err, floor = rel_l2(ref, chain64), rel_l2(chain32, chain64)
    print(f"cam {quat} ({n},{S}): cam_grad_ref vs chain64 {err:.2e}; floor chain32 vs chain64 {floor:.2e}")
    assert err <= 1e-5
    assert floor <= 1e-5


def _parts_nonzero(ref):
    return float(ref[:4].norm()) > 0 and float(ref[4:].norm()) > 0 and bool(torch.isfinite(ref).all())


def test_camera_cases_have_nonzero_gradient_parts():
    """Every one-camera, batch and tail case of the GPU tests: both parts of the reference gradient are non-zero
    (a bar relative to max|ref_part| means something), and NaN sits only in a batch's gap."""
    for n, S in ur.CAM_SHAPES:
        for nbuf in ur.cam_buffers(n, S):
            c = ur.cam_case(n, S, nbuf, ur.cam_quat_of(n, S))
            c2w, rd = _cpu_inputs(c)
            assert _parts_nonzero(ur.cam_grad_ref(c["cam"], c2w, c["g_pts"], c["z"], rd)), (n, S, nbuf)
    for n_cams, n_per, S, nbuf, _ in ur.BATCH_CASES:
        c = ur.batch_case(n_cams, n_per, S, nbuf)
        assert sorted(c["ray_begin"]) != c["ray_begin"] or n_cams == 1
        assert min(c["ray_begin"]) == 0 or n_cams == 1 and c["ray_begin"] == [ur.BATCH_GAP]
        assert int(torch.isnan(c["z"]).any(1).sum()) == ur.BATCH_GAP
        assert len({float(q.norm()) for q in c["cams"][:, :4]}) == n_cams
        for k in range(n_cams):
            rays, pts = ur.batch_slice(c, k)
            cam = c["cams"][k]
            c2w = ur.camera_pose(cam)
            ref = ur.cam_grad_ref(cam, c2w, [b[pts] for b in c["g_pts"]], c["z"][rays], ur.rays_of(c2w, c["dirs"][rays]))
            assert _parts_nonzero(ref), (n_cams, n_per, S, k)
    for n, S in ur.TAIL_SHAPES:
        c = ur.tail_case(n, S, 257)
        c2w, rd = _cpu_inputs(c)
        for gp in c["g_pts"]:
            ref = ur.cam_grad_ref(c["cam"], c2w, gp, c["z"], rd)
            assert _parts_nonzero(ref) and float(ref.abs().min()) > 1e-3  # (|g| >> eps: the first step moves by lr)


@pytest.mark.parametrize("n_loss", ur.TAIL_LOSS_LENGTHS)
def test_tail_loss_sequence(n_loss):
    """The tail case's losses improve at iterations 0 and 2, tie at 3 (bit-equal sums) and are NaN at 4; without
    rays every loss is 0: the first improves on the start value, the others tie."""
    c = ur.tail_case(21, 48, n_loss)
    g = [torch.ones(7)] * ur.K_STEPS
    for before in (False, True):
        r = ur.cam_tail_ref(c["cam"], g, c["ray_loss"], ur.TAIL_LR, 4 * ur.TAIL_LR, before)
        if n_loss == 0:
            assert r["set_at"] == [0] and r["loss"] == [0.0] * ur.K_STEPS
            continue
        assert r["set_at"] == [0, 2]
        assert r["loss"][3] == r["loss"][2] and np.isnan(r["loss"][4]) and r["loss"][5] > r["loss"][2]
        assert r["best_loss"][-1] == r["loss"][2]
        # the pose kept: the camera after step 2, or the one before it (= after step 1)
        assert torch.equal(r["best"][-1], r["cam"][1 if before else 2])
    # two rates: after the first step elements 0..3 have moved by lr_quat, 4..6 by lr
    r = ur.cam_tail_ref(c["cam"], g, c["ray_loss"], ur.TAIL_LR, 4 * ur.TAIL_LR, False)
    moved = (r["cam"][0] - c["cam"].double()).abs()
    assert torch.allclose(moved[:4], torch.full((4,), 4 * ur.TAIL_LR, dtype=torch.float64), rtol=1e-3, atol=0)
    assert torch.allclose(moved[4:], torch.full((3,), ur.TAIL_LR, dtype=torch.float64), rtol=1e-3, atol=0)


@pytest.mark.parametrize("name", sorted(ur.ADAM_CASES))
def test_adam_floors_and_movement(name):
    """Prints the case's floors (torch's float32 Adam against float64 Adam; nothing of the code under test) and
    checks that every element with a gradient moves by more than 100 x its bar (= 4 x floor), so a missed or
    misplaced element cannot pass; elements that never get one do not move in the reference either."""
    refs, floors = ur.adam_expect(name)
    print(f"adam {name}: floors p {floors['p']:.2e}  exp_avg {floors['exp_avg']:.2e}  exp_avg_sq {floors['exp_avg_sq']:.2e}")
    assert all(f > 0 for f in floors.values())
    for s, r in zip(ur.adam_case(name), refs):
        p0 = ur.rows_view(s["p0"])[s["rows"].long()] if s["rows"] is not None else s["p0"]
        moved = (r["p"] - p0.double()).abs().reshape(-1)
        live = ur.adam_live_mask(s)
        assert r["steps"] == sum(g is not None for g in s["grads"]) > 0
        assert float(moved[live].min()) > 100 * 4 * floors["p"], (name, s["name"], float(moved[live].min()))
        assert float(moved[~live].max() if (~live).any() else 0.0) == 0.0
        if s["rows"] is not None:
            assert s["rows"].tolist() != sorted(s["rows"].tolist()) or s["rows"].numel() == 1
            assert len(set(s["rows"].tolist())) == s["rows"].numel()


def test_adam_case_shapes():
    assert len(ur.adam_case("seg_limit")) == 16 and len(ur._case_seg_limit(17)) == 17
    kinds = {(s["kind"], s.get("compact")) for s in ur.adam_case("seg_limit")}
    assert kinds == {("dense", None), ("rows", True), ("rows", False)}
    s = ur.adam_case("grad_scale")[0]
    e = torch.arange(2049)
    assert all(float(g[e % 7 == 0].abs().max()) == 0 for g in s["grads"])
    assert float(s["grads"][1][e % 7 == 3].abs().min()) > 0 and float(s["grads"][2][e % 7 == 3].abs().max()) == 0
    # eps dominates: sqrt(v_hat) <= 1.5e-12 << 1e-8
    assert max(float(g.abs().max()) for g in s["grads"]) <= 1.5e-12
    cap = ur.adam_case("n_live")[0]
    assert cap["rows"].numel() == ur.N_LIVE_CAP == int(np.prod(ur.N_LIVE_ZYX))
    idx = ur.mirror_index(1025, 3000)
    both = ((idx[:, 0] >= 0) & (idx[:, 1] >= 0)).sum()
    none = ((idx[:, 0] < 0) & (idx[:, 1] < 0)).sum()
    used = idx[idx >= 0]
    assert both > 0 and none > 0 and ((idx[:, 0] >= 0) ^ (idx[:, 1] >= 0)).sum() > 0
    assert used.unique().numel() == used.numel() and int(used.max()) < 3000


def test_float32_betas_note():
    """The kernel's betas are floats and it forms 1 - beta in float32: exp_avg_sq of exact Adam at the rounded
    betas sits 1.3e-5 (relative) from Adam at (0.9, 0.999), far above a float32 floor — hence the moments'
    reference at BETAS_F32, while the parameters agree with either (the bias correction cancels it)."""
    s = ur.adam_case("dense")[4]
    p_a, _, v_a, _ = ur.adam_ref(s["p0"], s["grads"], s["lr"], betas=ur.BETAS)
    p_b, _, v_b, _ = ur.adam_ref(s["p0"], s["grads"], s["lr"], betas=ur.BETAS_F32)
    rel_v = float(((v_a - v_b).abs() / v_a).max())
    print(f"exp_avg_sq, rounded against exact betas: {rel_v:.2e} relative; parameters {float((p_a - p_b).abs().max()):.2e}")
    assert 1e-5 < rel_v < 2e-5
    assert float((p_a - p_b).abs().max()) < 1e-7
    assert float(np.float32(1) - np.float32(0.999)) == 1.0 - ur.BETAS_F32[1]
