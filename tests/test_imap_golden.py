"""tests/imap_ref.py (the plain-torch restatement of the iMAP* path) in float32 against the reference's own
outputs, tests/golden/imap_fixtures.*.npz (make_golden_imap.py) — on the CPU.

Tolerance.  The restatement runs the reference's formulas with the same torch operators, so on the generator's
machine it reproduces the fixtures to the last bit or nearly; on another CPU the BLAS and the vectorised reductions
may sum in another order.  Two float32 evaluations of one formula differ by at most about twice one evaluation's
error, which the fixture records per quantity as `floor` (reference float32 against the restatement in float64);
the bar is 4 x floor, and never below 1e-6 (16 float32 epsilons: sums of hundreds of terms in another order).
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imap_ref as ref  # noqa: E402
import imap_scene as sc  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return load_golden("imap_fixtures")


def bar(fx, case, name):
    return max(4.0 * float(fx[f"{case}.floor.{name}"]), 1e-6)


def close(fx, case, name, got):
    err = ref.rel_l2(got.detach(), torch.from_numpy(fx[f"{case}.{name}"]))
    print(f"{case}.{name}: rel_l2 {err:.3e} (bar {bar(fx, case, name):.3e})")
    assert err <= bar(fx, case, name), (case, name, err)


def leaf_sd(weights=sc.weights):
    return {k: torch.from_numpy(v).requires_grad_(True) for k, v in weights().items()}


BOUND = torch.from_numpy(np.asarray(sc.BOUND, dtype=np.float64))


def test_keys_are_the_reference_state_dict():
    assert sorted(sc.weights()) == sorted(ref.KEYS)


def test_mlp(fx):
    sd = leaf_sd()
    p = torch.from_numpy(sc.mlp_points()).requires_grad_(True)
    raw = ref.eval_points(sd, p, BOUND)
    raw.backward(torch.from_numpy(sc.cotangent((p.shape[0], 4), 12)))
    close(fx, "mlp", "raw", raw)
    close(fx, "mlp", "g_p", p.grad)
    for k in ref.KEYS:
        close(fx, "mlp", "g." + k, sd[k].grad)
    assert int((raw[:, 3] == 100).sum()) == int(fx["mlp.n_outside"]) and float(raw[sc.ON_FACE, 3]) == 100.0


@pytest.mark.parametrize("S", [32, 44, 70])
def test_composite(fx, S):
    raw_np, z_np, d_np = sc.composite_inputs(S)
    n = raw_np.shape[0]
    raw, d = torch.from_numpy(raw_np).requires_grad_(True), torch.from_numpy(d_np).requires_grad_(True)
    o = ref.composite_density(raw, torch.from_numpy(z_np), d)
    gd, gv = torch.from_numpy(sc.cotangent(n, 50 + S, np.float64)), torch.from_numpy(sc.cotangent(n, 51 + S, np.float64))
    ((o[0] * gd).sum() + (o[1] * gv).sum() + (o[2] * torch.from_numpy(sc.cotangent((n, 3), 52 + S))).sum()).backward()
    for name, v in zip(("depth", "var", "rgb", "weights", "g_raw", "g_rays_d"), (*o, raw.grad, d.grad)):
        close(fx, f"composite{S}", name, v)


def test_pdf(fx):
    z_np, w_np = sc.pdf_inputs()
    z, w = torch.from_numpy(z_np), torch.from_numpy(w_np)
    mid = .5 * (z[..., 1:] + z[..., :-1])
    close(fx, "pdf", "z_samples", ref.sample_pdf(mid, w[..., 1:-1], sc.N_IMPORTANCE))
    close(fx, "pdf", "z_out", ref.importance_z(z, w, sc.N_IMPORTANCE))


@pytest.mark.parametrize("tag", ["render_gt", "render_nogt"])
def test_render(fx, tag):
    ro_np, rd_np, gt_np = sc.rays(50, 61)
    n = ro_np.shape[0]
    sd = leaf_sd()
    ro, rd = torch.from_numpy(ro_np).requires_grad_(True), torch.from_numpy(rd_np).requires_grad_(True)
    gt = torch.from_numpy(gt_np) if tag == "render_gt" else None
    depth, var, color = ref.render_batch_ray(sd, rd, ro, BOUND, gt, sc.N_SAMPLES, sc.N_IMPORTANCE)
    gd, gv = torch.from_numpy(sc.cotangent(n, 62, np.float64)), torch.from_numpy(sc.cotangent(n, 63, np.float64))
    ((depth * gd).sum() + (var * gv).sum() + (color * torch.from_numpy(sc.cotangent((n, 3), 64))).sum()).backward()
    for name, v in (("depth", depth), ("var", var), ("color", color), ("g_rays_o", ro.grad), ("g_rays_d", rd.grad)):
        close(fx, tag, name, v)
    for k in ref.KEYS:
        close(fx, tag, "g." + k, sd[k].grad)


def test_regulation(fx):
    ro_np, rd_np, gt_np = sc.rays(40, 71, zero_frac=0.0)
    sd = leaf_sd()
    sigma = ref.regulation(sd, torch.from_numpy(rd_np), torch.from_numpy(ro_np), torch.from_numpy(gt_np), BOUND,
                           sc.N_SAMPLES, torch.from_numpy(fx["regulation.t_rand"]))
    sigma.abs().sum().backward()
    close(fx, "regulation", "sigma", sigma)
    for k in ("embedder._B", "output_linear.weight"):
        close(fx, "regulation", "g." + k, sd[k].grad)


def _frames():
    c2w, depth, color = sc.frames()
    return [(torch.from_numpy(c2w[k]), torch.from_numpy(depth[k]), torch.from_numpy(color[k])) for k in range(2)]


def _quat(c2w):
    import importlib
    P = importlib.import_module("nice-slam_amd")
    return P.common.get_tensor_from_camera(c2w)


@pytest.mark.parametrize("tag", ["map", "map_ba"])
def test_map_loop(fx, tag):
    """The loop's bars are the same 4 x floor: the floors of the updates are large (up to 1e-2) because Adam's
    first steps are sign-like, so a noise-level gradient that flips its sign moves the parameter by a full step."""
    fr = _frames()
    sd = leaf_sd(sc.loop_weights)
    draws = torch.from_numpy(fx[f"{tag}.draws"])
    t_rand = torch.from_numpy(fx[f"{tag}.t_rand"])
    ba = tag == "map_ba"
    losses, camt = ref.map_loop(sd, BOUND, sc.CAM, fr, fr[1], [(draws[2 * i], draws[2 * i + 1]) for i in range(sc.MAP_ITERS)],
                                list(t_rand), sc.MAP_ITERS, sc.MAP_LR, sc.MAP_W_COLOR, sc.N_SAMPLES, sc.N_IMPORTANCE,
                                ba_cam=_quat(fr[1][0]) if ba else None, ba_lr=sc.BA_CAM_LR)
    close(fx, tag, "losses", torch.tensor(losses, dtype=torch.float64))
    init = sc.loop_weights()
    for k in ref.KEYS:
        close(fx, tag, "update." + k, torch.from_numpy(sc.probe(k, sd[k].detach().numpy() - init[k])))
    if ba:
        close(fx, tag, "c2w_update", ref.camera_matrix(camt) - fr[1][0][:3])


def test_track_loop(fx):
    fr = _frames()
    sd = {k: torch.from_numpy(v) for k, v in sc.loop_weights().items()}
    cam0 = torch.from_numpy(fx["track.cam0"])
    losses, camt = ref.track_loop(sd, BOUND, sc.CAM, fr[1], cam0, list(torch.from_numpy(fx["track.draws"])),
                                  sc.TRACK_ITERS, sc.TRACK_LR, sc.TRACK_W_COLOR, sc.TRACK_EDGE, sc.N_SAMPLES,
                                  sc.N_IMPORTANCE)
    close(fx, "track", "losses", torch.tensor(losses, dtype=torch.float64))
    close(fx, "track", "cam_update", camt - cam0)
