#!/usr/bin/env python3
"""Rendering metrics at the Replica frame (680 x 1200 x 3): ms per call, against torch and against one render.

    python tools/metrics_bench.py [--repeat 20] [--out profiles/render_eval.json]

Each line is the median of `--repeat` device-event timings after a warm-up call:
  image_errors, ssim_1, ssim_5   ops.image_errors, ops.ssim with one and five levels (csrc/nslam_metrics.hip)
  render_metrics                 one evaluation.render_metrics call: both kernels and the download of its 34 doubles
  torch_*                        the same metrics written with F.conv2d / F.avg_pool2d (float32, the separable
                                 window as two grouped convolutions) and masked sums on the same device
  render_img                     one Renderer.render_img of a room0-size map (random grids and decoders: the time
                                 does not depend on what the map holds), the frame the metrics are taken of
The traffic floor of the level-0 pass (both images read once) is printed beside its time.  The values of both
implementations are compared, so a faster number is a number for the same result.
A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import scenes  # noqa: E402

HBM_PEAK = 8.0e12
CFG = {
    "coarse": False, "scale": 1, "occupancy": True, "verbose": False,
    "cam": dict(scenes.ROOM0_CAM, crop_edge=0),
    "grid_len": {"coarse": 2.0, "middle": 0.32, "fine": 0.16, "color": 0.16, "bound_divisible": 0.32},
    "mapping": {"bound": scenes.ROOM0_BOUND},
    "model": {"c_dim": 32, "coarse_bound_enlarge": 2, "pos_embedding_method": "fourier"},
    "data": {"dim": 3},
    "rendering": {"N_samples": 32, "N_surface": 16, "N_importance": 0, "lindisp": False, "perturb": 0.0},
}
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def timed(fn, repeat):
    """Median device-event milliseconds of fn() after one warm-up call; returns (ms, last result)."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def torch_window(dev):
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).float().to(dev)


def torch_ssim(x, y, g, levels, L=1.0):
    """x, y [B,C,H,W] float32 → [B,levels,C,2] float64: the means of the SSIM and CS maps, as ops.ssim defines them."""
    C = x.shape[1]
    kx, ky = g.reshape(1, 1, 1, 11).repeat(C, 1, 1, 1), g.reshape(1, 1, 11, 1).repeat(C, 1, 1, 1)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2

    def blur(a):
        return F.conv2d(F.conv2d(a, kx, groups=C), ky, groups=C)
    out = []
    for l in range(levels):
        if l:
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
        mx, my = blur(x), blur(y)
        sx, sy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        cs = (2 * sxy + C2) / (sx + sy + C2)
        ss = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
        out.append(torch.stack([ss.double().mean((2, 3)), cs.double().mean((2, 3))], -1))
    return torch.stack(out, 1)


def torch_errors(color, gt_color, depth, gt_depth):
    """[4] float64 on the device: ops.image_errors(mask="depth", clamp=True) for one image."""
    valid = gt_depth > 0
    d = (color.clamp(0, 1).double() - gt_color.double()) * valid[..., None]
    return torch.stack([(d * d).sum(), valid.sum() * 3.0, ((depth.double() - gt_depth.double()).abs() * valid).sum(),
                        valid.sum().double()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_eval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: no HIP device; nothing here can be measured on the CPU")
    P = importlib.import_module("nice-slam_amd")
    ops, dev = P.ops, torch.device("cuda:0")
    cam = scenes.ROOM0_CAM
    H, W = cam["H"], cam["W"]
    # the frame: one render of a room0-size map against a synthetic ground truth
    from types import SimpleNamespace
    gen = torch.Generator().manual_seed(3)
    bound = P.slam.load_bound(CFG)
    grids = P.slam.grid_init(CFG, bound, dev, generator=gen)
    decoders = P.slam.build_decoders(CFG, bound, dev)
    renderer = P.Renderer(CFG, None, SimpleNamespace(nice=True, bound=bound, **cam))
    b = scenes.enlarge_bound(scenes.ROOM0_BOUND, 0.32)
    c2w = scenes.look_pose(b.mean(1), 0.75, 0.5)
    gt_depth = torch.from_numpy(scenes.box_depth(c2w, cam, b, seed=1).astype(np.float32)).to(dev)
    gt_color = torch.from_numpy(scenes.color_image(cam, seed=2).astype(np.float32)).to(dev).contiguous()
    pose = torch.from_numpy(np.asarray(c2w, dtype=np.float32)).to(dev)
    ms_render, (depth, _, color) = timed(
        lambda: renderer.render_img(grids, decoders, pose, dev, stage="color", gt_depth=gt_depth), max(3, a.repeat // 4))
    # a rendered image near its ground truth (the regime the metrics are used in), colours leaving [0,1] in places
    noise = torch.randn(H, W, 3, generator=gen).to(dev)
    color = (gt_color + 0.05 * noise).contiguous()
    depth = (gt_depth + 0.01 * noise[..., 0]).float().contiguous()
    cb, gb, db, gdb = color[None], gt_color[None], depth[None], gt_depth[None]
    clamped = cb.clamp(0, 1)
    out = {"image": [H, W, 3], "repeat": a.repeat, "ms": {"render_img": round(ms_render, 4)}}
    ms = out["ms"]
    ms["image_errors"], err = timed(lambda: ops.image_errors(cb, gb, db, gdb, mask="depth"), a.repeat)
    ms["ssim_1"], s1 = timed(lambda: ops.ssim(clamped, gb, levels=1), a.repeat)
    ms["ssim_5"], s5 = timed(lambda: ops.ssim(clamped, gb, levels=5), a.repeat)
    ms["render_metrics"], m = timed(lambda: P.evaluation.render_metrics(color, gt_color, depth, gt_depth), a.repeat)
    g = torch_window(dev)
    xp, yp = clamped.permute(0, 3, 1, 2).contiguous(), gb.permute(0, 3, 1, 2).contiguous()
    ms["torch_errors"], err_t = timed(lambda: torch_errors(color, gt_color, depth, gt_depth), a.repeat)
    ms["torch_ssim_1"], t1 = timed(lambda: torch_ssim(xp, yp, g, 1), a.repeat)
    ms["torch_ssim_5"], t5 = timed(lambda: torch_ssim(xp, yp, g, 5), a.repeat)
    ms["torch_ssim_5_with_layout_change"], _ = timed(
        lambda: torch_ssim(clamped.permute(0, 3, 1, 2).contiguous(), gb.permute(0, 3, 1, 2).contiguous(), g, 5),
        a.repeat)
    for k in ms:
        ms[k] = round(ms[k], 4)
    level0_bytes = 2 * H * W * 3 * 4
    out["level0_traffic_floor_ms"] = round(level0_bytes / HBM_PEAK * 1e3, 5)
    out["level0_bytes"] = level0_bytes
    out["torch_over_hip"] = {"errors": round(ms["torch_errors"] / ms["image_errors"], 2),
                             "ssim_1": round(ms["torch_ssim_1"] / ms["ssim_1"], 2),
                             "ssim_5": round(ms["torch_ssim_5"] / ms["ssim_5"], 2)}
    out["metrics_over_render"] = round(ms["render_metrics"] / ms["render_img"], 4)
    out["max_difference_from_torch"] = {
        "errors_relative": float(((err[0] - err_t).abs() / err_t.abs().clamp(min=1)).max()),
        "ssim_1": float((s1 - t1).abs().max()), "ssim_5": float((s5 - t5).abs().max())}
    out["values"] = {k: m[k] for k in ("psnr", "ssim", "ms_ssim", "depth_l1")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
