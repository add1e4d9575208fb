#!/usr/bin/env python3
"""Depth odometry at the Azure Kinect camera (720 x 1280): ms per stage and per tracked frame.

    python tools/odometry_bench.py [--frames 12] [--repeat 5] [--out profiles/odometry.json]

Workload: a camera moving by about 2 cm and 0.5 degrees per frame through the analytic room tools/tsdf_bench.py
uses (the walls of Replica room0's bound shrunk by a tenth, tests/golden/scenes.py), looking into a corner (one
wall alone leaves the normal equations singular), its depth in millimetres without the sensor jitter of
scenes.box_depth (a 10 % jitter leaves no normals to track with), 4 % of it missing in 8 x 8 pixel holes.  The
volume has voxel 0.02 and truncation 0.06.  Each stage is timed with device events after a warm-up call, median
of `--repeat`: depth_maps, the ray cast of the volume after 4 fused frames, one icp_sums call per stride
(csrc/nslam_odometry.hip), and a whole DepthOdometry.track call (ray cast, maps, 19 ICP iterations with their
29-double downloads and host solves, fusion) over the following frames.
  icp_sums_torch   the sums of include/nslam.h written with torch operators on the same GPU: the bar.
                   nslam_icp_sums must not be slower than this
The photometric term (DepthOdometry(photo_weight=...)) is measured on the same scene with a procedural texture (a
smooth function of the world hit point): gray_pyramid, photo_sums at levels 2, 1 and 0 with the same sums in torch
operators as their bar, and a whole track call with the term next to the one without.
A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import scenes  # noqa: E402

CAM = dict(H=720, W=1280, fx=607.4694213867188, fy=607.4534912109375, cx=636.9967041015625, cy=369.2689514160156)
VOXEL, TRUNC, EXTENT, DEPTH_TRUNC, MAX_JUMP, DIST_TH, ANGLE = 0.02, 0.06, 10.0, 12.0, 0.06, 0.1, 30.0
STRIDES = (4, 2, 1)


def timed(fn, repeat):
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


def room_depth(c2w, seed, holes=True):
    """z-depth [H,W] float32 of the room's walls seen from the +z-forward pose c2w, in millimetre steps (holes:
    4 % of it missing in 8 x 8 pixel blocks)."""
    b = np.asarray(scenes.enlarge_bound(scenes.ROOM0_BOUND, 0.32), dtype=np.float64)
    ext = b[:, 1] - b[:, 0]
    lo, hi = b[:, 0] + 0.1 * ext, b[:, 1] - 0.1 * ext
    jj, ii = np.meshgrid(np.arange(CAM["H"], dtype=np.float64), np.arange(CAM["W"], dtype=np.float64), indexing="ij")
    d = np.stack([(ii - CAM["cx"]) / CAM["fx"], (jj - CAM["cy"]) / CAM["fy"], np.ones_like(ii)], -1) @ c2w[:3, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.stack([lo, hi], -1)[None, None] - c2w[:3, 3][None, None, :, None]) / d[..., None]
    z = np.min(np.max(t, -1), -1)
    if holes:
        gone = np.random.default_rng(seed).random((CAM["H"] // 8 + 1, CAM["W"] // 8 + 1)) < 0.04
        z[np.repeat(np.repeat(gone, 8, 0), 8, 1)[:CAM["H"], :CAM["W"]]] = 0.0
    return (np.clip(np.round(z * 1000.0), 0, 65535).astype(np.uint16).astype(np.float32) / np.float32(1000.0))


def room_color(depth, c2w):
    """uint8 [H,W,3]: sums of sinusoids (wavelengths 0.5 to 2 m) of the world point behind every pixel."""
    jj, ii = np.meshgrid(np.arange(CAM["H"], dtype=np.float64), np.arange(CAM["W"], dtype=np.float64), indexing="ij")
    d = depth.astype(np.float64)
    p = np.stack([(ii - CAM["cx"]) / CAM["fx"] * d, (jj - CAM["cy"]) / CAM["fy"] * d, d], -1) @ c2w[:3, :3].T + c2w[:3, 3]
    waves = [(0.16, (0.0, 9.0, 4.0)), (0.14, (3.0, -5.0, 11.0)), (0.12, (7.5, 3.0, -6.5)), (0.10, (-2.0, 2.5, 3.5))]
    out = np.empty(depth.shape + (3,), np.uint8)
    for c in range(3):
        f = 0.5 + sum(a * np.sin(p @ np.array(k) + 1.3 * c + 0.7 * i) for i, (a, k) in enumerate(waves))
        out[..., c] = np.floor(255.0 * np.clip(f, 0.0, 1.0) + 0.5).astype(np.uint8)
    return out


def torch_photo_sums(sv, sg, rg, level, rv, T, w2c, intr, depth_th, photo_th):
    """nslam_photo_sums' contract in torch operators (float64): the 29 sums on the device."""
    fx, fy, cx, cy = intr
    S = 1 << level
    Hr, Wr = rv.shape[:2]
    rh, rw = rg.shape
    s = sv[::S, ::S].reshape(-1, 3).double()
    ok = ~torch.isnan(s).any(-1)
    s = torch.nan_to_num(s)
    p = s @ T[:3, :3].T + T[:3, 3]
    pc = p @ w2c[:3, :3].T + w2c[:3, 3]
    ok &= pc[:, 2] > 0
    z = torch.where(ok, pc[:, 2], torch.ones_like(pc[:, 2]))
    x0, y0 = pc[:, 0] * fx / z + cx, pc[:, 1] * fy / z + cy
    xn, yn = x0 + 0.5, y0 + 0.5
    ok &= (xn >= 0) & (xn < Wr) & (yn >= 0) & (yn < Hr)
    at = torch.where(ok, yn.long() * Wr + xn.long(), torch.zeros_like(xn, dtype=torch.long))
    qz = rv.reshape(-1, 3)[at][:, 2].double()
    ok &= ~torch.isnan(rv.reshape(-1, 3)[at]).any(-1)
    ok &= (z - torch.nan_to_num(qz)).abs() <= depth_th
    xl, yl = x0 / S, y0 / S
    fi, fj = torch.floor(xl), torch.floor(yl)
    ok &= (fi >= 0) & (fi + 1 <= rw - 1) & (fj >= 0) & (fj + 1 <= rh - 1)
    i0 = torch.where(ok, fi, torch.zeros_like(fi)).long()
    j0 = torch.where(ok, fj, torch.zeros_like(fj)).long()
    a, b = xl - fi, yl - fj
    g = rg.reshape(-1).double()
    i1, j1 = (i0 + 1).clamp(max=rw - 1), (j0 + 1).clamp(max=rh - 1)
    I00, I10, I01, I11 = g[j0 * rw + i0], g[j0 * rw + i1], g[j1 * rw + i0], g[j1 * rw + i1]
    iref = (1 - b) * ((1 - a) * I00 + a * I10) + b * ((1 - a) * I01 + a * I11)
    gx = ((1 - b) * (I10 - I00) + b * (I11 - I01)) / S
    gy = ((1 - a) * (I01 - I00) + a * (I11 - I10)) / S
    r = iref - sg.reshape(-1).double()
    ok &= r.abs() <= photo_th
    gc = torch.stack([gx * (fx / z), gy * (fy / z), -(gx * fx * pc[:, 0] + gy * fy * pc[:, 1]) / (z * z)], -1)
    gw = gc @ w2c[:3, :3]
    J = torch.cat([torch.cross(p, gw, dim=-1), gw], -1) * ok[:, None]
    r = r * ok
    A = J.T @ J
    iu = torch.triu_indices(6, 6, device=A.device)
    return torch.cat([A[iu[0], iu[1]], J.T @ r, (r * r).sum()[None], ok.sum()[None].double()])


def torch_icp_sums(sv, sn, T, mv, mn, w2c, intr, stride, dist_th, cos_th):
    """nslam_icp_sums' contract in torch operators (float64): the 29 sums on the device."""
    fx, fy, cx, cy = intr
    Hm, Wm = mv.shape[:2]
    s, ns = sv[::stride, ::stride].reshape(-1, 3).double(), sn[::stride, ::stride].reshape(-1, 3).double()
    ok = ~(torch.isnan(s).any(-1) | torch.isnan(ns).any(-1))
    s, ns = torch.nan_to_num(s), torch.nan_to_num(ns)
    p = s @ T[:3, :3].T + T[:3, 3]
    pc = p @ w2c[:3, :3].T + w2c[:3, 3]
    ok &= pc[:, 2] > 0
    z = torch.where(ok, pc[:, 2], torch.ones_like(pc[:, 2]))
    uf, vf = pc[:, 0] * fx / z + cx + 0.5, pc[:, 1] * fy / z + cy + 0.5
    ok &= (uf >= 0) & (uf < Wm) & (vf >= 0) & (vf < Hm)
    at = torch.where(ok, vf.long() * Wm + uf.long(), torch.zeros_like(uf, dtype=torch.long))
    q, n = mv.reshape(-1, 3)[at].double(), mn.reshape(-1, 3)[at].double()
    ok &= ~(torch.isnan(q).any(-1) | torch.isnan(n).any(-1))
    q, n = torch.nan_to_num(q), torch.nan_to_num(n)
    d = p - q
    ok &= d.norm(dim=-1) <= dist_th
    ok &= ((ns @ T[:3, :3].T) * n).sum(-1) >= cos_th
    J = torch.cat([torch.cross(p, n, dim=-1), n], -1) * ok[:, None]
    r = (n * d).sum(-1) * ok
    A = J.T @ J
    iu = torch.triu_indices(6, 6, device=A.device)
    return torch.cat([A[iu[0], iu[1]], J.T @ r, (r * r).sum()[None], ok.sum()[None].double()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "odometry.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("odometry_bench: no HIP device; nothing here can be measured on the CPU")
    if a.frames < 4 + a.repeat + 1:
        raise SystemExit("odometry_bench: at least 5 + repeat frames")
    P = importlib.import_module("nice-slam_amd")
    ops, od_mod = P.ops, P.odometry
    dev = torch.device("cuda:0")
    intr = (CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
    ctr = np.asarray(scenes.enlarge_bound(scenes.ROOM0_BOUND, 0.32), dtype=np.float64).mean(1)
    first = P.tsdf.opengl_to_cv(scenes.look_pose(ctr, 0.75, 0.5).astype(np.float64))
    step = od_mod.se3_exp([0.004, 0.008, -0.003, 0.015, -0.008, 0.012])
    world = [first]
    for _ in range(1, a.frames):
        world.append(world[-1] @ step)
    depth = [torch.from_numpy(room_depth(p, k)).to(dev) for k, p in enumerate(world)]
    od = od_mod.DepthOdometry(CAM["H"], CAM["W"], *intr, VOXEL, TRUNC, EXTENT, dev, DEPTH_TRUNC, MAX_JUMP,
                              dist_th=DIST_TH, angle_deg=ANGLE, strides=STRIDES)
    res = [od.track(d) for d in depth[:4]]
    out = {"image": [CAM["H"], CAM["W"]], "voxel": VOXEL, "trunc": TRUNC, "extent": EXTENT, "repeat": a.repeat,
           "strides": list(STRIDES), "iters": od.iters, "blocks_after_4_frames": od.volume.n_blocks, "stages_ms": {}}
    ms, (sv, sn) = timed(lambda: ops.depth_maps(depth[4], *intr, DEPTH_TRUNC, MAX_JUMP), a.repeat)
    out["stages_ms"]["depth_maps"] = round(ms, 4)
    last = od.poses[-1]
    ms, (mv, mn) = timed(lambda: od.volume.raycast(last, CAM["H"], CAM["W"], *intr, od.near, od.far), a.repeat)
    out["stages_ms"]["raycast"] = round(ms, 4)
    out["raycast_hits"] = int((~torch.isnan(mv).any(-1)).sum())
    T = od_mod.predict(od.poses)
    w2c = np.linalg.inv(last)
    T_d, w2c_d = torch.from_numpy(T).to(dev), torch.from_numpy(w2c).to(dev)
    cos_th = math.cos(math.radians(ANGLE))
    out["icp_sums"] = {}
    for s in STRIDES:
        ms, got = timed(lambda: ops.icp_sums(sv, sn, T, mv, mn, w2c, *intr, s, DIST_TH, cos_th), a.repeat)
        ms_t, ref = timed(lambda: torch_icp_sums(sv, sn, T_d, mv, mn, w2c_d, intr, s, DIST_TH, cos_th), a.repeat)
        out["stages_ms"][f"icp_sums_stride{s}"] = round(ms, 4)
        out["stages_ms"][f"icp_sums_torch_stride{s}"] = round(ms_t, 4)
        scale = torch.maximum(ref.abs(), torch.ones_like(ref))
        out["icp_sums"][f"stride{s}"] = {"hip_not_slower_than_torch": bool(ms <= ms_t),
                                         "torch_over_hip": round(ms_t / ms, 2), "inliers": int(got[28]),
                                         "inliers_torch": int(ref[28]),
                                         "max_relative_difference_from_torch": float(((got - ref).abs() / scale).max())}
    frame_ms, lost, err = [], [], None
    for k in range(4, a.frames):
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        r = od.track(depth[k])
        b0.record()
        torch.cuda.synchronize()
        frame_ms.append(a0.elapsed_time(b0))
        if r["lost"]:
            lost.append(k)
        res.append(r)
    lost = [k for k, r in enumerate(res) if r["lost"]]
    rel = np.linalg.inv(world[0]) @ world[-1]
    d = np.linalg.inv(res[-1]["c2w"]) @ rel
    err = {"translation_mm": float(1e3 * np.linalg.norm(d[:3, 3])),
           "rotation_deg": float(math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(d[:3, :3]) - 1.0))))))}
    out["stages_ms"]["track_frame"] = round(statistics.median(frame_ms[1:1 + a.repeat]), 4)
    out["track"] = {"frames": a.frames, "lost": lost, "final_error": err, "inliers_last": res[-1]["inliers"],
                    "rms_last": res[-1]["rms"], "blocks": od.volume.n_blocks}
    # the photometric term: the same frames with a procedural texture
    weight = od_mod.PHOTO_WEIGHT
    # (a colour camera sees the wall where the depth has a hole: the texture is taken at the depth without holes)
    color = [torch.from_numpy(room_color(room_depth(p, k, holes=False), p)).to(dev) for k, p in enumerate(world)]
    od_p = od_mod.DepthOdometry(CAM["H"], CAM["W"], *intr, VOXEL, TRUNC, EXTENT, dev, DEPTH_TRUNC, MAX_JUMP,
                                dist_th=DIST_TH, angle_deg=ANGLE, strides=STRIDES, photo_weight=weight)
    res_p = [od_p.track(d, c) for d, c in zip(depth[:4], color[:4])]
    levels = max(STRIDES).bit_length()
    ms, gs = timed(lambda: ops.gray_pyramid(color[4], levels), a.repeat)
    out["stages_ms"]["gray_pyramid"] = round(ms, 4)
    gr, rv, ref_pose = od_p._ref
    T = od_mod.predict(od_p.poses)
    ref_w2c = np.linalg.inv(ref_pose)
    T_d, w2c_d = torch.from_numpy(T).to(dev), torch.from_numpy(ref_w2c).to(dev)
    out["photo_sums"] = {}
    for s in STRIDES:
        lv = s.bit_length() - 1
        ms, got = timed(lambda: ops.photo_sums(sv, gs[lv], gr[lv], lv, rv, T, ref_w2c, *intr, DIST_TH, 1e300), a.repeat)
        ms_t, ref = timed(lambda: torch_photo_sums(sv, gs[lv], gr[lv], lv, rv, T_d, w2c_d, intr, DIST_TH, 1e300),
                          a.repeat)
        out["stages_ms"][f"photo_sums_level{lv}"] = round(ms, 4)
        out["stages_ms"][f"photo_sums_torch_level{lv}"] = round(ms_t, 4)
        scale = torch.maximum(ref.abs(), torch.ones_like(ref))
        out["photo_sums"][f"level{lv}"] = {"hip_not_slower_than_torch": bool(ms <= ms_t),
                                           "torch_over_hip": round(ms_t / ms, 2), "inliers": int(got[28]),
                                           "inliers_torch": int(ref[28]),
                                           "max_relative_difference_from_torch": float(((got - ref).abs() / scale).max())}
    frame_ms = []
    for k in range(4, a.frames):
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        res_p.append(od_p.track(depth[k], color[k]))
        b0.record()
        torch.cuda.synchronize()
        frame_ms.append(a0.elapsed_time(b0))
    d = np.linalg.inv(res_p[-1]["c2w"]) @ rel
    out["stages_ms"]["track_frame_photometric"] = round(statistics.median(frame_ms[1:1 + a.repeat]), 4)
    out["track_photometric"] = {
        "photo_weight": weight, "lost": [k for k, r in enumerate(res_p) if r["lost"]],
        "final_error": {"translation_mm": float(1e3 * np.linalg.norm(d[:3, 3])),
                        "rotation_deg": float(math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(d[:3, :3]) - 1.0))))))},
        "inliers_last": res_p[-1]["inliers"], "photo_inliers_last": res_p[-1]["photo_inliers"],
        "photo_rms_last": res_p[-1]["photo_rms"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
