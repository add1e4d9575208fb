#!/usr/bin/env python3
"""Mesh extraction at Replica room0 size: ms per stage, GB/s on algorithmic bytes, V and F.

    python tools/mesh_bench.py [--resolution 256] [--keyframes 10] [--repeat 5] [--out profiles/mesh_extract.json]

Workload: the room0 marching-cubes bound at `--resolution`^3 lattice points, `--keyframes` keyframes at
680x1200 with analytic box depths (tests/golden/scenes.py), randomly initialised room0 grids and decoders
(timing only).  Stages, each timed with device events after a warm-up call (median of `--repeat`):
  masks_hip      nslam_point_masks over the whole lattice (depth_test, points_batch_size 500000)
  masks_torch    the same formulae as the reference writes them, in torch on the same GPU: the bar.
                 nslam_point_masks must not be slower than this
  eval_fine      the lattice's occupancy logits (Renderer.eval_points, fine stage)
  mc_count/emit  marching cubes of an analytic room volume (a box shell and two spheres: a closed surface of
                 realistic size; the random-weight field is noise and would give a meaningless mesh)
  cull, components   cleaning of that mesh
GB/s are algorithmic bytes (what the pass must read and write once, from shapes) over the measured time,
against the 8 TB/s HBM peak.  A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import ctypes
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
    "coarse": True, "scale": 1, "occupancy": True, "verbose": False,
    "cam": dict(scenes.ROOM0_CAM, crop_edge=0),
    "grid_len": {"coarse": 2.0, "middle": 0.32, "fine": 0.16, "color": 0.16, "bound_divisible": 0.32},
    "mapping": {"bound": scenes.ROOM0_BOUND, "marching_cubes_bound": [[-2.7, 8.7], [-3.0, 5.3], [-3.3, 3.1]]},
    "meshing": {"resolution": 256, "level_set": 0, "clean_mesh_bound_scale": 1.02,
                "remove_small_geometry_threshold": 0.2, "color_mesh_extraction_method": "direct_point_query",
                "get_largest_components": False, "depth_test": True},
    "model": {"c_dim": 32, "coarse_bound_enlarge": 2, "pos_embedding_method": "fourier"},
    "data": {"dim": 3},
    "rendering": {"N_samples": 32, "N_surface": 16, "N_importance": 0, "lindisp": False, "perturb": 0.0},
}


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


def torch_point_masks(points, w2c, depth, H, W, fx, fy, cx, cy, batch):
    """Mesher.point_masks' keyframe branch with depth_test (Mesher.py:127-199) as the reference writes it,
    on device tensors (w2c already inverted and uploaded) → (seen, forecast, unseen) bool [N]."""
    dev = points.device
    K = torch.tensor([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]], dtype=torch.float64, device=dev).float()
    seen_l, fore_l = [], []
    for pnts in torch.split(points, batch, dim=0):
        seen = torch.zeros(pnts.shape[0], dtype=torch.bool, device=dev)
        fore = torch.zeros(pnts.shape[0], dtype=torch.bool, device=dev)
        homo = torch.cat([pnts, torch.ones_like(pnts[:, :1])], dim=1).reshape(-1, 4, 1)
        for k in range(w2c.shape[0]):
            cam = (w2c[k] @ homo)[:, :3]
            cam[:, 0] *= -1
            uv = K @ cam
            z = uv[:, -1:] + 1e-8
            uv = uv[:, :2] / z
            zz = z[:, :, 0]
            s = ((uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0) & (zz < 0)).reshape(-1)
            f = ((uv[:, 0] < W + 1000) & (uv[:, 0] > -1000) & (uv[:, 1] < H + 1000) & (uv[:, 1] > -1000)
                 & (zz < 0)).reshape(-1)
            vgrid = uv.reshape(1, 1, -1, 2).clone()
            vgrid[..., 0] = vgrid[..., 0] / (W - 1) * 2.0 - 1.0
            vgrid[..., 1] = vgrid[..., 1] / (H - 1) * 2.0 - 1.0
            ds = F.grid_sample(depth[k].reshape(1, 1, H, W), vgrid, padding_mode="zeros",
                               align_corners=True).reshape(-1)
            pd = -cam[:, 2].reshape(-1)
            f = f & (pd < ds.max())
            s = s & (pd < ds + 2.4) & (ds - 2.4 < pd)
            seen |= s
            fore |= f
        fore &= ~seen
        seen_l.append(seen)
        fore_l.append(fore)
    seen, fore = torch.cat(seen_l), torch.cat(fore_l)
    return seen, fore, ~(seen | fore)


def room_volume(mesher, res, dev):
    """Occupancy-like field on the lattice (high inside matter): the shell between the marching-cubes bound
    shrunk by 0.4 m and by 0.6 m (walls seen from inside), and two solid spheres; level 0."""
    g = mesher.get_grid_uniform(res)
    x, y, z = (torch.as_tensor(np.asarray(a), device=dev) for a in g["xyz"])
    X, Y, Z = torch.meshgrid(x, y, z, indexing="ij")
    b = torch.as_tensor(np.asarray(CFG["mapping"]["marching_cubes_bound"]), device=dev)
    ctr, half = b.mean(1), (b[:, 1] - b[:, 0]) / 2
    q = torch.stack([(X - ctr[0]).abs() - half[0], (Y - ctr[1]).abs() - half[1], (Z - ctr[2]).abs() - half[2]], 0)
    box = q.max(0).values                                   # signed distance-like: < 0 inside the bound
    shell = 0.1 - (box + 0.5).abs()                         # > 0 within 0.1 m of the surface 0.5 m inside
    s1 = 0.8 - ((X - ctr[0] - 1.5) ** 2 + (Y - ctr[1]) ** 2 + (Z - ctr[2] + 1.0) ** 2).sqrt()
    s2 = 0.5 - ((X - ctr[0] + 2.0) ** 2 + (Y - ctr[1] - 1.0) ** 2 + (Z - ctr[2]) ** 2).sqrt()
    vol = torch.maximum(shell, torch.maximum(s1, s2)).float().contiguous()
    return vol, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--keyframes", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_extract.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: no HIP device; nothing here can be measured on the CPU")
    P = importlib.import_module("nice-slam_amd")
    dev = torch.device("cuda:0")
    cfg = dict(CFG, meshing=dict(CFG["meshing"], resolution=a.resolution))
    st = P.slam.SlamState(cfg, dev, n_img=a.keyframes, generator=torch.Generator().manual_seed(2))
    m = st.mesher
    H, W, fx, fy, cx, cy = st.H, st.W, st.fx, st.fy, st.cx, st.cy
    b = scenes.enlarge_bound(scenes.ROOM0_BOUND, 0.32)
    ctr = b.mean(1)
    poses = [scenes.look_pose(ctr, 0.6 * k, 0.12 * ((k % 3) - 1), (0.3 * ((k % 4) - 1.5), 0.2 * (k % 2), 0.05 * k))
             for k in range(a.keyframes)]
    kfs = [{"est_c2w": torch.from_numpy(p),
            "depth": torch.from_numpy(scenes.box_depth(p, scenes.ROOM0_CAM, b, seed=k)).to(dev)}
           for k, p in enumerate(poses)]
    c2w_list = torch.from_numpy(np.stack(poses, 0))
    res = a.resolution
    n = res ** 3
    points = m.get_grid_uniform(res)["grid_points"].to(dev).contiguous()
    w2c, depth = m._w2c_and_depth(kfs, c2w_list, a.keyframes - 1, dev, False)
    out = {"resolution": res, "points": n, "keyframes": a.keyframes, "image": [H, W],
           "points_batch_size": m.points_batch_size, "repeat": a.repeat, "stages_ms": {}, "gbps": {},
           "share_of_hbm_peak": {}}

    def rate(name, ms, nbytes):
        out["stages_ms"][name] = round(ms, 4)
        if nbytes:
            out["gbps"][name] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            out["share_of_hbm_peak"][name] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)

    mask_bytes = n * (12 + 3) + a.keyframes * H * W * 4
    ms, hip = timed(lambda: P.ops.point_masks(points, w2c, depth, H, W, fx, fy, cx, cy, True, False,
                                              m.points_batch_size), a.repeat)
    rate("masks_hip", ms, mask_bytes)
    ms_t, ref = timed(lambda: torch_point_masks(points, w2c, depth, H, W, fx, fy, cx, cy, m.points_batch_size),
                      max(1, a.repeat // 2))
    rate("masks_torch", ms_t, mask_bytes)
    diff = sum(int((x != y).sum()) for x, y in zip(hip, ref))
    out["masks"] = {"seen": int(hip[0].sum()), "forecast": int(hip[1].sum()), "unseen": int(hip[2].sum()),
                    "points_differing_from_torch": diff, "hip_not_slower_than_torch": bool(ms <= ms_t),
                    "torch_over_hip": round(ms_t / ms, 2)}
    del ref

    with torch.no_grad():
        ms, _ = timed(lambda: m.eval_points(points, st.shared_decoders, st.shared_c, "fine", dev),
                      max(1, a.repeat // 2))
    rate("eval_fine", ms, 0)

    vol, g = room_volume(m, res, dev)
    L = P._lib.lib()
    ws = torch.empty(L.nslam_mc_workspace_size(res, res, res), dtype=torch.uint8, device=dev)
    stream = P._lib.stream_ptr(dev)
    ms, _ = timed(lambda: P._lib.check(L.nslam_mc_count(vol.data_ptr(), res, res, res, 0.0, ws.data_ptr(), ws.numel(),
                                                        stream), "nslam_mc_count"), a.repeat)
    rate("mc_count", ms, n * 4 + n * 4)
    x, y, z = (np.asarray(v) for v in g["xyz"])
    origin, spacing = (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1])
    ms_all, (verts, faces) = timed(lambda: P.ops.marching_cubes(vol, 0.0, origin, spacing), a.repeat)
    out["stages_ms"]["mc_total_with_scans"] = round(ms_all, 4)
    V, Fc = int(verts.shape[0]), int(faces.shape[0])
    flags, ntri = ws[:3 * n], ws[3 * n:]
    voff = (torch.cumsum(flags, 0, dtype=torch.int32) - flags).contiguous()
    foff = (torch.cumsum(ntri, 0, dtype=torch.int32) - ntri).contiguous()
    o3, s3 = (ctypes.c_double * 3)(*map(float, origin)), (ctypes.c_double * 3)(*map(float, spacing))
    ms, _ = timed(lambda: P._lib.check(L.nslam_mc_emit(vol.data_ptr(), res, res, res, 0.0, o3, s3, voff.data_ptr(),
                                                       foff.data_ptr(), V, Fc, verts.data_ptr(), faces.data_ptr(),
                                                       stream), "nslam_mc_emit"), a.repeat)
    rate("mc_emit", ms, n * 4 + n * 16 + V * 24 + Fc * 12)
    out["V"], out["F"] = V, Fc

    vmask = ~m.point_masks_device(verts, kfs, c2w_list, a.keyframes - 1, dev)[0]
    ms, keep = timed(lambda: P.ops.mesh_face_cull(faces, vmask), a.repeat)
    rate("cull", ms, Fc * 13 + V)
    kept = faces[keep].contiguous()
    ms, (kv, kf, _) = timed(lambda: P.ops.mesh_keep_components(verts, kept, False, 0.2), max(1, a.repeat // 2))
    rate("components", ms, 0)
    out["after_cleaning"] = {"V": int(kv.shape[0]), "F": int(kf.shape[0])}
    out["notes"] = ("device-event medians after one warm-up; GB/s on algorithmic bytes vs 8 TB/s HBM; marching cubes "
                    "and cleaning on an analytic room volume, eval_fine on randomly initialised grids (timing only)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
