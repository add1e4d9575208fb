#!/usr/bin/env python3
"""Fuse a run's sensor depth into a coloured mesh along the estimated or the ground-truth trajectory.

    python tools/fuse_tsdf.py CONFIG [--output DIR] [--input_folder DIR] [--traj est|gt] [--every N]
                              [--voxel L] [--trunc T] [--mesh OUT.ply]

Reads the last checkpoint of DIR/ckpts (DIR: --output, else the config's data.output) for the trajectories and
the frames through the package's dataset reader, fuses every N-th frame (default 5) into a block-sparse TSDF
volume on the device (nice-slam_amd/tsdf.py) and writes the volume's mesh with its vertex colours as a binary
PLY (default DIR/mesh/tsdf_mesh.ply), in the run's scaled world frame divided by `scale`, as the run's own
meshes are.  The block table covers mapping.bound * scale grown by the truncation; samples beyond it are counted
(n_outside), not fused.  Frames whose pose holds NaN or inf are skipped and counted.  No cleaning: tools/cull_mesh.py
and tools/eval_recon.py take the file as it is.  Defaults: --voxel 4 scale / 512 and --trunc 0.04 scale, the
reference's values in Mesher.get_bound_from_frames.
"""
import argparse
import importlib
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from eval_ate import load_config  # noqa: E402

BATCH = 32


def main(argv=None):
    ap = argparse.ArgumentParser(description="Fuse a run's depth frames into a coloured TSDF mesh.")
    ap.add_argument("config", type=str, help="the run's YAML config")
    ap.add_argument("--output", type=str, help="output folder; overrides the config's data.output")
    ap.add_argument("--input_folder", type=str, help="dataset folder; overrides the config's data.input_folder")
    ap.add_argument("--traj", choices=("est", "gt"), default="est", help="the trajectory to fuse along")
    ap.add_argument("--every", type=int, default=5, help="fuse every N-th frame")
    ap.add_argument("--voxel", type=float, help="voxel edge in scaled world units (default 4 scale / 512)")
    ap.add_argument("--trunc", type=float, help="truncation distance (default 0.04 scale)")
    ap.add_argument("--mesh", type=str, help="the PLY to write (default DIR/mesh/tsdf_mesh.ply)")
    a = ap.parse_args(argv)
    if a.every < 1:
        raise SystemExit("fuse_tsdf: --every must be at least 1")
    cfg = load_config(a.config, "configs/nice_slam.yaml")
    scale = cfg.get("scale", 1)
    output = a.output if a.output is not None else cfg.get("data", {}).get("output")
    if output is None:
        raise SystemExit("fuse_tsdf: no output folder (pass --output or set data.output in the config)")
    ckptsdir = os.path.join(output, "ckpts")
    ckpts = sorted(f for f in os.listdir(ckptsdir) if "tar" in f) if os.path.isdir(ckptsdir) else []
    if not ckpts:
        raise SystemExit(f"fuse_tsdf: no checkpoint under {ckptsdir}")
    path = os.path.join(ckptsdir, ckpts[-1])
    print("Get ckpt :", path)
    if not torch.cuda.is_available():
        raise SystemExit("fuse_tsdf: no HIP device; the volume has no CPU fallback")
    P = importlib.import_module("nice-slam_amd")
    dev = torch.device("cuda:0")
    ck = P.datasets.load_checkpoint(path, device="cpu")  # only the trajectories are read
    poses = ck["estimate_c2w_list" if a.traj == "est" else "gt_c2w_list"]
    ds = P.get_dataset(cfg, a, scale, device=dev)
    n = min(int(ck["idx"]) + 1, len(ds), int(poses.shape[0]))
    voxel = a.voxel if a.voxel is not None else 4.0 * scale / 512.0
    trunc = a.trunc if a.trunc is not None else 0.04 * scale
    block = 16.0 * voxel
    bound = np.asarray(cfg["mapping"]["bound"], dtype=np.float64) * scale
    lo = [math.floor((b - trunc) / block) for b in bound[:, 0]]
    hi = [math.floor((b + trunc) / block) + 1 for b in bound[:, 1]]
    vol = P.tsdf.TSDFVolume(voxel, trunc, lo, hi, dev, color=True)
    _, _, fx, fy, cx, cy = P.slam.update_cam(cfg)  # the intrinsics of the images as the reader hands them out
    used = skipped = n_outside = 0
    depths, colors, c2ws = [], [], []

    def flush():
        nonlocal n_outside
        if depths:
            r = vol.integrate(torch.stack(depths, 0), torch.stack(colors, 0), np.stack(c2ws, 0), fx, fy, cx, cy)
            n_outside += r["n_outside"]
            depths.clear(), colors.clear(), c2ws.clear()

    for i in range(0, n, a.every):
        c2w = poses[i].detach().cpu().numpy()
        if not np.isfinite(c2w).all():
            skipped += 1
            continue
        _, color, depth, _ = ds[i]
        depths.append(depth.float())
        colors.append((color.float() * 255).to(torch.uint8))
        c2ws.append(P.tsdf.opengl_to_cv(c2w))
        used += 1
        if len(depths) == BATCH:
            flush()
    flush()
    mesh = vol.extract_mesh()
    v = (mesh["vertices"] / scale).cpu().numpy()
    f = mesh["faces"].cpu().numpy()
    out = a.mesh if a.mesh is not None else os.path.join(output, "mesh", "tsdf_mesh.ply")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    P.mesher.write_ply(out, v, f, mesh["colors"].cpu().numpy())
    res = {"mesh": out, "traj": a.traj, "frames": used, "skipped": skipped, "blocks": vol.n_blocks, "V": int(v.shape[0]),
           "F": int(f.shape[0]), "n_outside": n_outside}
    print(f"{out}: frames {used} (skipped {skipped}) blocks {vol.n_blocks} V {v.shape[0]} F {f.shape[0]} "
          f"n_outside {n_outside}")
    return res


if __name__ == "__main__":
    main()
