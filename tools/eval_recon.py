#!/usr/bin/env python3
"""Reconstruction metrics of a mesh against the ground truth (the reference's src/tools/eval_recon.py, on the
device): -3d accuracy [cm], completion [cm] and completion ratio [< 5 cm, %]; -2d depth L1 [cm] over views drawn
inside the ground truth; both after a point-to-point ICP alignment.

    python tools/eval_recon.py --rec_mesh rec.ply --gt_mesh gt.ply -3d [--no_align] [--n_points 200000] [--seed 0]
    python tools/eval_recon.py --rec_mesh rec.ply --gt_mesh gt.ply -2d [--no_align] [--n_imgs 1000] [--seed 0]
                               [--unseen_pc gt_pc_unseen.npy]

-2d reads the points no view may see from --unseen_pc, by default the ground truth's `_pc_unseen.npy` next to it,
as the reference does.  --cam_box FILE.npy ([4,4]: the extents, then the 3x4 box-to-world matrix) gives the box the
cameras are drawn from and needs no scipy; --height, --width, --focal, --z_near and --z_far change the camera
(DESIGN §7b).  -2d -3d runs both and returns both dicts merged.
"""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Reconstruction metrics of a mesh against its ground truth.")
    ap.add_argument("--rec_mesh", type=str, required=True, help="the reconstruction (PLY)")
    ap.add_argument("--gt_mesh", type=str, required=True, help="the ground truth (PLY)")
    ap.add_argument("-2d", "--metric_2d", action="store_true", help="depth L1")
    ap.add_argument("-3d", "--metric_3d", action="store_true", help="accuracy, completion, completion ratio")
    ap.add_argument("--no_align", action="store_true", help="skip the ICP alignment")
    ap.add_argument("--n_points", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n_imgs", type=int, default=1000, help="-2d: views")
    ap.add_argument("--unseen_pc", type=str, default=None, help="-2d: .npy [N,3] of points no view may see")
    ap.add_argument("--cam_box", type=str, default=None, help="-2d: .npy [4,4], extents then the 3x4 transform")
    ap.add_argument("--height", type=int, default=500)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--focal", type=float, default=300.0)
    ap.add_argument("--z_near", type=float, default=None)
    ap.add_argument("--z_far", type=float, default=20.0)
    a = ap.parse_args(argv)
    if not (a.metric_2d or a.metric_3d):
        raise SystemExit("eval_recon: nothing to do; pass -3d and / or -2d")
    E = importlib.import_module("nice-slam_amd").evaluation
    out = {}
    if a.metric_3d:
        out.update(E.calc_3d_metric(a.rec_mesh, a.gt_mesh, align=not a.no_align, n_points=a.n_points, seed=a.seed))
    if a.metric_2d:
        import numpy as np
        unseen = np.load(a.unseen_pc) if a.unseen_pc else None
        cam_box = None
        if a.cam_box:
            box = np.load(a.cam_box).astype(np.float64).reshape(4, 4)
            cam_box = (box[0, :3].copy(), np.concatenate([box[1:4], [[0.0, 0.0, 0.0, 1.0]]], 0))
        out.update(E.calc_depth_l1(a.rec_mesh, a.gt_mesh, align=not a.no_align, n_imgs=a.n_imgs, seed=a.seed,
                                   unseen_pc=unseen, cam_box=cam_box, H=a.height, W=a.width, focal=a.focal,
                                   z_near=a.z_near, z_far=a.z_far))
    return out


if __name__ == "__main__":
    main()
