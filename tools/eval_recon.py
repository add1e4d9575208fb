#!/usr/bin/env python3
"""3D reconstruction metrics of a mesh against the ground truth (the reference's src/tools/eval_recon.py, on the
device): accuracy [cm], completion [cm] and completion ratio [< 5 cm, %] after a point-to-point ICP alignment.

    python tools/eval_recon.py --rec_mesh rec.ply --gt_mesh gt.ply -3d [--no_align] [--n_points 200000] [--seed 0]

-2d (the depth-L1 metric) is not built: it needs a mesh rasteriser, oriented bounds and the dataset's
_pc_unseen.npy.
"""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description="3D reconstruction metrics of a mesh against its ground truth.")
    ap.add_argument("--rec_mesh", type=str, required=True, help="the reconstruction (PLY)")
    ap.add_argument("--gt_mesh", type=str, required=True, help="the ground truth (PLY)")
    ap.add_argument("-2d", "--metric_2d", action="store_true", help="2D metric (not built)")
    ap.add_argument("-3d", "--metric_3d", action="store_true", help="accuracy, completion, completion ratio")
    ap.add_argument("--no_align", action="store_true", help="skip the ICP alignment")
    ap.add_argument("--n_points", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if a.metric_2d:
        raise SystemExit("eval_recon: -2d (depth L1) is not built: it needs a mesh rasteriser, oriented bounds and "
                         "the dataset's _pc_unseen.npy; run -3d")
    if not a.metric_3d:
        raise SystemExit("eval_recon: nothing to do; pass -3d")
    E = importlib.import_module("nice-slam_amd").evaluation
    return E.calc_3d_metric(a.rec_mesh, a.gt_mesh, align=not a.no_align, n_points=a.n_points, seed=a.seed)


if __name__ == "__main__":
    main()
