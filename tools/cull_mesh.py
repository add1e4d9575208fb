#!/usr/bin/env python3
"""Drop the mesh faces no camera of a trajectory sees (the reference's src/tools/cull_mesh.py, on the device).

    python tools/cull_mesh.py --input_mesh mesh.ply --traj traj.txt --output_mesh culled.ply
                              [--H 680 --W 1200 --fx 600 --fy 600 --cx 599.5 --cy 339.5]

traj.txt holds one camera-to-world matrix per line (16 numbers), as the Replica dataset ships them.  Vertices are
kept (trimesh's update_faces keeps them too); the output is a binary PLY with the input's vertex colours.
"""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Drop the mesh faces that no camera of the trajectory sees.")
    ap.add_argument("--input_mesh", type=str, required=True, help="the PLY to cull")
    ap.add_argument("--traj", type=str, required=True, help="text file, one 4x4 camera-to-world matrix per line")
    ap.add_argument("--output_mesh", type=str, required=True, help="the PLY to write")
    for name, val in (("H", 680), ("W", 1200)):
        ap.add_argument("--" + name, type=int, default=val)
    for name, val in (("fx", 600.0), ("fy", 600.0), ("cx", 599.5), ("cy", 339.5)):
        ap.add_argument("--" + name, type=float, default=val)
    a = ap.parse_args(argv)
    E = importlib.import_module("nice-slam_amd").evaluation
    mesh = E.load_mesh(a.input_mesh)
    poses = E.load_poses(a.traj)
    out = E.cull_mesh(mesh, poses, a.H, a.W, a.fx, a.fy, a.cx, a.cy)
    E.write_ply(a.output_mesh, out["vertices"], out["faces"], out["colors"])
    print(f"{a.output_mesh}: kept {out['faces'].shape[0]} of {mesh['faces'].shape[0]} faces "
          f"({mesh['vertices'].shape[0]} vertices, {poses.shape[0]} poses)")


if __name__ == "__main__":
    main()
