#!/usr/bin/env python3
"""Prepare a self-recorded RGB-D sequence for a run (the reference's src/tools/prep_own_data.py, without open3d).

    python tools/prep_own_data.py --scene_folder DIR --output_config FILE [--base configs/Own/own.yaml]
                                  [--voxel L] [--trunc T] [--extent E] [--fuse_every N] [--depth_trunc D] [--force]
                                  [--photometric [--photo_weight W] [--photo_th G]]

DIR holds color/*.jpg, depth/*.png (16-bit, millimetres unless the base config says otherwise) and intrinsic.json,
as the Azure Kinect recorder writes them.  When DIR/scene/integrated.ply exists it is used as it is: no odometry,
no GPU.  Otherwise every frame is tracked by depth odometry on the device (nice-slam_amd/odometry.py: ray cast
of a TSDF volume and point-to-plane ICP), every N-th frame (default 5) is fused with its colour, and the tool
writes DIR/scene/trajectory.log (5 lines per frame: a header, then the +z-forward camera-to-world matrix, the
format datasets.Azure reads) and DIR/scene/integrated.ply.  Neither file is overwritten without --force.  If the
odometry lost a frame the tool names the frames and exits with status 2 after writing its files.

Depth alone cannot hold a pose that sees one plane only (a wall, a floor, a table top): such frames are lost.
--photometric adds the colour images to the alignment (a photometric term against the last tracked frame, weighted
by --photo_weight, default odometry.PHOTO_WEIGHT), which holds the pose wherever the plane has texture; --photo_th
leaves out pixels whose grey values (0 to 1) differ by more than G, e.g. 0.1 against blank or badly exposed frames
(default: no gate).  The default weight was tuned on synthetic 48 x 64 images only.

FILE gets what the reference writes: inherit_from, cam (H, W, fx, fy, cx, cy from intrinsic.json), data.input_folder,
data.output, and mapping.bound / mapping.marching_cubes_bound = the mesh's axis-aligned box grown by 1.0 per side
— as valid YAML (the reference's tab-indented tail is not).  --ouput_config, the reference's spelling, is accepted.
Defaults: --voxel 0.01, --trunc 0.04, --extent 6.0 (the half edge of the volume's cube around the first camera),
--depth_trunc 5.0.
"""
import argparse
import glob
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def read_intrinsic(scene_folder):
    with open(os.path.join(scene_folder, "intrinsic.json"), "r") as f:
        k = json.load(f)
    m = k["intrinsic_matrix"]   # column-major 3x3
    return {"H": k["height"], "W": k["width"], "fx": m[0], "fy": m[4], "cx": m[6], "cy": m[7]}


def depth_scale(base):
    """cam.png_depth_scale of the base config when it can be read here, else 1000 (millimetres)."""
    try:
        import yaml
        with open(base, "r") as f:
            return float((yaml.safe_load(f) or {}).get("cam", {}).get("png_depth_scale", 1000.0))
    except (OSError, ValueError, TypeError, AttributeError):
        return 1000.0


def track_and_fuse(a, cam):
    """Odometry over every frame → (poses, mesh dict of numpy arrays, lost frame numbers)."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prep_own_data: no HIP device and no scene/integrated.ply; the odometry has no CPU fallback")
    P = importlib.import_module("nice-slam_amd")
    colors = sorted(glob.glob(os.path.join(a.scene_folder, "color", "*.jpg")))
    depths = sorted(glob.glob(os.path.join(a.scene_folder, "depth", "*.png")))
    if not depths or len(colors) != len(depths):
        raise SystemExit(f"prep_own_data: {len(colors)} colour and {len(depths)} depth images under {a.scene_folder}")
    scale = np.float32(depth_scale(a.base))
    photo = {}
    if a.photometric:
        photo["photo_weight"] = P.odometry.PHOTO_WEIGHT if a.photo_weight is None else a.photo_weight
        photo["photo_th"] = a.photo_th
    od = P.odometry.DepthOdometry(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], a.voxel, a.trunc,
                                  a.extent, "cuda:0", a.depth_trunc, max_jump=a.trunc, fuse_every=a.fuse_every,
                                  color=True, **photo)
    poses, lost = [], []
    for i, (cp, dp) in enumerate(zip(colors, depths)):
        depth = P.datasets._read_depth(dp).astype(np.float32) / scale
        res = od.track(depth, P.datasets._read_color(cp))
        poses.append(res["c2w"])
        if res["lost"]:
            lost.append(i)
    mesh = od.volume.extract_mesh()
    if int(mesh["vertices"].shape[0]) == 0:
        raise SystemExit("prep_own_data: the fused volume has no surface (check the depth scale and --depth_trunc)")
    return poses, {k: (None if v is None else v.cpu().numpy()) for k, v in mesh.items()}, lost


def _num(x):
    """A number as YAML reads it back: integers as they are, floats in positional notation (PyYAML takes 1e-05
    for a string)."""
    return str(x) if isinstance(x, int) else np.format_float_positional(float(x), trim="0")


def write_config(path, a, cam, lo, hi):
    bound = "[" + ",".join(f"[{_num(float(mi) - 1.0)},{_num(float(ma) + 1.0)}]" for mi, ma in zip(lo, hi)) + "]"
    folder = a.scene_folder.rstrip("/\\")
    lines = [f"inherit_from: {json.dumps(a.base)}", "cam:"]
    lines += [f"  {k}: {_num(cam[k])}" for k in ("H", "W", "fx", "fy", "cx", "cy")]
    lines += ["data:", f"  input_folder: {json.dumps(a.scene_folder)}",
              f"  output: {json.dumps('output/Own/' + os.path.basename(folder))}",
              "mapping:", f"  bound: {bound}", f"  marching_cubes_bound: {bound}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description="Trajectory, mesh and config for a self-recorded RGB-D sequence.")
    ap.add_argument("--scene_folder", type=str, required=True, help="folder with color/, depth/ and intrinsic.json")
    ap.add_argument("--output_config", "--ouput_config", dest="output_config", type=str, required=True,
                    help="the YAML config to write")
    ap.add_argument("--base", type=str, default="configs/Own/own.yaml", help="the config to inherit from")
    ap.add_argument("--voxel", type=float, default=0.01, help="voxel edge of the fused volume")
    ap.add_argument("--trunc", type=float, default=0.04, help="truncation distance of the fused volume")
    ap.add_argument("--extent", type=float, default=6.0, help="half edge of the volume's cube around the first camera")
    ap.add_argument("--fuse_every", type=int, default=5, help="fuse every N-th frame")
    ap.add_argument("--depth_trunc", type=float, default=5.0, help="depths beyond this are ignored")
    ap.add_argument("--force", action="store_true", help="overwrite scene/trajectory.log and scene/integrated.ply")
    ap.add_argument("--photometric", action="store_true", help="align the colour images too (textured planes)")
    ap.add_argument("--photo_weight", type=float, default=None, help="weight of the photometric term")
    ap.add_argument("--photo_th", type=float, default=None, help="grey residual gate of the photometric term")
    a = ap.parse_args(argv)
    if a.photo_weight is not None and not (a.photometric and a.photo_weight > 0):
        raise SystemExit("prep_own_data: --photo_weight needs --photometric and a positive weight")
    if a.photo_th is not None and not (a.photometric and a.photo_th >= 0):
        raise SystemExit("prep_own_data: --photo_th needs --photometric and must not be negative")
    if a.fuse_every < 1:
        raise SystemExit("prep_own_data: --fuse_every must be at least 1")
    cam = read_intrinsic(a.scene_folder)
    scene = os.path.join(a.scene_folder, "scene")
    ply, log = os.path.join(scene, "integrated.ply"), os.path.join(scene, "trajectory.log")
    lost = []
    if os.path.exists(ply) and not a.force:
        P = importlib.import_module("nice-slam_amd")
        verts = np.asarray(P.evaluation.load_mesh(ply)["vertices"], dtype=np.float64)
        print(f"prep_own_data: using {ply}")
    else:
        if os.path.exists(log) and not a.force:
            raise SystemExit(f"prep_own_data: {log} exists; pass --force to overwrite it")
        poses, mesh, lost = track_and_fuse(a, cam)
        P = importlib.import_module("nice-slam_amd")
        os.makedirs(scene, exist_ok=True)
        P.odometry.write_trajectory_log(log, poses)
        P.mesher.write_ply(ply, mesh["vertices"], mesh["faces"], mesh["colors"])
        verts = np.asarray(mesh["vertices"], dtype=np.float32).astype(np.float64)   # as the file stores them
        print(f"prep_own_data: wrote {log} ({len(poses)} poses) and {ply} ({verts.shape[0]} vertices)")
    if verts.shape[0] == 0:
        raise SystemExit(f"prep_own_data: {ply} has no vertices")
    write_config(a.output_config, a, cam, verts.min(0), verts.max(0))
    print(f"prep_own_data: wrote {a.output_config}")
    if lost:
        print(f"prep_own_data: the odometry lost frames {lost}: their poses are predictions", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
