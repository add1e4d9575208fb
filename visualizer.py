"""Replay a finished run as rendered frames (the reference's visualizer.py):

    python visualizer.py configs/Replica/room0.yaml --output DIR [--save_rendering] [--no_gt_traj]

It reads what run.py left in DIR: the last checkpoint's pose lists (ckpts/*.tar) and the meshes (mesh/{i:05d}_mesh.ply),
and walks the frames 0 .. idx as the reference does (visualizer.py:64-91), on the device and without a window
(nice-slam_amd/replay.py).  What differs from the reference:
  * one frame is rendered per index; the reference captures one per window refresh, which depends on the wall
    clock.  There are no sleeps;
  * with --save_rendering the frames go to DIR/tmp_rendering/{k:06d}.jpg (k from 1) and then, through ffmpeg when
    it is installed, to DIR/vis.mp4 with the reference's arguments, else to DIR/vis.avi (Motion-JPEG, written
    here).  Without it there is no window to show: only the last frame is written, as DIR/vis_last.jpg;
  * --vis_input_frame shows a cv2 window in the reference and nothing of it reaches the video: it is accepted and
    raises NotImplementedError;
  * --width, --height, --fov, --every, --cull, --point_size are extensions (replay.py: intrinsics, culling).
"""
import argparse
import importlib
import os
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FPS = 30


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Arguments to visualize the SLAM process.")
    parser.add_argument("config", type=str, help="Path to config file.")
    parser.add_argument("--input_folder", type=str,
                        help="input folder, this have higher priority, can overwrite the one in config file")
    parser.add_argument("--output", type=str,
                        help="output folder, this have higher priority, can overwrite the one in config file")
    nice_parser = parser.add_mutually_exclusive_group(required=False)
    nice_parser.add_argument("--nice", dest="nice", action="store_true")
    nice_parser.add_argument("--imap", dest="nice", action="store_false")
    parser.set_defaults(nice=True)
    parser.add_argument("--save_rendering", action="store_true",
                        help="save rendering video to `vis.mp4` (or `vis.avi`) in output folder")
    parser.add_argument("--vis_input_frame", action="store_true", help="visualize input frames (not implemented)")
    parser.add_argument("--no_gt_traj", action="store_true", help="not visualize gt trajectory")
    parser.add_argument("--width", type=int, default=1920)
    parser.add_argument("--height", type=int, default=1080)
    parser.add_argument("--fov", type=float, default=60.0, help="vertical field of view in degrees")
    parser.add_argument("--every", type=int, default=1, help="render every K-th index only")
    parser.add_argument("--cull", choices=("none", "back", "front"), default="none")
    parser.add_argument("--point_size", type=float, default=4)
    return parser.parse_args(argv)


def main(argv=None):
    import torch

    args = parse_args(argv)
    if args.vis_input_frame:
        raise NotImplementedError("--vis_input_frame: the reference's cv2 window of the input frames is not "
                                  "reproduced (nothing of it reaches the rendering)")
    if args.every < 1:
        raise ValueError("--every must be at least 1")
    pkg = importlib.import_module("nice-slam_amd")
    cfg = pkg.config.load_config(args.config, "configs/nice_slam.yaml" if args.nice else "configs/imap.yaml")
    scale = cfg["scale"]
    output = cfg["data"]["output"] if args.output is None else args.output
    ckptsdir = os.path.join(output, "ckpts")
    ckpts = sorted(f for f in os.listdir(ckptsdir) if "tar" in f) if os.path.isdir(ckptsdir) else []
    if not ckpts:
        raise FileNotFoundError(f"{ckptsdir}: no checkpoint (*.tar) to replay")
    ckpt_path = os.path.join(ckptsdir, ckpts[-1])
    print("Get ckpt :", ckpt_path)
    ckpt = torch.load(ckpt_path, map_location=torch.device("cpu"))
    estimate_c2w_list = ckpt["estimate_c2w_list"].clone().double().cpu().numpy()    # copies: the reference divides
    gt_c2w_list = ckpt["gt_c2w_list"].clone().double().cpu().numpy()                # the checkpoint's own tensors
    N = int(ckpt["idx"])
    estimate_c2w_list[:, :3, 3] /= scale
    gt_c2w_list[:, :3, 3] /= scale

    frontend = pkg.replay.Replay(output, init_pose=estimate_c2w_list[0], cam_scale=0.3, near=0,
                                 estimate_c2w_list=estimate_c2w_list, gt_c2w_list=gt_c2w_list, H=args.height,
                                 W=args.width, fov=args.fov, point_size=args.point_size, cull=args.cull).start()
    tmp = os.path.join(output, "tmp_rendering")
    if args.save_rendering:
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp)
    jpegs = []
    for i in range(0, N + 1):
        meshfile = os.path.join(output, "mesh", f"{i:05d}_mesh.ply")
        if os.path.isfile(meshfile):
            frontend.update_mesh(meshfile)
        frontend.update_pose(1, estimate_c2w_list[i], gt=False)
        if not args.no_gt_traj:
            frontend.update_pose(1, gt_c2w_list[i], gt=True)
        if i % 10 == 0:
            frontend.update_cam_trajectory(i, gt=False)
            if not args.no_gt_traj:
                frontend.update_cam_trajectory(i, gt=True)
        if args.save_rendering and i % args.every == 0:
            jpegs.append(frontend.save(os.path.join(tmp, f"{len(jpegs) + 1:06d}.jpg")))
    written = None
    if args.save_rendering:
        ffmpeg = shutil.which("ffmpeg")
        if ffmpeg:
            written = os.path.join(output, "vis.mp4")
            subprocess.run([ffmpeg, "-f", "image2", "-r", str(FPS), "-pattern_type", "glob", "-i",
                            os.path.join(tmp, "*.jpg"), "-y", written], check=True)
        else:
            written = os.path.join(output, "vis.avi")
            pkg.replay.write_mjpeg_avi(written, jpegs, FPS, args.width, args.height)
    else:
        written = os.path.join(output, "vis_last.jpg")
        frontend.save(written)
    print("Wrote", written)
    return {"frames": len(jpegs), "written": written, "frontend": frontend}


if __name__ == "__main__":
    main()
