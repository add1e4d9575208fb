#!/usr/bin/env python3
"""NICE_SLAM.run() at Replica room0's shapes on a synthetic folder, and what one visualisation costs.

    python tools/run_bench.py [--frames 60] [--repeat 5] [--workers 4] [--out profiles/slam_run.json]

  run        A Replica-layout folder of `--frames` synthetic 680x1200 frames (the box scene of tests/golden/scenes.py
             at room0's bound) is written to a temporary directory and NICE_SLAM.run() runs over it with
             configs/Replica/room0.yaml's settings (tracking 10 x 200 px, edges 100; mapping every 5th frame,
             60 x 1000 px, window 5, keyframe_every 50, BA on) and every vis / mesh / ckpt frequency beyond the
             sequence.  Frames/s is the wall time from the start of frame 1 to the start of the last frame
             (synchronised at both ends): the first frame's 1500 iterations and the last frame's colour
             refinement, checkpoint and mesh are left out, graph captures are not (a second run in the same
             process, whose graphs cannot be reused across Mapper objects, would pay them again).  Set against
             bench.py's leg room0_slam_loop on the same machine: the run adds the files' decode and upload
             (prefetch workers), the keyframe selection's read-back, the window's growth (each new window size
             captures its graphs) and the pose lists.
  vis        One visualisation at 680x1200 on the run's final map, each part the median of `--repeat`
             synchronised calls: render_img, nslam_vis_panels (with its max reduction), the device-to-host copy
             of the mosaic, Pillow's JPEG; and, where matplotlib is installed, the reference-layout figure
             (Visualizer.py:57-100) on the same images, which also needs the four float images on the host.
A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, GOLDEN)

import run_scene  # noqa: E402
import scenes  # noqa: E402

ROOM0_BOUND = [[-2.9, 8.9], [-3.2, 5.5], [-3.5, 3.3]]  # configs/Replica/room0.yaml


def write_sequence(folder, n):
    from PIL import Image
    os.makedirs(os.path.join(folder, "results"))
    b = scenes.enlarge_bound(ROOM0_BOUND, 0.32)
    ctr = b.mean(1)
    cam = scenes.ROOM0_CAM
    with open(os.path.join(folder, "traj.txt"), "w") as f:
        for i in range(n):
            c2w = scenes.look_pose(ctr, 0.35 + 0.01 * i, 0.05 + 0.002 * (i % 5), (0.01 * i, -0.005 * i, 0.0))
            depth = scenes.box_depth(c2w, cam, b, seed=900 + i)
            color = scenes.color_image(cam, seed=1000 + i)
            Image.fromarray(np.clip(np.rint(color * 255), 0, 255).astype(np.uint8)).save(
                os.path.join(folder, f"results/frame{i:06d}.jpg"), quality=95)
            Image.fromarray(np.clip(np.rint(depth * 6553.5), 0, 65535).astype(np.uint16)).save(
                os.path.join(folder, f"results/depth{i:06d}.png"))
            m = np.asarray(c2w, dtype=np.float64).copy()
            m[:3, 1] *= -1
            m[:3, 2] *= -1
            f.write(" ".join(f"{v:.17g}" for v in m.ravel()) + "\n")


def config(root, P):
    with open(os.path.join(GOLDEN, "configs", "nice_slam.yaml")) as f:
        cfg = yaml.full_load(f)
    tiny = scenes.load_parts(os.path.join(GOLDEN, "tiny_scene"))
    sd = {k[3:]: torch.from_numpy(v) for k, v in tiny.items() if k.startswith("sd.")}
    coarse, mf = run_scene.write_pretrained(root, sd)
    never = 10 ** 6
    P.config.update_recursive(cfg, {
        "dataset": "replica", "verbose": False, "low_gpu_mem": False, "coarse": False,
        "pretrained_decoders": {"coarse": coarse, "middle_fine": mf},
        "data": {"input_folder": os.path.join(root, "seq"), "output": os.path.join(root, "out")},
        "meshing": {"resolution": 64, "eval_rec": False},
        "tracking": {"vis_freq": never, "vis_inside_freq": 25, "ignore_edge_W": 100, "ignore_edge_H": 100,
                     "seperate_LR": False, "const_speed_assumption": True, "lr": 0.001, "pixels": 200, "iters": 10},
        "mapping": {"bound": ROOM0_BOUND, "marching_cubes_bound": ROOM0_BOUND, "every_frame": 5, "vis_freq": never,
                    "vis_inside_freq": 30, "mesh_freq": never, "ckpt_freq": never, "keyframe_every": 50,
                    "mapping_window_size": 5, "pixels": 1000, "iters_first": 1500, "iters": 60}})
    return cfg


def median_ms(fn, repeat):
    out = []
    for _ in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out[1:]), res


def reference_figure(gd, gc, d, c, path):
    """Visualizer.py:57-100 on host images: the reference's figure, for its cost only."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    dres = np.abs(gd - d)
    dres[gd == 0] = 0
    cres = np.abs(gc - c)
    cres[gd == 0] = 0
    fig, axs = plt.subplots(2, 3)
    fig.tight_layout()
    vmax = np.max(gd)
    for k, img in enumerate((gd, d, dres)):
        axs[0, k].imshow(img, cmap="plasma", vmin=0, vmax=vmax)
    for k, img in enumerate((gc, c, cres)):
        axs[1, k].imshow(np.clip(img, 0, 1), cmap="plasma")
    for ax in axs.ravel():
        ax.set_xticks([])
        ax.set_yticks([])
    plt.subplots_adjust(wspace=0, hspace=0)
    plt.savefig(path, bbox_inches="tight", pad_inches=0.2)
    plt.close(fig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workers", type=int, default=4, help="decode processes of frame_reader.prefetch()")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "slam_run.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("run_bench: needs a HIP device")
    P = importlib.import_module("nice-slam_amd")
    root = tempfile.mkdtemp(prefix="slam_run_")
    try:
        t0 = time.perf_counter()
        write_sequence(os.path.join(root, "seq"), args.frames)
        t_write = time.perf_counter() - t0
        cfg = config(root, P)
        slam = P.NICE_SLAM(cfg, SimpleNamespace(nice=True, output=None, input_folder=None))
        n = slam.n_img
        stamps = {}
        track = slam.tracker.track

        def timed_track(idx, frame):
            if int(idx) in (1, n - 1):
                torch.cuda.synchronize()
                stamps[int(idx)] = time.perf_counter()
            return track(idx, frame)

        slam.tracker.track = timed_track
        slam.prefetch = {"workers": args.workers, "ahead": 2 * args.workers}
        t0 = time.perf_counter()
        slam.run()
        torch.cuda.synchronize()
        t_run = time.perf_counter() - t0
        dt = stamps[n - 1] - stamps[1]
        # the frame source alone, same settings: decode in the workers, upload and normalisation on the device
        t1 = time.perf_counter()
        for _ in slam.frame_reader.prefetch(**slam.prefetch):
            pass
        torch.cuda.synchronize()
        reader_s = time.perf_counter() - t1
        res = {"frames": n, "H": slam.H, "W": slam.W, "run_s": t_run, "sequence_write_s": t_write,
               "first_frame_s": stamps[1] - t0, "last_frame_s": t0 + t_run - stamps[n - 1],
               "steady_frames": n - 2, "frames_per_s": (n - 2) / dt, "ms_per_frame": dt / (n - 2) * 1e3,
               "prefetch_workers": args.workers, "reader_alone_frames_per_s": n / reader_s,
               "tracker_graphs": len(slam.tracker._graphs), "mapper_graphs": len(slam.mapper._graphs),
               "keyframes": list(slam.mapper.keyframe_list)}
        # one visualisation on the final map
        _, gt_color, gt_depth, gt_c2w = slam.frame_reader[n // 2]
        dev = slam.tracker.device
        r, c_, dec = slam.renderer, slam.shared_c, slam.shared_decoders
        gd = gt_depth.float().contiguous()
        gc = gt_color.float().contiguous()
        ms_render, (d, _, col) = median_ms(lambda: r.render_img(c_, dec, gt_c2w, dev, stage="color", gt_depth=gt_depth),
                                           args.repeat)
        ms_panels, mosaic = median_ms(lambda: P.ops.vis_panels(gd, gc, d, col, gd.max()), args.repeat)
        ms_d2h, host = median_ms(lambda: mosaic.cpu().numpy(), args.repeat)
        ms_jpeg, _ = median_ms(lambda: P.visualizer.encode_jpeg(host), args.repeat)
        vis = {"render_img_ms": ms_render, "vis_panels_ms": ms_panels, "mosaic_d2h_ms": ms_d2h, "jpeg_ms": ms_jpeg,
               "mosaic_bytes": int(mosaic.numel()), "total_ms": ms_render + ms_panels + ms_d2h + ms_jpeg}
        ms_f32, imgs = median_ms(lambda: (gd.cpu().numpy(), gc.cpu().numpy(), d.float().cpu().numpy(), col.cpu().numpy()),
                                 args.repeat)
        vis["four_float_images_d2h_ms"] = ms_f32
        try:
            import matplotlib  # noqa: F401
            ms_fig, _ = median_ms(lambda: reference_figure(*imgs, os.path.join(root, "ref.jpg")), min(args.repeat, 3))
            vis["matplotlib_figure_ms"] = ms_fig
        except ImportError:
            vis["matplotlib_figure_ms"] = None
        res["vis"] = vis
        res["device"] = torch.cuda.get_device_name(0)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
