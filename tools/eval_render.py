#!/usr/bin/env python3
"""Rendering quality of a finished run over the frames it was trained on: PSNR, SSIM, MS-SSIM and rendered-depth
L1 of the map's renders at the estimated poses (evaluation.eval_rendering; LPIPS is not computed).

    python tools/eval_render.py CONFIG [--input_folder DIR] [--output DIR] [--every N] [--mask depth|none]
                                [--nice | --imap] [--save_images]

Reads the last checkpoint of OUTPUT/ckpts (OUTPUT: --output, else the config's data.output), renders every N-th
frame up to the checkpoint's and writes OUTPUT/eval_render.json: the means, the per-frame lists and the arguments.
--mask depth (the default) counts only pixels with a ground-truth depth for the PSNR.  --save_images also writes
OUTPUT/eval_render/{idx:05d}.jpg, rendered | ground truth side by side.  Depth L1 is printed in cm (x 100 / the
config's scale, the convention of tools/eval_recon.py); the JSON holds it in the depth's own unit and in cm.
"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description="PSNR, SSIM, MS-SSIM and depth L1 of a run's renders.")
    ap.add_argument("config", type=str, help="the run's YAML config")
    ap.add_argument("--input_folder", type=str, help="overrides the config's data.input_folder")
    ap.add_argument("--output", type=str, help="output folder; overrides the config's data.output")
    ap.add_argument("--every", type=int, default=5, help="evaluate every N-th frame")
    ap.add_argument("--mask", choices=("depth", "none"), default="depth", help="pixels the PSNR counts")
    grp = ap.add_mutually_exclusive_group(required=False)
    grp.add_argument("--nice", dest="nice", action="store_true")
    grp.add_argument("--imap", dest="nice", action="store_false")
    ap.set_defaults(nice=True)
    ap.add_argument("--save_images", action="store_true", help="write rendered | ground truth JPEGs")
    a = ap.parse_args(argv)
    P = importlib.import_module("nice-slam_amd")
    cfg = P.config.load_config(a.config, "configs/nice_slam.yaml" if a.nice else "configs/imap.yaml")
    output = cfg["data"]["output"] if a.output is None else a.output
    on_frame = None
    if a.save_images:
        import numpy as np
        img_dir = os.path.join(output, "eval_render")
        os.makedirs(img_dir, exist_ok=True)

        def on_frame(idx, color, gt_color):
            pair = np.concatenate([color.float().cpu().numpy(), gt_color.float().cpu().numpy()], axis=1)
            with open(os.path.join(img_dir, f"{int(idx):05d}.jpg"), "wb") as f:
                f.write(P.visualizer.encode_jpeg(P.visualizer._rgb_np(pair)))
    try:
        res = P.evaluation.eval_rendering(cfg, a, every=a.every, mask=a.mask, device=cfg["mapping"]["device"],
                                          on_frame=on_frame)
    except FileNotFoundError as e:
        raise SystemExit(f"eval_render: {e}")
    scale = cfg.get("scale", 1)
    m = res["mean"]
    res["mean"]["depth_l1_cm"] = None if m["depth_l1"] is None else m["depth_l1"] * 100.0 / scale
    res["args"] = {"config": a.config, "input_folder": a.input_folder, "output": output, "every": a.every,
                   "mask": a.mask, "nice": a.nice, "save_images": a.save_images}
    path = os.path.join(output, "eval_render.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)

    def show(v, fmt):
        return "n/a" if v is None else format(v, fmt)
    print(f"frames {len(res['frames'])} (every {a.every}, up to {res['frames'][-1] if res['frames'] else '-'}), "
          f"{res['frames_without_depth']} without a valid depth pixel")
    print(f"PSNR {show(m['psnr'], '.3f')} dB  SSIM {show(m['ssim'], '.4f')}  MS-SSIM {show(m['ms_ssim'], '.4f')}  "
          f"depth L1 {show(m['depth_l1_cm'], '.3f')} cm")
    print("wrote", path)
    return res


if __name__ == "__main__":
    main()
