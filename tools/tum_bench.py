#!/usr/bin/env python3
"""The TUM-RGBD additions at the TUM shapes: the lens undistortion and a tracked frame with separate
learning rates.

    python tools/tum_bench.py [--repeat 5] [--variants abc] [--out profiles/tum_frame.json]

  undistort_u8    nslam_undistort_u8 at 480x640x3 (freiburg1's lens): time per frame, as the median of `--repeat`
                  windows of 200 back-to-back launches each (device events around a window), and GB/s on the
                  algorithmic bytes (4 taps x 3 B read + 3 B written per pixel).  One small launch: expected to
                  be launch-bound, so the figure is reported as such, not as a share of the memory peak.
  track_frame     Tracker.track_frame at the TUM tracking shape (configs/TUM_RGBD/tum.yaml: 5000 pixels, 200
                  camera iterations, lr 0.01, edges 20; the 384x512 crop_size image minus crop_edge 8 = 368x496,
                  freiburg1's intrinsics scaled and shifted to match) on bench.py's room0-style synthetic scene.
                  Variants, each with its own Tracker over the same map, one frame per timed window (device
                  events), the windows of the variants alternated in one process, medians of `--repeat` after a
                  warm-up frame each (the graph variants capture there):
                    a  seperate_LR = True, fused = False: the eager autograd loop (what a seperate_LR config ran
                       before the fused camera tail took two rates)
                    b  seperate_LR = True on the fused path: one captured hipGraph per frame
                    c  seperate_LR = False on the fused path: the same graph with one rate
                  b is the launches of c with two constants changed: b / c is expected within 5 % (runs of the
                  frame loop spread about ±2 %).  a / b is the speed-up, recorded as measured.
A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import bench  # noqa: E402  (the room0-style synthetic scene)

FREIBURG1 = {"fx": 517.3, "fy": 516.5, "cx": 318.6, "cy": 255.3}
FREIBURG1_DIST = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def undistort_stage(P, dev, repeat, launches=200):
    H, W, C = 480, 640, 3
    src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, C), dtype=np.uint8)).to(dev)
    out = torch.empty_like(src)
    intr = tuple(FREIBURG1[k] for k in ("fx", "fy", "cx", "cy"))

    def window():
        for _ in range(launches):
            P.ops.undistort_u8(src, *intr, FREIBURG1_DIST, out=out)

    window()
    torch.cuda.synchronize()
    ms = statistics.median(event_ms(window)[0] for _ in range(repeat)) / launches
    nbytes = H * W * (4 * C + C)
    return {"shape": [H, W, C], "us_per_frame": ms * 1e3, "algorithmic_bytes": nbytes,
            "GB_per_s_algorithmic": nbytes / (ms * 1e-3) / 1e9, "launches_per_window": launches,
            "bound": "launch (one 1200-workgroup kernel of a few microseconds; back-to-back launches measure the "
                     "launch rate, not the memory system)"}


def tum_tracking_cfg(seperate_lr):
    s = 384 / 480  # crop_size [384, 512] of a 480x640 image, then crop_edge 8
    cam = {"H": 384 - 16, "W": 512 - 16, "fx": FREIBURG1["fx"] * s, "fy": FREIBURG1["fy"] * s,
           "cx": FREIBURG1["cx"] * s - 8, "cy": FREIBURG1["cy"] * s - 8}
    scene_cfg = dict(bench.ROOM0, **cam)
    cfg = bench.nice_slam_cfg(scene_cfg, tracking_edge=20)
    cfg["tracking"].update(lr=0.01, pixels=5000, iters=200, seperate_LR=seperate_lr)
    return scene_cfg, cfg


def track_stage(P, dev, repeat, variants):
    scene_cfg, _ = tum_tracking_cfg(False)
    scene = bench.Room0Scene(dev, 0, cfg=dict(scene_cfg), path="autograd")
    for t in scene.grids.values():
        t.requires_grad_(False)
    slam = bench.slam_state(scene)
    spec = {"a": (True, False), "b": (True, True), "c": (False, True)}
    trackers = {}
    for v in variants:
        sep, fused = spec[v]
        tr = P.Tracker(tum_tracking_cfg(sep)[1], None, slam)
        tr.fused = fused
        trackers[v] = tr
    nudge = torch.tensor([0.02, -0.01, 0.015], device=dev)
    F = scene_cfg["window"]

    def frame(v, i):
        f = i % F
        gt = bench._pose4(scene.c2w[f])
        pre = gt.clone()
        pre[:3, 3] += nudge
        return trackers[v].track_frame(i + 1, scene.color[f], scene.depth[f], gt, pre_c2w=pre)

    for v in variants:  # warm-up (the graph variants capture here)
        frame(v, 0)
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    for r in range(repeat):
        for v in variants:  # alternated windows
            ms[v].append(event_ms(lambda: frame(v, r + 1))[0])
    res = {"shape": {"H": scene_cfg["H"], "W": scene_cfg["W"], "pixels": 5000, "iters": 200, "lr": 0.01,
                     "ignore_edge": 20, "scene": "bench.py Room0Scene (synthetic room0 grids and decoders)"},
           "ms_per_frame": {v: statistics.median(ms[v]) for v in variants}, "ms_windows": ms,
           "graphs": {v: len(trackers[v]._graphs) for v in variants},
           "variants": {"a": "seperate_LR, fused=False: eager autograd loop", "b": "seperate_LR, fused: one hipGraph",
                        "c": "single rate, fused: one hipGraph"}}
    m = res["ms_per_frame"]
    if "b" in m and "c" in m:
        res["b_over_c"] = m["b"] / m["c"]
        res["b_within_5_percent_of_c"] = bool(abs(m["b"] / m["c"] - 1.0) <= 0.05)
    if "a" in m and "b" in m:
        res["speedup_a_over_b"] = m["a"] / m["b"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--variants", default="abc", help="track_frame variants to time (a, b, c)")
    ap.add_argument("--no-undistort", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tum_frame.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tum_bench.py needs a HIP device")
    P = importlib.import_module("nice-slam_amd")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "repeat": args.repeat,
           "method": "device events, one warm-up, medians; track_frame variants alternated in one process"}
    if not args.no_undistort:
        out["undistort_u8"] = undistort_stage(P, dev, args.repeat)
        print(json.dumps({"undistort_u8": out["undistort_u8"]}), flush=True)
    out["track_frame"] = track_stage(P, dev, args.repeat, [v for v in "abc" if v in args.variants])
    print(json.dumps({"track_frame": out["track_frame"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
