#!/usr/bin/env python3
"""Absolute trajectory error of a run (the reference's src/tools/eval_ate.py, without its plot).

    python tools/eval_ate.py CONFIG [--output DIR] [--scale S]

Reads the last checkpoint of DIR/ckpts (DIR: --output, else the config's data.output) with the package's
checkpoint loader, masks ground-truth poses holding NaN or inf, aligns the estimate onto the ground truth in
closed form (Horn) and prints the reference's result dict.  CONFIG is the run's YAML (its inherit_from chain is
followed, configs/nice_slam.yaml is the default); only `scale` and `data.output` are read, and --scale / --output
override them.
"""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def load_config(path, default_path=None):
    """The YAML at `path` over its inherit_from chain (or default_path when the chain ends)."""
    import yaml

    def merge(dst, src):
        for k, v in src.items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = v
        return dst
    with open(path, "r") as f:
        special = yaml.safe_load(f) or {}
    parent = special.get("inherit_from")
    if parent is not None:
        cfg = load_config(parent, default_path)
    elif default_path is not None and os.path.exists(default_path):
        with open(default_path, "r") as f:
            cfg = yaml.safe_load(f) or {}
    else:
        cfg = {}
    return merge(cfg, special)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Absolute trajectory error of a run's last checkpoint.")
    ap.add_argument("config", type=str, help="the run's YAML config")
    ap.add_argument("--output", type=str, help="output folder; overrides the config's data.output")
    ap.add_argument("--scale", type=float, help="overrides the config's scale")
    a = ap.parse_args(argv)
    cfg = load_config(a.config, "configs/nice_slam.yaml")
    scale = a.scale if a.scale is not None else cfg.get("scale", 1)
    output = a.output if a.output is not None else cfg.get("data", {}).get("output")
    if output is None:
        raise SystemExit("eval_ate: no output folder (pass --output or set data.output in the config)")
    ckptsdir = os.path.join(output, "ckpts")
    ckpts = sorted(f for f in os.listdir(ckptsdir) if "tar" in f) if os.path.isdir(ckptsdir) else []
    if not ckpts:
        raise SystemExit(f"eval_ate: no checkpoint under {ckptsdir}")
    path = os.path.join(ckptsdir, ckpts[-1])
    print("Get ckpt :", path)
    P = importlib.import_module("nice-slam_amd")
    ck = P.datasets.load_checkpoint(path, device="cpu")  # the trajectory is host work: the grids stay there too
    res = P.evaluation.evaluate_ate_checkpoint(ck, scale)
    print(res)
    return res


if __name__ == "__main__":
    main()
