"""Config loading (src/config.py): YAML files with `inherit_from` chains over a default file.

`load_config(path, default_path=None)` and `update_recursive` keep the reference's semantics: the file named by
`inherit_from` is loaded first (recursively, with the same default underneath), else the default file, and the
given file then overrides it key by key, recursing into dicts.

Relative paths (`inherit_from`, the default file) resolve against the working directory first, as the reference's
plain open() does.  Failing that, they resolve against the directory that contains the given config's `configs/`
ancestor, so `python run.py /data/nice-slam/configs/Replica/room0.yaml` works from anywhere: this repository
ships no config tree of its own.

`get_model(cfg, nice)` forwards to slam.build_decoders (src/conv_onet/config.py:4-33).
"""
from __future__ import annotations

import os

import yaml


def _tree_root(path):
    """The directory holding the `configs/` ancestor of a config file, or None."""
    d = os.path.dirname(os.path.abspath(path))
    while True:
        parent = os.path.dirname(d)
        if os.path.basename(d) == "configs":
            return parent
        if parent == d:
            return None
        d = parent


def _resolve(rel, anchor):
    """`rel` as the reference opens it (working directory), else under the anchor config's tree root."""
    if os.path.isabs(rel) or os.path.exists(rel):
        return rel
    root = _tree_root(anchor)
    if root is not None and os.path.exists(os.path.join(root, rel)):
        return os.path.join(root, rel)
    return rel  # (open() raises FileNotFoundError with the reference's own path)


def load_config(path, default_path=None):
    """src/config.py:10-42."""
    with open(path, "r") as f:
        cfg_special = yaml.full_load(f)
    inherit_from = cfg_special.get("inherit_from")
    if inherit_from is not None:
        cfg = load_config(_resolve(inherit_from, path), None if default_path is None else _resolve(default_path, path))
    elif default_path is not None:
        with open(_resolve(default_path, path), "r") as f:
            cfg = yaml.full_load(f)
    else:
        cfg = dict()
    update_recursive(cfg, cfg_special)
    return cfg


def update_recursive(dict1, dict2):
    """src/config.py:45-59."""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v


def get_model(cfg, nice=True, bound=None, device=None):
    """src/config.py:63-79 → slam.build_decoders.  The reference wires the bound into the decoders afterwards
    (NICE_SLAM.load_bound); here it is an argument (default: the config's own, slam.load_bound)."""
    from .slam import build_decoders, load_bound
    bound = load_bound(cfg) if bound is None else bound
    return build_decoders(cfg, bound, cfg["mapping"]["device"] if device is None else device, nice=nice)
