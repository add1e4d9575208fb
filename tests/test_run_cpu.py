"""The SLAM system's scheduling layer on the CPU: config loading, the pretrained-decoder loader, and
NICE_SLAM.run() against the trace the reference's own Tracker.run / Mapper.run left
(tests/golden/run_trace.json, tests/golden/make_golden_run.py).

The five entry points below the frame loops are replaced by the recorders that produced the trace
(tests/golden/run_scene.py), so the scheduling layer must make no kernel call of its own.
"""
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import yaml

from conftest import GOLDEN, sd_from

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import run_scene  # noqa: E402

CONFIGS = os.path.join(GOLDEN, "configs")


# ------------------------------------------------------------------------------------------------
# config.load_config
# ------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    root = tmp_path / "elsewhere"
    (root / "configs" / "Scene").mkdir(parents=True)
    (root / "configs" / "default.yaml").write_text(yaml.safe_dump(
        {"scale": 1, "mapping": {"iters": 60, "stage": {"color": {"color_lr": 0.005, "fine_lr": 0.005}}},
         "tracking": {"lr": 0.001}}))
    (root / "configs" / "Scene" / "common.yaml").write_text(yaml.safe_dump(
        {"dataset": "replica", "mapping": {"iters": 30, "stage": {"color": {"fine_lr": 0.01}}}, "cam": {"H": 4}}))
    (root / "configs" / "Scene" / "room.yaml").write_text(yaml.safe_dump(
        {"inherit_from": "configs/Scene/common.yaml", "mapping": {"bound": [[0, 1], [0, 1], [0, 1]]},
         "cam": {"W": 6}, "tracking": {"lr": 0.002}}))
    return root


def test_load_config_inherits_over_the_default(pkg, tmp_path, monkeypatch):
    root = _tree(tmp_path)
    want = {"scale": 1, "dataset": "replica", "inherit_from": "configs/Scene/common.yaml",
            "mapping": {"iters": 30, "bound": [[0, 1], [0, 1], [0, 1]],
                        "stage": {"color": {"color_lr": 0.005, "fine_lr": 0.01}}},
            "tracking": {"lr": 0.002}, "cam": {"H": 4, "W": 6}}
    # from the tree's own root, as the reference is run: plain relative paths
    monkeypatch.chdir(root)
    assert pkg.config.load_config("configs/Scene/room.yaml", "configs/default.yaml") == want
    # from anywhere else: the relative paths resolve against the tree that holds the given config
    monkeypatch.chdir(tmp_path)
    assert pkg.config.load_config(str(root / "configs" / "Scene" / "room.yaml"), "configs/default.yaml") == want
    # no default, no inherit_from: the file itself
    assert pkg.config.load_config(str(root / "configs" / "default.yaml")) == \
        {"scale": 1, "mapping": {"iters": 60, "stage": {"color": {"color_lr": 0.005, "fine_lr": 0.005}}},
         "tracking": {"lr": 0.001}}
    with pytest.raises(FileNotFoundError):
        pkg.config.load_config(str(root / "configs" / "Scene" / "room.yaml"), "configs/missing.yaml")


def test_update_recursive(pkg):
    a = {"x": {"y": 1, "z": 2}, "k": 1}
    pkg.config.update_recursive(a, {"x": {"y": 5, "w": {"v": 0}}, "n": 3})
    assert a == {"x": {"y": 5, "z": 2, "w": {"v": 0}}, "k": 1, "n": 3}


def test_committed_config_tree(pkg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = pkg.config.load_config(os.path.join(CONFIGS, "run_a.yaml"), "configs/nice_slam.yaml")
    assert cfg["mapping"]["every_frame"] == 2 and cfg["mapping"]["keyframe_every"] == 2
    assert cfg["mapping"]["stage"]["color"]["color_lr"] == 0.005  # (the default underneath)
    assert cfg["mapping"]["lr_first_factor"] == 5 and cfg["cam"] == dict(run_scene.CAM, png_depth_scale=1.0, crop_edge=0)
    assert cfg["coarse"] is False and cfg["sync_method"] == "strict"


# ------------------------------------------------------------------------------------------------
# NICE_SLAM on CPU tensors
# ------------------------------------------------------------------------------------------------
def _cfg(pkg, name, tmp_path, sd):
    cfg = pkg.config.load_config(os.path.join(CONFIGS, run_scene.CONFIGS[name]), "configs/nice_slam.yaml")
    coarse, mf = run_scene.write_pretrained(str(tmp_path), sd)
    cfg["pretrained_decoders"] = {"coarse": coarse, "middle_fine": mf}
    cfg["data"]["output"] = str(tmp_path / "out")
    return cfg


def _slam(pkg, cfg, n, monkeypatch):
    monkeypatch.setattr(pkg.NICE_SLAM, "_frame_reader", staticmethod(lambda cfg, args, device: run_scene.Frames(n)))
    return pkg.NICE_SLAM(cfg, SimpleNamespace(nice=True, output=None, input_folder=None))


def test_load_pretrain(pkg, tiny, tmp_path, monkeypatch, capsys):
    sd = sd_from(tiny)
    cfg = _cfg(pkg, "A", tmp_path, sd)
    cfg["coarse"] = True
    slam = _slam(pkg, cfg, 3, monkeypatch)
    got = slam.shared_decoders.state_dict()
    for name in ("coarse_decoder", "middle_decoder", "fine_decoder"):
        keys = [k for k in sd if k.startswith(name + ".")]
        assert keys
        for k in keys:
            assert torch.equal(got[k], sd[k]), k
    # the colour decoder has no pretrained file: it keeps its own initialisation
    assert not torch.equal(got["color_decoder.output_linear.weight"], sd["color_decoder.output_linear.weight"])
    assert slam.n_img == 3 and slam.ckptsdir == os.path.join(slam.output, "ckpts")
    assert os.path.isdir(slam.ckptsdir) and os.path.isdir(os.path.join(slam.output, "mesh"))
    assert hasattr(slam, "coarse_mapper") and slam.coarse_mapper.coarse_mapper
    out = capsys.readouterr().out
    assert f"INFO: The output folder is {slam.output}" in out and "tracking_vis/ and" in out
    # a missing file names its config key
    cfg["pretrained_decoders"]["middle_fine"] = str(tmp_path / "nowhere.pt")
    with pytest.raises(FileNotFoundError, match="pretrained_decoders.middle_fine"):
        _slam(pkg, cfg, 3, monkeypatch)
    # iMAP*: no grids, nothing loaded
    icfg = pkg.config.load_config(os.path.join(CONFIGS, "run_b.yaml"), "configs/imap.yaml")
    icfg["pretrained_decoders"] = {"coarse": "nowhere.pt", "middle_fine": "nowhere.pt"}
    icfg["data"]["output"] = str(tmp_path / "imap_out")
    icfg["occupancy"] = False
    monkeypatch.setattr(pkg.NICE_SLAM, "_frame_reader", staticmethod(lambda cfg, args, device: run_scene.Frames(2)))
    islam = pkg.NICE_SLAM(icfg, SimpleNamespace(nice=False, output=None, input_folder=None))
    assert islam.shared_c == {} and not hasattr(islam, "coarse_mapper")


@pytest.fixture(scope="module")
def trace():
    with open(os.path.join(GOLDEN, "run_trace.json")) as f:
        return json.load(f)


def _install(pkg, rec, monkeypatch):
    monkeypatch.setattr(pkg.Tracker, "optimize_cam_in_batch", rec.bind("optimize_cam_in_batch"))
    monkeypatch.setattr(pkg.Mapper, "optimize_map", rec.bind("optimize_map"))
    monkeypatch.setattr(pkg.Mesher, "get_mesh", rec.bind("get_mesh"))
    monkeypatch.setattr(pkg.Logger, "log", rec.bind("log"))
    monkeypatch.setattr(pkg.Visualizer, "vis", rec.bind("vis"))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_run_matches_the_reference_trace(pkg, tiny, trace, tmp_path, monkeypatch, name):
    want = trace[name]
    cfg = _cfg(pkg, name, tmp_path, sd_from(tiny))
    rec = run_scene.Recorder()
    _install(pkg, rec, monkeypatch)
    slam = _slam(pkg, cfg, run_scene.N_IMG[name], monkeypatch)
    slam.tracker.fused = False  # (the autograd camera loop: it calls optimize_cam_in_batch per iteration)
    slam.run()
    # event for event, floats bit for bit (JSON keeps a float32's double exactly)
    assert len(rec.mapper) == len(want["mapper"]), [(e["kind"], e["idx"]) for e in rec.mapper]
    for got, ref in zip(rec.mapper, want["mapper"]):
        assert got == ref, (got, ref)
    assert len(rec.tracker) == len(want["tracker"]), [(e["kind"], e["idx"]) for e in rec.tracker]
    for got, ref in zip(rec.tracker, want["tracker"]):
        assert got == ref, (got, ref)
    assert sorted(os.listdir(os.path.join(slam.output, "mesh"))) == want["mesh_files"]
    counters = {"idx": slam.idx, "mapping_idx": slam.mapping_idx, "mapping_cnt": slam.mapping_cnt,
                "mapping_first_frame": slam.mapping_first_frame}
    assert rec.final(slam.estimate_c2w_list, slam.gt_c2w_list, slam.mapper, counters) == want["final"]
    if name == "B":  # save_selected_keyframes_info: the dict reaches the logger
        assert all(e["selected"] for e in rec.mapper if e["kind"] == "ckpt")
