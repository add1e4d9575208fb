"""The SLAM system end to end on the device, through run.py's main: a synthetic Replica-layout folder (96 x 128
frames of the tiny box scene), synthesised pretrained decoders, small iteration counts.

What is checked is the system's bookkeeping, not tracking accuracy (nobody has measured what this synthetic
scene reaches): the call sequence against the CPU scheduler's for the same config (whose own sequence is pinned
to the reference's by tests/test_run_cpu.py), the pose lists and keyframe poses bit for bit against the recorded
returns of track_frame / optimize_map, the files a run leaves, and that frames without a visualisation replay
the cached graphs.
"""
import importlib
import os
import shutil
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from conftest import GOLDEN, REPO, sd_from

sys.path.insert(0, GOLDEN)
import run_scene  # noqa: E402
import scenes  # noqa: E402

if REPO not in sys.path:
    sys.path.insert(0, REPO)
import run as run_py  # noqa: E402

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
CAM = scenes.TINY_CAM
POSE_KEYS = ("cur_c2w", "est", "pose", "cam0")


def write_sequence(folder, n):
    """results/frame%06d.jpg, results/depth%06d.png, traj.txt (datasets.Replica) of a camera swinging through
    the tiny box → the poses as the loader hands them out."""
    os.makedirs(os.path.join(folder, "results"))
    b = scenes.enlarge_bound(scenes.TINY_BOUND, 0.32)
    ctr = b.mean(1)
    poses = []
    with open(os.path.join(folder, "traj.txt"), "w") as f:
        for i in range(n):
            c2w = scenes.look_pose(ctr, 0.5 + 0.02 * i, 0.3 + 0.01 * (i % 3), (0.01 * i, -0.008 * i, 0.004 * (i % 2)))
            depth = scenes.box_depth(c2w, CAM, b, seed=700 + i)
            color = scenes.color_image(CAM, seed=800 + i)
            Image.fromarray(np.clip(np.rint(color * 255), 0, 255).astype(np.uint8)).save(
                os.path.join(folder, f"results/frame{i:06d}.jpg"), quality=95)
            Image.fromarray(np.clip(np.rint(depth * 6553.5), 0, 65535).astype(np.uint16)).save(
                os.path.join(folder, f"results/depth{i:06d}.png"))
            m = np.asarray(c2w, dtype=np.float64).copy()
            m[:3, 1] *= -1  # (the loader flips y and z back)
            m[:3, 2] *= -1
            f.write(" ".join(f"{v:.17g}" for v in m.ravel()) + "\n")
            poses.append(torch.from_numpy(np.asarray(c2w, dtype=np.float32)))
    return poses


def write_config(root, name, over):
    """root/configs/<name>.yaml over copies of the two default files (resolved through the config's own tree)."""
    os.makedirs(os.path.join(root, "configs"), exist_ok=True)
    for f in ("nice_slam.yaml", "imap.yaml"):
        shutil.copyfile(os.path.join(GOLDEN, "configs", f), os.path.join(root, "configs", f))
    cfg = {"dataset": "replica", "coarse": False, "verbose": False, "low_gpu_mem": False, "scale": 1,
           "data": {"input_folder": "unused", "output": os.path.join(root, "unused_out")},
           "cam": dict(CAM, png_depth_scale=6553.5, crop_edge=0),
           "meshing": {"resolution": 32},
           "tracking": {"iters": 4, "pixels": 200, "ignore_edge_W": 10, "ignore_edge_H": 10, "vis_freq": 3,
                        "vis_inside_freq": 2},
           "mapping": {"bound": scenes.TINY_BOUND, "marching_cubes_bound": [[0.1, 2.9], [-0.4, 2.1], [0.3, 2.4]],
                       "every_frame": 1, "keyframe_every": 1, "iters_first": 30, "iters": 10, "pixels": 400,
                       "ckpt_freq": 3, "mesh_freq": 4, "vis_freq": 4, "vis_inside_freq": 5}}
    P.config.update_recursive(cfg, over)
    path = os.path.join(root, "configs", name + ".yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


class Calls(run_scene.Recorder):
    """The recorders wrapped around the real entry points: record, then call through; plus the returns of
    track_frame / optimize_map and the graph replays each frame made."""

    def __init__(self, monkeypatch, graphs):
        super().__init__()
        self.track_ret, self.map_ret, self.kf_after, self.replays = {}, [], [], {"track": {}, "map": {}}
        self.n_replay = 0
        rec = self
        real_replay = torch.cuda.CUDAGraph.replay

        def replay(g):
            rec.n_replay += 1
            return real_replay(g)

        monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
        real = {k: getattr(c, k) for c, k in ((P.Tracker, "track_frame"), (P.Mapper, "optimize_map"),
                                              (P.Mesher, "get_mesh"), (P.Logger, "log"), (P.Visualizer, "vis"))}

        def track_frame(self, idx, *a, **k):
            n0 = rec.n_replay
            out = real["track_frame"](self, idx, *a, **k)
            rec.track_ret[int(idx)] = out.detach().clone()
            rec.replays["track"][int(idx)] = rec.n_replay - n0
            return out

        def optimize_map(self, num_joint_iters, lr_factor, idx, *a, **k):
            run_scene.Recorder.optimize_map(rec, self, num_joint_iters, lr_factor, idx, *a, **k)
            n0 = rec.n_replay
            out = real["optimize_map"](self, num_joint_iters, lr_factor, idx, *a, **k)
            rec.map_ret.append((int(idx), bool(self.BA), None if out is None else out.detach().clone()))
            rec.kf_after.append([kf["est_c2w"].detach().clone() for kf in self.keyframe_dict])
            rec.replays["map"].setdefault(int(idx), 0)
            rec.replays["map"][int(idx)] += rec.n_replay - n0
            return out

        def get_mesh(self, *a, **k):
            run_scene.Recorder.get_mesh(rec, self, *a, **k)
            return real["get_mesh"](self, *a, **k)

        def log(self, *a, **k):
            run_scene.Recorder.log(rec, self, *a, **k)
            return real["log"](self, *a, **k)

        def vis(self, *a, **k):
            run_scene.Recorder.vis(rec, self, *a, **k)
            return real["vis"](self, *a, **k)

        for cls, fn in ((P.Tracker, track_frame), (P.Mapper, optimize_map), (P.Mesher, get_mesh), (P.Logger, log),
                        (P.Visualizer, vis)):
            monkeypatch.setattr(cls, fn.__name__, fn)
        real_init = P.NICE_SLAM.__init__

        def init(self, cfg, args):
            real_init(self, cfg, args)
            self.mapper.graphs = self.tracker.graphs = graphs
            # (the run with graphs keeps a decode worker process; the others read in-process: no fork)
            self.prefetch = {"workers": 1, "ahead": 2} if graphs else {"workers": 0}

        monkeypatch.setattr(P.NICE_SLAM, "__init__", init)


def schedule(events, kinds=None):
    return [{k: v for k, v in e.items() if k not in POSE_KEYS} for e in events if kinds is None or e["kind"] in kinds]


def cpu_schedule(cfg_path, n, tmp_path, nice, sd, monkeypatch):
    """What the CPU scheduler does for the same config (the five entry points replaced by the recorders)."""
    cfg = P.config.load_config(cfg_path, "configs/nice_slam.yaml" if nice else "configs/imap.yaml")
    cfg["mapping"]["device"] = cfg["tracking"]["device"] = "cpu"
    cfg["data"]["output"] = str(tmp_path / ("cpu_out_Demo" if "Demo" in cfg["data"]["output"] else "cpu_out"))
    if nice:
        coarse, mf = run_scene.write_pretrained(str(tmp_path), sd)
        cfg["pretrained_decoders"] = {"coarse": coarse, "middle_fine": mf}
    rec = run_scene.Recorder()
    with monkeypatch.context() as mp:
        for cls, name in ((P.Tracker, "optimize_cam_in_batch"), (P.Mapper, "optimize_map"), (P.Mesher, "get_mesh"),
                          (P.Logger, "log"), (P.Visualizer, "vis")):
            mp.setattr(cls, name, rec.bind(name))
        mp.setattr(P.NICE_SLAM, "_frame_reader", staticmethod(lambda cfg, args, device: run_scene.Frames(n)))
        slam = P.NICE_SLAM(cfg, SimpleNamespace(nice=nice, output=None, input_folder=None))
        slam.tracker.fused = False
        slam.run()
    return rec


def run_system(tmp_path, monkeypatch, tiny, name, n, over, graphs, nice=True, out="out"):
    seq = str(tmp_path / "seq")
    poses = write_sequence(seq, n)
    sd = sd_from(tiny)
    if nice:
        coarse, mf = run_scene.write_pretrained(str(tmp_path), sd)
        over = dict(over, pretrained_decoders={"coarse": coarse, "middle_fine": mf})
    path = write_config(str(tmp_path), name, over)
    want = cpu_schedule(path, n, tmp_path, nice, sd, monkeypatch)
    calls = Calls(monkeypatch, graphs)
    torch.manual_seed(5)
    np.random.seed(5)
    slam = run_py.main([path, "--input_folder", seq, "--output", str(tmp_path / out)] + ([] if nice else ["--imap"]))
    torch.cuda.synchronize()
    return slam, calls, want, poses


def check_schedule(calls, want):
    # (the CPU run's optimize_map is a recorder, so the visualiser inside it is seen on the device run only)
    assert schedule(calls.mapper, ("map", "ckpt", "mesh")) == schedule(want.mapper)
    assert schedule(calls.tracker, ("vis",)) == schedule(want.tracker, ("vis",))


def check_vis_files(slam, calls):
    for stream, folder in ((calls.tracker, slam.tracker.visualizer.vis_dir),
                           (calls.mapper, None if slam.mapper.visualizer is None else slam.mapper.visualizer.vis_dir)):
        names = sorted(f"{e['idx']:05d}_{e['iter']:04d}.jpg" for e in stream if e["kind"] == "vis")
        if folder is not None:
            assert sorted(os.listdir(folder)) == names, folder
            for f in names:
                with Image.open(os.path.join(folder, f)) as im:
                    assert im.size == (3 * CAM["W"], 2 * CAM["H"])
        else:
            assert names == []


def test_run_bookkeeping(tmp_path, monkeypatch, tiny):
    n = 8
    slam, calls, want, poses = run_system(tmp_path, monkeypatch, tiny, "gpu", n, {}, graphs=False)
    check_schedule(calls, want)
    maps = [e for e in calls.mapper if e["kind"] == "map"]
    assert [e["idx"] for e in maps] == [0, 1, 2, 3, 4, 5, 6] + [7] * 5       # colour refinement: 5 outer iterations
    assert [e["BA"] for e in maps] == [False] * 5 + [True] * 7                # from the fifth keyframe on
    assert maps[0]["num_joint_iters"] == 30 and maps[0]["lr_factor"] == 5.0 and maps[-1]["num_joint_iters"] == 10
    assert maps[-1]["window"] == 10 and maps[-1]["fix_color"] and not maps[-1]["frustum"]
    # the pose list: frame 0 is the ground truth, every later one its track_frame return or the BA write-back
    est = slam.estimate_c2w_list
    assert torch.equal(est[0], poses[0]) and torch.equal(slam.gt_c2w_list, torch.stack(poses))
    ba = {}
    for idx, on, out in calls.map_ret:
        if on:
            ba[idx] = out
    assert sorted(ba) == [5, 6, 7] and sorted(calls.track_ret) == list(range(1, n))
    for i in range(1, n):
        exp = ba.get(i, calls.track_ret[i])
        assert torch.equal(est[i], exp.cpu()), i
    assert any(not torch.equal(ba[i].cpu(), calls.track_ret[i].cpu()) for i in ba)  # (BA did move a pose)
    # keyframes: inserted with the frame's pose, then moved by BA alone
    kfs = slam.mapper.keyframe_dict
    assert slam.mapper.keyframe_list == list(range(n)) and [kf["idx"] for kf in kfs] == list(range(n))
    last = calls.kf_after[-1]
    assert len(last) == n - 1
    for j in range(n - 1):
        assert torch.equal(kfs[j]["est_c2w"], last[j]), j
    assert torch.equal(kfs[n - 1]["est_c2w"].cpu(), est[n - 1])
    prev = []
    for (idx, on, out), snap in zip(calls.map_ret, calls.kf_after):
        if not on:  # without BA a call moves no keyframe
            assert len(snap) == len(prev) or len(snap) == len(prev) + 1
            assert all(torch.equal(a, b) for a, b in zip(snap, prev))
            if len(snap) == len(prev) + 1:  # the keyframe the previous frame inserted: with that frame's pose
                assert torch.equal(snap[-1].cpu(), est[len(snap) - 1]) or len(snap) - 1 in ba
        prev = snap
    assert int(slam.idx[0]) == n - 1 and int(slam.mapping_idx[0]) == n - 1 and int(slam.mapping_cnt[0]) == n
    # files: checkpoints with the reference's keys, meshes, visualisations
    assert sorted(os.listdir(slam.ckptsdir)) == ["00003.tar", "00006.tar", "00007.tar"]
    ck = P.datasets.load_checkpoint(os.path.join(slam.ckptsdir, "00007.tar"))
    assert set(ck) == {"c", "decoder_state_dict", "gt_c2w_list", "estimate_c2w_list", "keyframe_list",
                       "selected_keyframes", "idx"}
    assert torch.equal(ck["estimate_c2w_list"], est) and ck["keyframe_list"] == list(range(n)) and int(ck["idx"]) == 7
    assert set(ck["c"]) == {"grid_middle", "grid_fine", "grid_color"}
    for k, v in slam.shared_c.items():
        assert torch.equal(ck["c"][k], v)
    mesh = P.mesher.read_ply(os.path.join(slam.output, "mesh", "final_mesh.ply"))
    assert mesh["vertices"].shape[0] > 0 and mesh["faces"].shape[0] > 0 and mesh["faces"].max() < mesh["vertices"].shape[0]
    assert sorted(os.listdir(os.path.join(slam.output, "mesh"))) == ["00004_mesh.ply", "00007_mesh.ply", "final_mesh.ply"]
    with open(os.path.join(slam.output, "mesh", "final_mesh.ply"), "rb") as a, \
            open(os.path.join(slam.output, "mesh", "00007_mesh.ply"), "rb") as b:
        assert a.read() == b.read()
    check_vis_files(slam, calls)
    assert [(e["idx"], e["iter"]) for e in calls.tracker if e["kind"] == "vis"] == [(3, 0), (3, 2), (6, 0), (6, 2)]
    assert [(e["idx"], e["iter"]) for e in calls.mapper if e["kind"] == "vis"] == [(4, 0), (4, 5)]


def test_run_replays_graphs_off_the_vis_frames(tmp_path, monkeypatch, tiny):
    """Graphs on: a window of two frames and no BA / refinement, so one stage-graph set serves frames 1..4."""
    over = {"mapping": {"mapping_window_size": 2, "BA": False, "color_refine": False, "vis_freq": 3, "ckpt_freq": 50,
                        "mesh_freq": 50, "iters_first": 10, "iters": 5, "vis_inside_freq": 3},
            "tracking": {"vis_freq": 2, "vis_inside_freq": 3}, "meshing": {"resolution": 16}}
    slam, calls, want, poses = run_system(tmp_path, monkeypatch, tiny, "graphs", 5, over, graphs=True)
    check_schedule(calls, want)
    check_vis_files(slam, calls)
    # tracking: frames 2 and 4 visualise (eager), 1 and 3 replay the frame graph
    assert calls.replays["track"] == {1: 1, 2: 0, 3: 1, 4: 0}
    # (two graphs: frame 1 has no second-last pose for the constant-speed guess, frame 3 has)
    assert sorted(k.speed for k in slam.tracker._graphs) == [False, True]
    # mapping: the first frame's one-off schedule and frame 3 (it visualises) run eagerly; the others replay
    # the setup graph and one graph per stage
    assert calls.replays["map"][0] == 0 and calls.replays["map"][3] == 0
    assert all(calls.replays["map"][i] >= 3 for i in (1, 2, 4)), calls.replays["map"]
    assert any(k.kind == "stage" for k in slam.mapper._graphs)
    est = slam.estimate_c2w_list
    assert torch.equal(est[0], poses[0])
    for i in range(1, 5):
        assert torch.equal(est[i], calls.track_ret[i].cpu()), i


def test_run_demo_output_has_one_vis_folder(tmp_path, monkeypatch, tiny):
    over = {"mapping": {"color_refine": False, "iters_first": 10, "iters": 5, "vis_freq": 1, "ckpt_freq": 50,
                        "mesh_freq": 50},
            "tracking": {"vis_freq": 1, "vis_inside_freq": 2}, "meshing": {"resolution": 16},
            "data": {"output": "Demo_unused"}}
    slam, calls, want, _ = run_system(tmp_path, monkeypatch, tiny, "demo", 3, over, graphs=False, out="Demo_out")
    check_schedule(calls, want)
    assert slam.mapper.visualizer is None and os.path.basename(slam.tracker.visualizer.vis_dir) == "vis"
    assert sorted(os.listdir(slam.output)) == ["ckpts", "mesh", "vis"]
    check_vis_files(slam, calls)
    assert sorted(os.listdir(os.path.join(slam.output, "vis"))) == ["00001_0000.jpg", "00001_0002.jpg", "00002_0000.jpg",
                                                                   "00002_0002.jpg"]


def test_run_with_the_coarse_mapper(tmp_path, monkeypatch, tiny):
    """cfg['coarse']: the coarse mapper maps every frame the mapper maps, right after it, with its own keyframes."""
    over = {"coarse": True, "mapping": {"color_refine": False, "iters_first": 10, "iters": 5, "vis_freq": 50,
                                        "ckpt_freq": 50, "mesh_freq": 50, "every_frame": 2},
            "tracking": {"vis_freq": 50}, "meshing": {"resolution": 16}}
    slam, calls, want, poses = run_system(tmp_path, monkeypatch, tiny, "coarse", 4, over, graphs=False)
    check_schedule(calls, want)
    maps = [(e["idx"], e["coarse"]) for e in calls.mapper if e["kind"] == "map"]
    assert maps == [(0, False), (0, True), (2, False), (2, True), (3, False), (3, True)]
    assert slam.coarse_mapper.keyframe_list == slam.mapper.keyframe_list == [0, 2, 3]
    assert slam.coarse_mapper.keyframe_dict is not slam.mapper.keyframe_dict
    ck = P.datasets.load_checkpoint(os.path.join(slam.ckptsdir, "00003.tar"))
    assert set(ck["c"]) == {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}
    assert int(slam.mapping_cnt[0]) == 3  # (the coarse mapper does not count)


def test_run_imap(tmp_path, monkeypatch, tiny):
    """--imap: no grids, no pretrained files, three outer iterations per mapped frame."""
    over = {"scale": 1, "mapping": {"iters_first": 6, "iters": 6, "pixels": 400, "ckpt_freq": 50, "mesh_freq": 50,
                                    "vis_freq": 50, "color_refine": False},
            "tracking": {"iters": 3, "pixels": 200, "vis_freq": 50}, "meshing": {"resolution": 16},
            "pretrained_decoders": {"coarse": "nowhere/coarse.pt", "middle_fine": "nowhere/middle_fine.pt"}}
    slam, calls, want, poses = run_system(tmp_path, monkeypatch, tiny, "imap_run", 3, over, graphs=False, nice=False)
    check_schedule(calls, want)
    assert slam.shared_c == {} and not slam.nice
    maps = [e for e in calls.mapper if e["kind"] == "map"]
    assert [(e["idx"], e["num_joint_iters"]) for e in maps] == [(0, 6)] + [(1, 2)] * 3 + [(2, 2)] * 3
    est = slam.estimate_c2w_list
    assert torch.equal(est[0], poses[0])
    for i in (1, 2):
        assert torch.equal(est[i], calls.track_ret[i].cpu()), i
    ck = P.datasets.load_checkpoint(os.path.join(slam.ckptsdir, "00002.tar"))
    assert ck["c"] == {} and ck["keyframe_list"] == [0, 1, 2]
