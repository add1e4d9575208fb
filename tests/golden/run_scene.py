"""The frame-loop scene shared by tests/golden/make_golden_run.py (which runs the reference's Tracker.run and
Mapper.run over it and records what they do) and tests/test_run_cpu.py / tests/test_gpu_run.py (which run
NICE_SLAM.run() over it and compare): small CPU frames, and the recorders that stand in for the five entry
points below the frame loops — Tracker.optimize_cam_in_batch, Mapper.optimize_map, Mesher.get_mesh, Logger.log
and Visualizer.vis.  The recorders read only what both implementations share (the reference's argument lists
and attribute names), so the same code records either.

Two event streams are kept, the tracker's and the mapper's.  Under strict sync the reference's mapper publishes
mapping_idx before its mesh events (Mapper.py:633-640), so those run beside the tracker's next frame: the order
BETWEEN the streams there is a matter of process timing, the order within each is not.
"""
from __future__ import annotations

import os

import numpy as np
import torch

import scenes

CONFIGS = {"A": "run_a.yaml", "B": "run_b.yaml", "C": "run_c.yaml"}
N_IMG = {"A": 14, "B": 8, "C": 13}
CAM = dict(H=6, W=8, fx=4.0, fy=4.0, cx=3.5, cy=2.5)
BA_OFFSET = (0.03, -0.02, 0.01)      # what the optimize_map recorder moves cur_c2w by under BA
TRACK_OFFSET = (0.004, 0.002, -0.003)  # what the camera recorder moves the guess by (its first iteration)


def flat(t):
    return [float(v) for v in torch.as_tensor(t).detach().cpu().double().reshape(-1)]


def frames(n):
    """n frames (idx, color f64 [H,W,3], depth f32 [H,W], c2w f32 [4,4]) on the CPU: a camera swinging through
    the tiny bound.  depth is (idx + 1) everywhere, which is how the camera recorder knows the frame."""
    b = scenes.enlarge_bound(scenes.TINY_BOUND, 0.32)
    ctr = b.mean(1)
    out = []
    for i in range(n):
        c2w = scenes.look_pose(ctr, 0.3 + 0.07 * i, 0.25 + 0.03 * ((i % 4) - 1.5), (0.02 * i, -0.015 * i, 0.01 * (i % 3)))
        c2w = torch.from_numpy(np.asarray(c2w)).float()
        if c2w.shape[0] == 3:
            c2w = torch.cat([c2w, torch.tensor([[0, 0, 0, 1.0]])], 0)
        color = torch.from_numpy(scenes.color_image(CAM, seed=500 + i)).double()
        depth = torch.full((CAM["H"], CAM["W"]), float(i + 1), dtype=torch.float32)
        out.append((i, color, depth, c2w))
    return out


def write_pretrained(folder, sd, seed=3):
    """ConvONet-layout checkpoints synthesised from a NICE state dict (the tiny scene's): coarse.pt holds
    'decoder.*', middle_fine.pt holds 'decoder_coarse.*' (the middle decoder) and 'decoder_fine.*', each beside
    encoder keys that a loader must ignore (NICE_SLAM.py:159-190).  → the two paths."""
    g = torch.Generator().manual_seed(seed)
    junk = lambda: torch.randn(4, 4, generator=g)  # noqa: E731
    coarse = {"encoder.conv_in.weight": junk(), "encoder.decoder_like.weight": junk()}
    coarse.update({"decoder." + k[len("coarse_decoder."):]: v.clone() for k, v in sd.items()
                   if k.startswith("coarse_decoder.")})
    mf = {"encoder_coarse.fc_pos.weight": junk(), "encoder_fine.unet3d.decoders.0.weight": junk()}
    mf.update({"decoder_coarse." + k[len("middle_decoder."):]: v.clone() for k, v in sd.items()
               if k.startswith("middle_decoder.")})
    mf.update({"decoder_fine." + k[len("fine_decoder."):]: v.clone() for k, v in sd.items()
               if k.startswith("fine_decoder.")})
    paths = os.path.join(folder, "coarse.pt"), os.path.join(folder, "middle_fine.pt")
    torch.save({"model": coarse, "epoch_it": 3}, paths[0])
    torch.save({"model": mf, "epoch_it": 5}, paths[1])
    return paths


class Frames(torch.utils.data.Dataset):
    """The frames as a dataset: what get_dataset returns in the harness (indexable by an int or a 0-d tensor),
    with datasets.BaseDataset's prefetch()."""

    def __init__(self, n):
        self.items = frames(n)
        self.n_img = n

    def __len__(self):
        return self.n_img

    def __getitem__(self, i):
        idx, color, depth, c2w = self.items[int(i)]
        return idx, color.clone(), depth.clone(), c2w.clone()

    def prefetch(self, indices=None):
        for i in (range(self.n_img) if indices is None else indices):
            yield self[i]


class Recorder:
    """Stand-ins for the five entry points; `tracker` and `mapper` are the recorded event streams."""

    def __init__(self):
        self.tracker, self.mapper = [], []
        self._opt = None

    # -- Tracker.optimize_cam_in_batch(camera_tensor, gt_color, gt_depth, batch_size, optimizer) ------------
    def optimize_cam_in_batch(rec, self, camera_tensor, gt_color, gt_depth, batch_size, optimizer):
        if optimizer is not rec._opt:  # a frame's first iteration: the initial camera tensor, then one "step"
            rec._opt = optimizer
            rec._cur = {"kind": "track", "idx": int(gt_depth.reshape(-1)[0]) - 1, "cam0": flat(camera_tensor),
                        "pixels": int(batch_size), "iters": 0}
            rec.tracker.append(rec._cur)
            with torch.no_grad():
                camera_tensor[-3:] += torch.tensor(TRACK_OFFSET, dtype=camera_tensor.dtype,
                                                   device=camera_tensor.device)
        rec._cur["iters"] += 1
        return 1.0  # (a constant loss: the first iteration's camera is the candidate kept)

    # -- Mapper.optimize_map(...) ----------------------------------------------------------------------------
    def optimize_map(rec, self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w, keyframe_dict,
                     keyframe_list, cur_c2w):
        rec.mapper.append({"kind": "map", "coarse": bool(self.coarse_mapper), "idx": int(idx),
                           "num_joint_iters": int(num_joint_iters), "lr_factor": float(lr_factor), "BA": bool(self.BA),
                           "window": int(self.mapping_window_size), "middle_iter_ratio": float(self.middle_iter_ratio),
                           "fine_iter_ratio": float(self.fine_iter_ratio), "fix_color": bool(self.fix_color),
                           "frustum": bool(self.frustum_feature_selection), "n_kf": len(keyframe_list),
                           "cur_c2w": flat(cur_c2w)})
        if not self.BA:
            return None
        out = cur_c2w.clone()
        out[:3, 3] += torch.tensor(BA_OFFSET, dtype=out.dtype, device=out.device)
        return out

    # -- Mesher.get_mesh(...) ----------------------------------------------------------------------------------
    def get_mesh(rec, self, mesh_out_file, c, decoders, keyframe_dict, estimate_c2w_list, idx, device="cuda:0",
                 show_forecast=False, color=True, clean_mesh=True, get_mask_use_all_frames=False):
        idx = int(idx)
        rec.mapper.append({"kind": "mesh", "file": os.path.basename(mesh_out_file), "idx": idx,
                           "show_forecast": bool(show_forecast), "clean_mesh": bool(clean_mesh),
                           "all_frames": bool(get_mask_use_all_frames), "n_kf": len(keyframe_dict),
                           "est": flat(estimate_c2w_list[:idx + 1])})
        with open(mesh_out_file, "wb"):  # (the loop copies final_mesh.ply afterwards)
            pass

    # -- Logger.log(idx, keyframe_dict, keyframe_list, selected_keyframes=None) -----------------------------
    def log(rec, self, idx, keyframe_dict, keyframe_list, selected_keyframes=None):
        idx = int(idx)
        rec.mapper.append({"kind": "ckpt", "idx": idx, "keyframe_list": [int(k) for k in keyframe_list],
                           "selected": selected_keyframes is not None, "est": flat(self.estimate_c2w_list[:idx + 1])})

    # -- Visualizer.vis(idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders) -------------------
    def vis(rec, self, idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders):
        if int(idx) % self.freq == 0 and int(iter) % self.inside_freq == 0:  # (the calls that would write a file)
            where = os.path.basename(os.path.normpath(self.vis_dir))
            stream = rec.mapper if where == "mapping_vis" else rec.tracker
            stream.append({"kind": "vis", "dir": where, "idx": int(idx), "iter": int(iter),
                           "pose": flat(c2w_or_camera_tensor)})

    def bind(rec, name):
        fn = getattr(Recorder, name)
        return lambda self, *a, **k: fn(rec, self, *a, **k)

    def final(rec, estimate_c2w_list, gt_c2w_list, mapper, counters):
        return {"estimate_c2w_list": flat(estimate_c2w_list), "gt_c2w_list": flat(gt_c2w_list),
                "keyframe_list": [int(k) for k in mapper.keyframe_list],
                "keyframe_est_c2w": [flat(kf["est_c2w"]) for kf in mapper.keyframe_dict],
                "keyframe_idx": [int(kf["idx"]) for kf in mapper.keyframe_dict],
                **{k: int(v[0]) for k, v in counters.items()}}
