"""Tracker drop-in: camera optimisation on the HIP render path (src/Tracker.py).

`optimize_cam_in_batch` keeps the reference's signature and semantics (Tracker.py:71-128).
The frame loop's per-frame logic (Tracker.py:184-256) is `track_frame`; `track` is one pass of
Tracker.run's loop body around it (the pose lists, the strict-sync re-read of the previous pose, the
visualiser calls), which NICE_SLAM.run schedules serially (nice_slam.py).

tracking.seperate_LR (the TUM-RGBD configs; Tracker.py:202-209) takes the same fused paths as a single rate:
the reference's two Adam groups (translation lr, quaternion lr·0.2) are one elementwise Adam over the 7-vector
with a per-element rate, and its candidate is the camera before the iteration's step (it rebuilds
camera_tensor from the two leaves at the top of every iteration, Tracker.py:226-227) — both are arguments of
the fused camera tail (nslam_cam_grad_step_lr2).  So a fused seperate_LR tracker without a generator draws
its pixels in the gather kernel, as every other fused tracker does; `fused = False` keeps the autograd loop.
"""
from __future__ import annotations

import collections
import copy

import numpy as np
import torch

from . import common as _common
from . import ops
from .common import (camera_tensors, constant_speed_guess, get_camera_from_tensor, get_samples,
                     get_tensor_from_camera, inside_mask, pose4)

# A frame's captured camera loop: the key of its graph (ops.GraphCache) and every host value its body reads.
# cam_lr / lr_quat: the Adam rates (lr_quat None without seperate_LR); seed: the device draws' stream.
FramePlan = collections.namedtuple("FramePlan", "kind iters n speed seperate_LR cam_lr lr_quat seed")


class Tracker(object):
    def __init__(self, cfg, args, slam, generator=None):
        self.cfg = cfg
        self.args = args
        self.scale = cfg.get("scale", 1)
        self.coarse = cfg["coarse"]
        self.occupancy = cfg["occupancy"]
        self.nice = slam.nice
        self.bound = slam.bound
        self.renderer = slam.renderer
        self.shared_c = slam.shared_c
        self.shared_decoders = slam.shared_decoders
        self.estimate_c2w_list = slam.estimate_c2w_list
        self.gt_c2w_list = slam.gt_c2w_list
        self.mapping_idx = slam.mapping_idx
        t = cfg["tracking"]
        self.cam_lr = t["lr"]
        self.device = t["device"]
        self.num_cam_iters = t["iters"]
        self.gt_camera = t["gt_camera"]
        self.tracking_pixels = t["pixels"]
        self.seperate_LR = t["seperate_LR"]
        self.w_color_loss = t["w_color_loss"]
        self.ignore_edge_W = t["ignore_edge_W"]
        self.ignore_edge_H = t["ignore_edge_H"]
        self.handle_dynamic = t["handle_dynamic"]
        self.use_color_in_tracking = t["use_color_in_tracking"]
        self.const_speed_assumption = t["const_speed_assumption"]
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.prev_mapping_idx = -1
        self.generator = generator  # pixel-selection RNG (None = torch's global device generator)
        self.c = {}
        self.decoders = None
        self._bound_dev = None
        self.fused = True     # track_frame on engine.TrackingEngine (no host sync per iteration)
        self.graphs = True    # fused, no generator: a frame's camera loop is one cached hipGraph (device draws)
        self._engine = None
        self._fstate = None   # persistent buffers of the captured camera loop
        self._graphs = ops.GraphCache()  # FramePlan -> the frame's graph
        self._draw_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if not self.nice:  # iMAP*: the autograd camera loop (the fused engine evaluates the NICE decoders)
            self.fused = False

    def _inside_mask(self, rays_o, rays_d, gt_depth):
        """Tracker.py:95-100: keep rays whose AABB exit distance >= gt depth."""
        if self._bound_dev is None or self._bound_dev.device != rays_o.device:
            self._bound_dev = self.bound.to(rays_o.device)
        return inside_mask(rays_o, rays_d, gt_depth, self._bound_dev)

    def optimize_cam_in_batch(self, camera_tensor, gt_color, gt_depth, batch_size, optimizer):
        """One camera iteration: sample pixels, render, uncertainty-weighted L1, backward, step."""
        device = self.device
        H, W, fx, fy, cx, cy = self.H, self.W, self.fx, self.fy, self.cx, self.cy
        optimizer.zero_grad()
        c2w = get_camera_from_tensor(camera_tensor)
        Wedge, Hedge = self.ignore_edge_W, self.ignore_edge_H
        rays_o, rays_d, b_depth, b_color = get_samples(Hedge, H - Hedge, Wedge, W - Wedge, batch_size, H, W, fx, fy,
                                                       cx, cy, c2w, gt_depth, gt_color, device,
                                                       generator=self.generator)
        if self.nice:
            keep = self._inside_mask(rays_o, rays_d, b_depth)
            rays_d, rays_o, b_depth, b_color = rays_d[keep], rays_o[keep], b_depth[keep], b_color[keep]
        depth, uncertainty, color = self.renderer.render_batch_ray(self.c, self.decoders, rays_d, rays_o, device,
                                                                   stage="color", gt_depth=b_depth)
        uncertainty = uncertainty.detach()
        resid = torch.abs(b_depth - depth) / torch.sqrt(uncertainty + 1e-10)
        if self.handle_dynamic:
            mask = (resid < 10 * resid.median()) & (b_depth > 0)
        else:
            mask = b_depth > 0
        loss = resid[mask].sum()
        if self.use_color_in_tracking:
            loss = loss + self.w_color_loss * torch.abs(b_color - color)[mask].sum()
        loss.backward()
        optimizer.step()
        optimizer.zero_grad()
        return loss.item()

    def update_para_from_mapping(self):
        """Tracker.py:130-142: snapshot the mapper's decoders and grids (no gradients needed).  The first
        snapshot is a deep copy; later ones are copied into it in place, so the tracking engine (and the
        hipGraphs captured over it) stay bound to the same buffers."""
        if self.mapping_idx[0] != self.prev_mapping_idx:
            same = (self.decoders is not None and set(self.c) == set(self.shared_c)
                    and all(self.c[k].shape == v.shape and self.c[k].stride() == v.stride()
                            for k, v in self.shared_c.items()))
            if same:
                with torch.no_grad():
                    for a, b in zip(self.decoders.parameters(), self.shared_decoders.parameters()):
                        a.copy_(b)
                    for key, val in self.shared_c.items():
                        self.c[key].copy_(val)
                if self._engine is not None:
                    for d in self._engine.eng.decs.values():  # the MFMA-packed copies of the new weights
                        d.repack()
            else:
                self.decoders = copy.deepcopy(self.shared_decoders).to(self.device)
                # tracking optimises the camera only: decoder/grid gradients are never used
                self.decoders.requires_grad_(False)
                for key, val in self.shared_c.items():
                    self.c[key] = val.detach().clone().to(self.device)
                self._engine = None  # re-bound to the new snapshot on first use
                self._fstate = None
                self._graphs.drop()  # (captured over the old snapshot's engine and buffers)
            self.prev_mapping_idx = self.mapping_idx[0].clone()

    def engine(self):
        """TrackingEngine over the current decoder/grid snapshot."""
        if self._engine is None:
            from .engine import TrackingEngine
            r = self.renderer
            c = {k: ops.channels_last(v) for k, v in self.c.items() if k != "grid_coarse"}
            self._engine = TrackingEngine(self.decoders, c, self.bound, r.N_samples, r.N_surface, (self.H, self.W),
                                          (self.fx, self.fy, self.cx, self.cy),
                                          ignore_edge=(self.ignore_edge_H, self.ignore_edge_W),
                                          w_color=self.w_color_loss, handle_dynamic=self.handle_dynamic,
                                          use_color=self.use_color_in_tracking, device=self.device)
        return self._engine

    def track_frame(self, idx, gt_color, gt_depth, gt_c2w, pre_c2w=None, prev2_c2w=None):
        """Per-frame camera estimate (Tracker.py:184-256, without sync/visualisation) → c2w [4,4]."""
        device = self.device
        self.update_para_from_mapping()
        gt_depth, gt_color = gt_depth.to(device), gt_color.to(device)
        if idx == 0 or self.gt_camera:
            return gt_c2w.clone()
        if self.fused and _common.replays_graphs(self):
            return self._track_graph(gt_color, gt_depth, pre_c2w,
                                     prev2_c2w if self.const_speed_assumption else None)
        if self.const_speed_assumption and prev2_c2w is not None:
            est = constant_speed_guess(pre_c2w.float().to(device), prev2_c2w.to(device).float())
        else:
            est = pre_c2w.to(device)
        # (on the device: no host round trip per frame)
        camera_tensor = camera_tensors(est.detach().float()[None])[0] if self.fused else \
            get_tensor_from_camera(est.detach()).to(device)
        if self.fused:  # (seperate_LR too: two rates on the fused camera tail)
            return self._track_fused(camera_tensor, gt_color, gt_depth)
        if self.seperate_LR:
            T = camera_tensor[-3:].clone().requires_grad_(True)
            quad = camera_tensor[:4].clone().requires_grad_(True)
            optimizer = torch.optim.Adam([{"params": [T], "lr": self.cam_lr},
                                          {"params": [quad], "lr": self.cam_lr * 0.2}])
        else:
            camera_tensor = camera_tensor.clone().requires_grad_(True)
            optimizer = torch.optim.Adam([camera_tensor], lr=self.cam_lr)
        best, best_loss = None, np.inf
        for cam_iter in range(self.num_cam_iters):
            if self.seperate_LR:
                camera_tensor = torch.cat([quad, T], 0)
            if self._iter_hook is not None:
                self._iter_hook(cam_iter, camera_tensor)
            loss =self.optimize_cam_in_batch(camera_tensor, gt_color, gt_depth, self.tracking_pixels, optimizer)
            if loss < best_loss:
                best_loss, best = loss, camera_tensor.clone().detach()
        return pose4(get_camera_from_tensor(best))

    # -- the frame loop (Tracker.run, Tracker.py:144-258) ------------------------------------------
    def attach_run(self, slam):
        """What Tracker.__init__ (Tracker.py:19-69) takes from `slam` and cfg for the frame loop, and the
        tracking visualiser.  NICE_SLAM calls it once; track_frame alone does not need it."""
        import os

        from .visualizer import Visualizer
        cfg = self.cfg
        self.idx = slam.idx
        self.output = slam.output
        self.verbose = slam.verbose
        self.low_gpu_mem = slam.low_gpu_mem
        self.mapping_cnt = slam.mapping_cnt
        self.sync_method = cfg["sync_method"]
        self.every_frame = cfg["mapping"]["every_frame"]
        self.no_vis_on_first_frame = cfg["mapping"]["no_vis_on_first_frame"]
        self.n_img = slam.n_img
        self.pose_work, self.gt_pose_work = slam.pose_work, slam.gt_pose_work
        self.visualizer = Visualizer(freq=cfg["tracking"]["vis_freq"], inside_freq=cfg["tracking"]["vis_inside_freq"],
                                     vis_dir=os.path.join(self.output, "vis" if "Demo" in self.output else "tracking_vis"),
                                     renderer=self.renderer, verbose=self.verbose, device=self.device)
        self._pre_c2w = None

    def track(self, idx, frame):
        """One pass of Tracker.run's loop body (Tracker.py:152-258) for frame = (idx, color, depth, c2w) → c2w.

        The pose lists are read and written through their working copies (NICE_SLAM.pose_work: on the tracking
        device, so a tracked frame costs no host synchronisation; the CPU lists themselves when the device is
        the CPU).  On a frame whose visualisation fires the camera loop runs eagerly with the visualiser called
        before every iteration, as Tracker.py:228-229 has it; every other frame replays the cached graph."""
        idx = int(idx)
        device = self.device
        _, gt_color, gt_depth, gt_c2w = frame
        est = self.pose_work
        # strict sync: the pose the mapper may have moved by BA is read again (Tracker.py:164-168); between
        # those frames pre_c2w is the tracker's own last result (Tracker.py:254)
        if idx > 0 and (idx % self.every_frame == 1 or self.every_frame == 1):
            self._pre_c2w = est[idx - 1].to(device).clone()
        if self.verbose:
            print("Tracking Frame ", idx)
        if idx == 0 or self.gt_camera:
            self.update_para_from_mapping()
            c2w = gt_c2w
            if not self.no_vis_on_first_frame:
                self.visualizer.vis(idx, 0, gt_depth, gt_color, c2w, self.c, self.decoders)
        else:
            prev2 = est[idx - 2].to(device) if (self.const_speed_assumption and idx - 2 >= 0) else None
            vis = self.visualizer
            if idx % vis.freq == 0:  # (the visualiser's own idx condition: it fires on some iteration)
                self._iter_hook = lambda it, cam: vis.vis(idx, it, gt_depth, gt_color, cam, self.c, self.decoders)
            try:
                c2w = self.track_frame(idx, gt_color, gt_depth, gt_c2w, pre_c2w=self._pre_c2w, prev2_c2w=prev2)
            finally:
                self._iter_hook = None
        est[idx] = c2w.clone()
        self.gt_pose_work[idx] = gt_c2w.clone()
        self._pre_c2w = c2w.clone()
        self.idx[0] = idx
        if self.low_gpu_mem:
            torch.cuda.empty_cache()
        return c2w

    _iter_hook = None  # track(): called as hook(cam_iter, camera_tensor) before each camera iteration

    def _frame_plan(self, speed=False):
        """This frame's camera loop as a FramePlan: the key of its graph and all its body reads."""
        lr = float(self.cam_lr)
        return FramePlan("frame", int(self.num_cam_iters), int(self.tracking_pixels), bool(speed),
                         bool(self.seperate_LR), lr, lr * 0.2 if self.seperate_LR else None, int(self._draw_seed))

    @staticmethod
    def _lr2(plan, zero=False):
        """iteration()'s keywords for tracking.seperate_LR (Tracker.py:202-209, 226-227): the quaternion's
        Adam group steps with lr·0.2, and the candidate kept is the camera before the step."""
        return {"lr_quat": 0.0 if zero else plan.lr_quat, "best_before_step": True} if plan.seperate_LR else {}

    def _track_fused(self, camera_tensor, gt_color, gt_depth):
        """The camera loop of track_frame (Tracker.py:225-250) on the TrackingEngine, eagerly: the best pose
        (lowest pre-step loss → the pose right after that step, as the reference keeps it; with
        seperate_LR the pose before it, as the reference keeps it there) is selected on the device; no
        host sync.  Pixels by torch.randint per iteration (a generator pins them).  It walks the same
        FramePlan as the captured loop (_track_graph)."""
        eng = self.engine()
        device = self.device
        plan = self._frame_plan()
        cam = camera_tensor.detach().clone().requires_grad_(True)
        opt = ops.FusedAdam([{"params": [cam], "lr": plan.cam_lr}])
        best = cam.detach().clone()
        best_loss = torch.full((), float("inf"), dtype=torch.float64, device=device)
        depth = gt_depth.float().contiguous()
        color = gt_color.float().contiguous()
        for cam_iter in range(plan.iters):
            if self._iter_hook is not None:
                self._iter_hook(cam_iter, cam.detach())
            pix = torch.randint(eng.n_window(), (plan.n,), device=device, generator=self.generator)
            eng.iteration(cam, depth, color, pix, opt, best=(best_loss, best), **self._lr2(plan))  # (+ Tracker.py:245-247)
        return pose4(get_camera_from_tensor(best))

    def _frame_state(self):
        """Persistent buffers of the captured camera loop (its graphs hold them by address)."""
        if self._fstate is None:
            dev = self.device
            cam = torch.zeros(7, dtype=torch.float32, device=dev).requires_grad_(True)
            self._fstate = {
                "depth": torch.zeros(self.H, self.W, dtype=torch.float32, device=dev),
                "color": torch.zeros(self.H, self.W, 3, dtype=torch.float32, device=dev),
                "pre": torch.eye(4, dtype=torch.float32, device=dev), "prev2": torch.eye(4, dtype=torch.float32, device=dev),
                "cam": cam, "opt": ops.FusedAdam([{"params": [cam], "lr": 0.0}]),
                "best": torch.zeros(7, dtype=torch.float32, device=dev),
                "best_loss": torch.zeros((), dtype=torch.float64, device=dev),
                "out": torch.eye(4, dtype=torch.float32, device=dev)}
            self._fstate["opt"].init_state()
        return self._fstate

    @staticmethod
    def _frame(plan, eng, st, zero_lr=False):
        """A frame's work on the buffers st, as `plan` has it (every host value of the loop comes from the plan):
        the pose guess, its 7-vector, a fresh Adam, the camera loop, the result pose.  zero_lr: the capture's
        warm-up, one iteration with every rate zero."""
        cam, opt, best, best_loss = st["cam"], st["opt"], st["best"], st["best_loss"]
        pre = st["pre"]
        est = constant_speed_guess(pre, st["prev2"]) if plan.speed else pre
        # the guess's 7-vector into the camera and the best pose in one launch (ABI v22)
        ops.cam_vector_batch(est[None], cam.detach().view(1, 7), best.view(1, 7))
        best_loss.fill_(float("inf"))
        opt.reset_state()
        opt.param_groups[0]["lr"] = 0.0 if zero_lr else plan.cam_lr
        for _ in range(1 if zero_lr else plan.iters):
            # (the iteration's loss launch also keeps the best pose, Tracker.py:245-247)
            eng.iteration(cam, st["depth"], st["color"], None, opt, n=plan.n, seed=plan.seed,
                          best=(best_loss, best), **Tracker._lr2(plan, zero=zero_lr))
        ops.cam_pose(best, st["out"][:3])  # get_camera_from_tensor(best), one launch

    def _track_graph(self, gt_color, gt_depth, pre_c2w, prev2_c2w):
        """track_frame's whole per-frame work as ONE captured hipGraph, replayed for every frame: the pose
        guess (constant speed, Tracker.py:191-198), its camera 7-vector, a fresh Adam, the camera loop with
        device pixel draws and the device-side best-pose selection (Tracker.py:225-250), and the result pose.
        Per frame the host copies the frame and the previous poses into persistent buffers and replays the
        graph of the frame's FramePlan (ops.GraphCache: the capture sequence and what a key must hold)."""
        eng = self.engine()
        st = self._frame_state()
        st["depth"].copy_(gt_depth)
        st["color"].copy_(gt_color)
        st["pre"][:3].copy_(pre_c2w[:3])  # (the bottom row stays [0, 0, 0, 1])
        if prev2_c2w is not None:
            st["prev2"][:3].copy_(prev2_c2w[:3])
        plan = self._frame_plan(speed=prev2_c2w is not None)
        draws = eng.eng.draws(plan.seed)

        def body():
            self._frame(plan, eng, st)
            return draws  # (kept with the graph that advances it: ops.GraphCache)

        g, _, _ = self._graphs.graph(plan, body, warm=lambda: self._frame(plan, eng, st, zero_lr=True),
                                     rewind=[draws.counter])
        g.replay()
        return st["out"].clone()
