"""Mapper drop-in: map optimisation on the HIP render path (src/Mapper.py).

`optimize_map` keeps the reference's signature and semantics (Mapper.py:230-540): staged
middle → fine → colour schedule, Adam re-created per call, frustum-masked grid parameters,
optional bundle adjustment of keyframe cameras.  It runs on the fused mapping engine
(engine.MappingEngine: one gather / sampler / forward / loss / backward / Adam chain of HIP launches
per iteration, no autograd) — `Mapper.fused = False` selects the autograd drop-in of the same loop.
Differences from the reference (none changes the maths):
  * keyframe images stay resident on the device (the reference copies them host→device every
    iteration, Mapper.py:439-440);
  * the frustum voxel mask (Mapper.py:93-164) is computed with torch on the device; cv2.remap's
    bilinear lookup is emulated including its 1/32-pixel fixed-point positions and zero border
    (OpenCV is not installed: parity with cv2 itself is unpinned);
  * the masked grid vectors are not copied in and out of the grids every iteration
    (Mapper.py:394-401, 511-519): Adam updates the selected voxels in place, with state for them
    alone — the same elementwise update; the optimiser's state is reset per call (a fresh Adam);
  * the inside-mask prefilter (Mapper.py:469-481) gives dropped rays zero loss weight instead of
    compacting them (their gradients are exactly zero; the sampler's batch max sees kept rays only);
  * pixel draws: through common.select_uv (torch.randint, eager) when it is replaced (tests pin the
    draws that way) or a generator is given; otherwise drawn inside the gather kernel (uniform over
    the image like select_uv, a counter-based stream instead of torch's Philox) so that each stage's
    iterations are captured ONCE in a hipGraph and replayed by every later call with the same plan
    (StagePlan below: the graph's key holds every host value it baked in; ops.GraphCache; the window's
    frames are copied into persistent slots, the frustum selection is bound on the device with
    capacity-sized buffers: engine.MappingEngine.bind_masks).
One pass of the mapping loop driver (Mapper.run, Mapper.py:572-654) is `map_frame`; NICE_SLAM.run schedules it
serially (nice_slam.py).
"""
from __future__ import annotations

import collections
import functools
import os
import time

import numpy as np
import torch

from . import common as _common
from . import ops
from .common import (get_camera_from_tensor, get_samples, get_tensor_from_camera, inside_mask, pose4,
                     random_select)

_STAGE_GROUPS = ("decoders", "coarse", "middle", "fine", "color")

# The plans of a fused call: each is the key of a cached graph (ops.GraphCache) and holds every host value the
# captured body reads; the eager path walks the same records.
# StagePlan: `iters` iterations of one stage over a window of F frames × n_per pixels whose slots c0.. hold the
# ncam BA cameras.  lrs: the effective rates of _STAGE_GROUPS (cfg × lr_factor); cam_lr: the cameras' (0 before
# the colour stage and without BA); trainable: the decoders in the optimiser; record: losses are kept; first:
# the run also sets the BA cameras up; prefetch: the next batch is drawn beside this iteration;
# intrinsics = (fx, fy, cx, cy); seed: the device draws' stream.
StagePlan = collections.namedtuple("StagePlan", "kind stage iters F n_per c0 ncam lrs cam_lr trainable record first "
                                                "prefetch H W intrinsics seed")
# SetupPlan: the per-call setup over n_kf scored keyframes; frustum / coarse / hooked (get_mask_from_c2w is
# replaced on the instance) steer how the frustum selection is bound (_bind_frustum); trainable names the
# optimiser whose state the setup zeroes.
SetupPlan = collections.namedtuple("SetupPlan", "kind n_kf frustum coarse hooked trainable H W intrinsics")


def _remap_bilinear(img, u, v):
    """cv2.remap(img, u, v, INTER_LINEAR, BORDER_CONSTANT=0) for float32 maps (INTER_BITS=5)."""
    H, W = img.shape
    X = torch.round(u.clamp(-1e8, 1e8) * 32).to(torch.int64)
    Y = torch.round(v.clamp(-1e8, 1e8) * 32).to(torch.int64)
    x0, y0 = torch.div(X, 32, rounding_mode="floor"), torch.div(Y, 32, rounding_mode="floor")
    fx = (X - x0 * 32).to(torch.float32) / 32
    fy = (Y - y0 * 32).to(torch.float32) / 32

    def tap(x, y):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return torch.where(ok, img[y.clamp(0, H - 1), x.clamp(0, W - 1)], torch.zeros((), device=img.device))

    w00, w01 = (1 - fx) * (1 - fy), fx * (1 - fy)
    w10, w11 = (1 - fx) * fy, fx * fy
    return tap(x0, y0) * w00 + tap(x0 + 1, y0) * w01 + tap(x0, y0 + 1) * w10 + tap(x0 + 1, y0 + 1) * w11


_KMAT = {}


def _intrinsics(fx, fy, cx, cy, dev):
    """The camera matrix as a float64 device tensor, made once per (intrinsics, device): a hipGraph
    capturing its users must not copy it from the host."""
    key = (float(fx), float(fy), float(cx), float(cy), str(dev))
    if key not in _KMAT:
        _KMAT[key] = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64, device=dev)
    return _KMAT[key]


_POINTS = {}


def _grid_points(bound, val_shape, dev):
    """The grid's voxel positions in get_mask_from_c2w's meshgrid order [X*Y*Z, 3] (cached per shape)."""
    b = bound
    key = (tuple(float(v) for v in torch.as_tensor(b).reshape(-1)), tuple(int(v) for v in val_shape), str(dev))
    if key not in _POINTS:
        nz, ny, nx = (int(v) for v in val_shape)
        X, Y, Z = torch.meshgrid(torch.linspace(float(b[0][0]), float(b[0][1]), nx, device=dev),
                                 torch.linspace(float(b[1][0]), float(b[1][1]), ny, device=dev),
                                 torch.linspace(float(b[2][0]), float(b[2][1]), nz, device=dev), indexing="ij")
        _POINTS[key] = torch.stack([X, Y, Z], dim=-1).reshape(-1, 3)
    return _POINTS[key]


def _world_to_uvz(points, c2w, K):
    """World points [N,3] in the pixel frame of the camera c2w ([3,4] or [4,4]) with intrinsics K, as the
    reference projects them (Mapper.py:131-141, 196-207): float64 [N,3] = (u·z, v·z, z) with x flipped."""
    w2c = torch.linalg.inv_ex(pose4(c2w.to(points.device).float()))[0]  # (no error check: no host sync, capturable)
    cam = (points @ w2c[:3, :3].T + w2c[:3, 3]).double()
    cam[:, 0] *= -1
    return cam @ K.T


def frustum_rows_device(c2w, val_shape, depth, bound, H, W, fx, fy, cx, cy, slot, rows, n_live, mask_ref=None):
    """frustum_mask fused with its compaction (ABI v20 nslam_frustum_rows): slot [Z*Y*X] int32, rows (>= the
    voxel count) int32 and n_live int64 [1] are written in place, as MappingEngine.bind_masks would from the
    mask.  The two projection GEMMs and the near-camera test run here with frustum_mask's own torch ops (the
    same values bit for bit); the remap, the depth tests and the compaction run in one kernel sequence.
    mask_ref: optional uint8 [X*Y*Z] receiving the mask in frustum_mask's order."""
    from ._lib import check, lib, ptr, stream_ptr
    dev = depth.device
    nz, ny, nx = (int(v) for v in val_shape)
    n = nx * ny * nz
    for name, t in (("slot", slot), ("rows", rows)):  # (the kernels write n entries of each)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"frustum_rows_device: {name} must be contiguous int32 with at least {n} entries, got "
                             f"{t.dtype} {tuple(t.shape)}")
    if n_live.dtype != torch.int64 or tuple(n_live.shape) != (1,):
        raise ValueError(f"frustum_rows_device: n_live must be int64 [1], got {n_live.dtype} {tuple(n_live.shape)}")
    points = _grid_points(bound, val_shape, dev)
    c2w = c2w.to(dev).float()
    uvz = _world_to_uvz(points, c2w, _intrinsics(fx, fy, cx, cy, dev))
    d = points - c2w[:3, 3]
    near = ((d * d).sum(1) < 0.5 * 0.5).to(torch.uint8)
    wsb = lib().nslam_frustum_rows_workspace_size(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dep = depth.float().contiguous()
    rc = lib().nslam_frustum_rows(ptr(uvz.contiguous()), ptr(near), ptr(dep), H, W, nx, ny, nz, ptr(slot), ptr(rows),
                                  ptr(n_live), ptr(mask_ref), ptr(ws), wsb, stream_ptr(dev))
    check(rc, "nslam_frustum_rows")


def frustum_mask(c2w, key, val_shape, depth, bound, H, W, fx, fy, cx, cy):
    """Mapper.get_mask_from_c2w (Mapper.py:93-164) on the device: bool mask [X, Y, Z] of the
    grid voxels inside the camera frustum up to the observed depth + 0.5 m, or within 0.5 m of
    the camera.  val_shape = (Z, Y, X)."""
    dev = depth.device
    nz, ny, nx = val_shape[0], val_shape[1], val_shape[2]
    if key == "grid_coarse":
        return torch.ones(nx, ny, nz, dtype=torch.bool, device=dev)
    points = _grid_points(bound, val_shape, dev)
    c2w = c2w.to(dev).float()
    uvz = _world_to_uvz(points, c2w, _intrinsics(fx, fy, cx, cy, dev))
    z = uvz[:, 2] + 1e-5
    uv = (uvz[:, :2] / z[:, None]).float()
    depths = _remap_bilinear(depth.float(), uv[:, 0], uv[:, 1])
    mask = (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
    depths = torch.where(depths == 0, depths.max(), depths)
    mask = mask & (0 <= -z) & (-z <= depths.double() + 0.5)
    ray_o = c2w[:3, 3]
    d = points - ray_o
    mask = mask | ((d * d).sum(1) < 0.5 * 0.5)
    return mask.reshape(nx, ny, nz)


class _Window(object):
    """One fused optimize_map call's window: its frames copied into the mapper's persistent slots (the oldest
    frame, fixed under BA, first; then the others in optimize_frame order) and, with BA, the camera buffers.
    F frames of n_per pixels each; slots c0.. hold the ncam optimised cameras; poses [F,3,4] as copied in;
    ar: the pixel index table of eager select_uv draws (None: the gather kernel draws)."""

    def __init__(self, mapper, optimize_frame, oldest_frame, keyframe_dict, cur_gt_depth, cur_gt_color, cur_c2w,
                 device_draws):
        dev = mapper.device
        self.optimize_frame = optimize_frame
        F = self.F = len(optimize_frame)
        self.n_per = mapper.mapping_pixels // F
        fixed = mapper.BA and oldest_frame is not None
        self.order = list(optimize_frame)
        if fixed:
            self.order.remove(oldest_frame)
            self.order.insert(0, oldest_frame)
        depth_s, color_s, self.c2w_s = mapper._window_slots(F)
        poses = []
        for s, fr in enumerate(self.order):
            if fr == -1:
                d, c, m = cur_gt_depth, cur_gt_color, cur_c2w
            else:
                d, c = mapper._frame_images(keyframe_dict[fr])
                m = keyframe_dict[fr]["est_c2w"].to(dev).float()
            depth_s[s].copy_(d)
            color_s[s].copy_(c)
            poses.append(m[:3])
        self.poses = torch.stack(poses)
        self.restore_poses()
        self.frames = [(depth_s[s], color_s[s], self.c2w_s[s]) for s in range(F)]
        c0 = self.c0 = 1 if fixed else 0
        self.ncam = (F - c0) if mapper.BA else 0
        if self.ncam:  # the 7-vectors of the optimised frames (Mapper.py:349-363)
            self.cams, self.cgrad, self.cws, self.ctk, self.copt = mapper._cam_state(self.ncam)
            self.copt.init_state()
            # the optimised frames are gathered from their 7-vectors: the gather forms each pose
            # (get_camera_from_tensor) and writes it to the frame's slot for the camera gradient (ABI v21)
            self.frames[c0:] = [(depth_s[s], color_s[s], self.c2w_s[s], self.cams[s - c0]) for s in range(c0, F)]
        self.ar = None if device_draws else torch.arange(mapper.H * mapper.W, device=dev)

    def restore_poses(self):
        self.c2w_s[:self.F, :3].copy_(self.poses)

    def cams_init(self):
        """The BA cameras from the slots' poses (get_tensor_from_camera of each, one launch), a fresh Adam."""
        ops.cam_vector_batch(self.c2w_s[self.c0:self.F], self.cams)
        self.copt.reset_state()

    def post_bwd(self, gps, ro, rd, z):
        """BA: camera gradients of every optimised frame, then their Adam step."""
        c0, n_per = self.c0, self.n_per
        ops.cam_grad_batch(self.cams, self.c2w_s[c0:self.F], [(c0 + k) * n_per for k in range(self.ncam)], n_per, gps,
                           z, rd, self.cgrad, self.cws, self.ctk)
        self.copt.step(grads={self.cams: self.cgrad})

    def write_back(self, keyframe_dict, cur_c2w):
        """Mapper.py:521-540: the optimised poses into keyframe_dict; returns the current frame's."""
        out = torch.zeros(self.ncam, 4, 4, dtype=torch.float32, device=self.cams.device)
        out[:, 3, 3] = 1.0
        ops.cam_pose_batch(self.cams, out)
        for k, fr in enumerate(self.order[self.c0:]):
            if fr == -1:
                cur_c2w = out[k]
            else:
                keyframe_dict[fr]["est_c2w"] = out[k]
        return cur_c2w


class Mapper(object):
    def __init__(self, cfg, args, slam, coarse_mapper=False, generator=None):
        self.cfg = cfg
        self.args = args
        self.coarse_mapper = coarse_mapper
        self.nice = slam.nice
        self.c = slam.shared_c
        self.bound = slam.bound
        self.renderer = slam.renderer
        self.decoders = slam.shared_decoders
        self.estimate_c2w_list = slam.estimate_c2w_list
        self.coarse = cfg["coarse"]
        self.occupancy = cfg["occupancy"]
        m = cfg["mapping"]
        self.device = m["device"]
        self.fix_fine = m["fix_fine"]
        self.BA = False
        self.BA_cam_lr = m["BA_cam_lr"]
        self.fix_color = m["fix_color"]
        self.mapping_pixels = m["pixels"]
        self.num_joint_iters = m["iters"]
        self.w_color_loss = m["w_color_loss"]
        self.fine_iter_ratio = m["fine_iter_ratio"]
        self.middle_iter_ratio = m["middle_iter_ratio"]
        self.mapping_window_size = m["mapping_window_size"]
        self.frustum_feature_selection = m["frustum_feature_selection"]
        self.keyframe_selection_method = m["keyframe_selection_method"]
        if self.nice and coarse_mapper:
            self.keyframe_selection_method = "global"
        self.keyframe_dict = []
        self.keyframe_list = []
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.generator = generator
        self.stage = "middle"
        self.loss_history = None  # set to [] to record per-iteration losses (detached, no host sync)
        self.regulation_draws = None  # iMAP* test hook: n_rays -> t_rand [n_rays, N_samples] (recorded jitter)
        self.fused = True   # optimize_map on engine.MappingEngine (False: the autograd drop-in)
        self.graphs = True  # fused path with device draws: each stage's iterations as one cached hipGraph
        self._eng = None
        self._fopt = {}     # trainable decoders -> the fused path's FusedAdam
        self._cam = {}      # number of BA cameras -> (cams, grad, ws, tickets, FusedAdam)
        self._slots = None  # (depth [F,H,W], color [F,H,W,3], c2w [F,4,4]) of the window
        self._setup = None  # persistent inputs of the captured per-call setup (_setup_inputs)
        self._graphs = ops.GraphCache()  # StagePlan / SetupPlan -> (graph, what its body returned)
        # the device draws' stream key (from torch's CPU generator, so torch.manual_seed pins it)
        self._draw_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.calls = 0
        self.timing = None  # set to [] to record per-call phase times (host clock + HIP events; bench legs)

    # ------------------------------------------------------------------------------------------
    def get_mask_from_c2w(self, c2w, key, val_shape, depth):
        """Frustum voxel selection (Mapper.py:93-164) → bool mask [X, Y, Z] on the device."""
        return frustum_mask(c2w, key, val_shape, depth, self.bound, self.H, self.W, self.fx, self.fy, self.cx,
                            self.cy)

    def keyframe_overlap_scores(self, gt_color, gt_depth, c2w, keyframe_dict, N_samples=16, pixels=100):
        """Mapper.py:185-221: per keyframe, the fraction of the current frame's near-surface samples
        (100 pixels × 16 depths in [0.8·d, d + 0.5]) that project inside it (20-px margin, in front
        of the camera).  One host sync for all keyframes (the reference's loop is host numpy)."""
        counts, n = self._overlap_counts(gt_color, gt_depth, c2w, [kf["est_c2w"] for kf in keyframe_dict], N_samples,
                                         pixels)
        if counts is None:
            return []
        # mask.sum() / uv.shape[0] as the reference divides: an integer count over the sample count
        return [int(cnt) / n for cnt in counts.cpu()]

    def _overlap_counts(self, gt_color, gt_depth, c2w, poses, N_samples=16, pixels=100, camera=None):
        """The device half of keyframe_overlap_scores: (counts [len(poses)] device int64 or None, samples).
        camera = (H, W, fx, fy, cx, cy), the mapper's own by default (the captured setup passes its plan's)."""
        dev = self.device
        H, W, fx, fy, cx, cy = camera or (self.H, self.W, self.fx, self.fy, self.cx, self.cy)
        rays_o, rays_d, gd, _ = get_samples(0, H, 0, W, pixels, H, W, fx, fy, cx, cy, c2w, gt_depth, gt_color, dev,
                                            generator=self.generator)
        if not poses:
            return None, 0
        gd = gd.reshape(-1, 1).repeat(1, N_samples)
        t = torch.linspace(0.0, 1.0, N_samples, device=dev)
        z = gd * 0.8 * (1.0 - t) + (gd + 0.5) * t
        verts = (rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]).reshape(-1, 3)
        K = _intrinsics(fx, fy, cx, cy, dev)
        counts = []
        for pose in poses:
            uvz = _world_to_uvz(verts, pose, K)
            zz = uvz[:, 2] + 1e-5
            uv = (uvz[:, :2] / zz[:, None]).float()
            edge = 20
            m = (uv[:, 0] < W - edge) & (uv[:, 0] > edge) & (uv[:, 1] < H - edge) & (uv[:, 1] > edge) & (zz < 0)
            counts.append(m.sum())
        return torch.stack(counts), verts.shape[0]

    def keyframe_selection_overlap(self, gt_color, gt_depth, c2w, keyframe_dict, k, N_samples=16, pixels=100):
        """Mapper.py:166-228: keyframes whose frustum sees the current frame's surface samples,
        ranked by overlap (stable sort, as `sorted`), then a random permutation (numpy RNG) of the
        ones with any overlap, truncated to k."""
        scores = self.keyframe_overlap_scores(gt_color, gt_depth, c2w, keyframe_dict, N_samples, pixels)
        return self._rank_keyframes(scores, k)

    @staticmethod
    def _rank_keyframes(scores, k):
        """The host half of keyframe_selection_overlap (Mapper.py:222-228)."""
        ranked = sorted(enumerate(scores), key=lambda s: s[1], reverse=True)
        sel = [kid for kid, s in ranked if s > 0.0]
        return list(np.random.permutation(np.array(sel))[:k])

    # ------------------------------------------------------------------------------------------
    def _frame_images(self, kf):
        if "_dev" not in kf:  # keyframe images resident on the device (one copy per keyframe)
            kf["_dev"] = (kf["depth"].to(self.device), kf["color"].to(self.device).float())
        return kf["_dev"]

    def optimize_map(self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w, keyframe_dict,
                     keyframe_list, cur_c2w):
        """Mapping iterations (Mapper.py:230-540); returns the BA-updated cur_c2w or None."""
        self.calls += 1
        if not self.nice:  # iMAP*: the autograd loop only (no fused engine, no graph capture)
            impl = self._optimize_map_imap
        else:
            impl = self._optimize_map_fused if self.fused else self._optimize_map_autograd
        return impl(num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w, keyframe_dict,
                    keyframe_list, cur_c2w)

    # ------------------------------------------------------------------------------------------
    def _select_keyframes(self, keyframe_dict, cur_gt_color, cur_gt_depth, cur_c2w):
        """The keyframes selected for the window besides the last one (Mapper.py:256-266)."""
        if len(keyframe_dict) == 0:
            return []
        if self.keyframe_selection_method == "global":
            return random_select(len(self.keyframe_dict) - 1, self.mapping_window_size - 2)
        return self.keyframe_selection_overlap(cur_gt_color, cur_gt_depth, cur_c2w, keyframe_dict[:-1],
                                               self.mapping_window_size - 2)

    @staticmethod
    def _window_of(selected, keyframe_list):
        """optimize_frame (the selection, the last keyframe, -1 = the current frame) and the oldest keyframe
        in it (Mapper.py:268-272, 346-349)."""
        optimize_frame, oldest_frame = list(selected), None
        if len(keyframe_list) > 0:
            optimize_frame.append(len(keyframe_list) - 1)
            oldest_frame = min(optimize_frame)
        return optimize_frame + [-1], oldest_frame

    def _stage_of(self, joint_iter, num_joint_iters):
        """Mapper.py:403-411."""
        if self.coarse_mapper:
            return "coarse"
        if joint_iter <= int(num_joint_iters * self.middle_iter_ratio):
            return "middle"
        if joint_iter <= int(num_joint_iters * self.fine_iter_ratio):
            return "fine"
        return "color"

    def _stage_runs(self, num_joint_iters):
        """A call's schedule as runs of one stage: [(stage, iterations), ...] (Mapper.py:403-421)."""
        runs = []
        for it in range(num_joint_iters):
            stg = self._stage_of(it, num_joint_iters)
            if runs and runs[-1][0] == stg:
                runs[-1][1] += 1
            else:
                runs.append([stg, 1])
        return [tuple(r) for r in runs]

    def _grid_keys(self):
        return ["grid_coarse"] if self.coarse_mapper else [k for k in ("grid_middle", "grid_fine", "grid_color")
                                                          if k in self.c]

    def engine(self):
        """The persistent MappingEngine over the shared grids and decoders (built on first use)."""
        if self._eng is None:
            from .engine import MappingEngine
            c = {k: self.c[k] for k in self._grid_keys()}
            r = self.renderer
            self._eng = MappingEngine(self.decoders, c, self.bound, r.N_samples, r.N_surface, lindisp=r.lindisp,
                                      w_color=self.w_color_loss, device=self.device)
        return self._eng

    def _trainable(self):
        """Decoders in the optimiser's "decoders" group (Mapper.py:335-341)."""
        return tuple(n for n, fixed in (("fine", self.fix_fine), ("color", self.fix_color)) if not fixed)

    def _optimizer(self, eng, trainable):
        """The persistent FusedAdam of the fused path, one per set of trainable decoders (graphs hold its
        state by address, and their keys name that set): groups decoders / coarse / middle / fine / colour as
        the reference's (Mapper.py:365-389); grid groups hold the frustum rows with their live count."""
        if trainable not in self._fopt:
            dec = [eng.decs[n].param for n in trainable if n in eng.decs]
            groups = [{"params": dec, "lr": 0.0}]
            for name in _STAGE_GROUPS[1:]:
                k = "grid_" + name
                if k in eng.c:
                    rows, n_live = eng.live_rows(k)
                    groups.append({"params": [eng.c[k]], "lr": 0.0, "rows": rows, "n_live": n_live})
                else:
                    groups.append({"params": [], "lr": 0.0})
            self._fopt[trainable] = ops.FusedAdam(groups)
        return self._fopt[trainable]

    def _cam_state(self, n):
        """Persistent BA camera buffers for n cameras: cams [n,7], their gradient, the camera-gradient
        workspace / tickets, and their Adam (the reference's param group 5, Mapper.py:386-389)."""
        if n not in self._cam:
            dev = self.device
            cams = torch.zeros(n, 7, dtype=torch.float32, device=dev)
            grad = torch.zeros(n, 7, dtype=torch.float32, device=dev)
            ws = torch.zeros(n * ops.CAM_GRAD_WS_DOUBLES, dtype=torch.float64, device=dev)
            tickets = torch.zeros(n, dtype=torch.int32, device=dev)
            self._cam[n] = (cams, grad, ws, tickets, ops.FusedAdam([{"params": [cams], "lr": 0.0}]))
        return self._cam[n]

    def _window_slots(self, F):
        if self._slots is None or self._slots[0].shape[0] < F:
            dev, H, W = self.device, self.H, self.W
            n = max(F, self.mapping_window_size)
            self._slots = (torch.zeros(n, H, W, dtype=torch.float32, device=dev),
                           torch.zeros(n, H, W, 3, dtype=torch.float32, device=dev),
                           torch.eye(4, dtype=torch.float32, device=dev).repeat(n, 1, 1))
            self._graphs.drop("stage")  # the window slots regrew: the stage graphs read the old ones
        return self._slots

    def _setup_plan(self, n_kf=0):
        """This call's per-call setup as a SetupPlan (n_kf: the keyframes its overlap selection scores)."""
        return SetupPlan("setup", int(n_kf), bool(self.frustum_feature_selection), bool(self.coarse_mapper),
                         "get_mask_from_c2w" in self.__dict__, self._trainable(), int(self.H), int(self.W),
                         (float(self.fx), float(self.fy), float(self.cx), float(self.cy)))

    def _bind_frustum(self, eng, c2w, depth, plan):
        """This call's frustum selection bound into the engine's capacity buffers (Mapper.py:314-333): the
        fused kernel (nslam_frustum_rows) per grid shape, the other grids of that shape copying its rows;
        the coarse grid (an all-true mask, Mapper.py:113-115) and frustum_feature_selection=False through
        bind_masks.  get_mask_from_c2w replaced on the instance (a test hook) also goes through bind_masks.
        Which of these, and the camera, come from the SetupPlan; the grids are the engine's."""
        if not plan.frustum or plan.coarse or plan.hooked:
            eng.bind_masks(self._call_masks(eng, c2w, depth, plan))
            return
        if getattr(eng, "_cap_keys", None) != tuple(sorted(eng.c)):
            eng.bind_masks({k: None for k in eng.c})  # (first call: the capacity buffers)
        eng.rows_gen += 1  # the slot maps are rewritten in place: live-point lists formed from them are stale
        done = {}
        for k, grid in eng.c.items():
            shp = tuple(grid.shape[2:])
            rows, n_live = eng.live_rows(k)
            slot = eng.slot[k]
            if shp in done:
                s0, r0, n0 = done[shp]
                slot.copy_(s0)
                rows.copy_(r0)
                n_live.copy_(n0)
            else:
                frustum_rows_device(c2w, shp, depth, self.bound, plan.H, plan.W, *plan.intrinsics, slot, rows, n_live)
                done[shp] = (slot, rows, n_live)

    def _call_masks(self, eng, c2w, depth, plan):
        """This call's frustum masks of the engine's grids (Mapper.py:314-333; None = every voxel, all of them
        without plan.frustum): grids of one shape share one.  A hooked get_mask_from_c2w is called; otherwise
        frustum_mask with the plan's camera."""
        def mask(k, shp):
            if plan.hooked:
                return self.get_mask_from_c2w(c2w, k, shp, depth)
            return frustum_mask(c2w, k, shp, depth, self.bound, plan.H, plan.W, *plan.intrinsics)

        masks, by_shape = {}, {}
        for k, grid in eng.c.items():
            shp = tuple(grid.shape[2:])
            if not plan.frustum:
                masks[k] = None
            elif k == "grid_coarse":
                masks[k] = mask(k, shp)
            else:
                if shp not in by_shape:
                    by_shape[shp] = mask(k, shp)
                masks[k] = by_shape[shp]
        return masks

    def _setup_inputs(self, K):
        """Persistent inputs of the captured per-call setup: the current frame, its pose, the keyframe poses."""
        st = self._setup
        if st is None or st["poses"].shape[0] < K:
            dev, H, W = self.device, self.H, self.W
            st = self._setup = {"depth": torch.zeros(H, W, dtype=torch.float32, device=dev),
                                "color": torch.zeros(H, W, 3, dtype=torch.float32, device=dev),
                                "c2w": torch.eye(4, dtype=torch.float32, device=dev),
                                "poses": torch.eye(4, dtype=torch.float32, device=dev).repeat(max(8, 2 * K), 1, 1)}
            self._graphs.drop("setup")  # the setup's input buffers were (re)made: its graphs read the old ones
        return st

    # -- optimize_map on the fused engine (see the module docstring) -------------------------------
    @staticmethod
    def _mark(tm, name):
        """Host time and a HIP event on the caller's stream at a phase boundary of a timed call."""
        if tm is not None:
            tm[name] = time.perf_counter()
            tm["ev"][name] = torch.cuda.Event(enable_timing=True)
            tm["ev"][name].record()

    def _run_setup(self, plan, eng, st):
        """The captured per-call setup of `plan` over the inputs st (_setup_inputs): the frustum selection, a
        fresh Adam (its state made, then zeroed) and the overlap counts of the plan's keyframes →
        (counts or None, samples)."""
        self._bind_frustum(eng, st["c2w"], st["depth"], plan)
        opt = self._optimizer(eng, plan.trainable)
        opt.init_state()
        opt.reset_state()
        if plan.n_kf:
            return self._overlap_counts(st["color"], st["depth"], st["c2w"], [st["poses"][i] for i in range(plan.n_kf)],
                                        camera=(plan.H, plan.W) + plan.intrinsics)
        return None, 0

    def _fused_setup(self, eng, use_graphs, overlap_here, cur_gt_color, cur_gt_depth, cur_c2w, keyframe_dict):
        """What a call enqueues before its keyframe selection: the frustum selection (Mapper.py:314-333) bound
        on the device, a fresh Adam (Mapper.py:365-389: zero moments and step counts) and, when overlap_here,
        the overlap counts of keyframe_dict[:-1] — with graphs as one captured graph per SetupPlan over
        persistent inputs.  Returns (optimiser, counts, samples)."""
        kfs = keyframe_dict[:-1] if overlap_here else []  # (overlap_here: only with graphs)
        plan = self._setup_plan(len(kfs))
        if not use_graphs:
            self._bind_frustum(eng, cur_c2w, cur_gt_depth, plan)
            opt = self._optimizer(eng, plan.trainable)
            opt.reset_state()
            return opt, None, 0
        st = self._setup_inputs(plan.n_kf)
        st["depth"].copy_(cur_gt_depth)
        st["color"].copy_(cur_gt_color)
        st["c2w"][:cur_c2w.shape[0]].copy_(cur_c2w)
        if kfs:
            st["poses"][:len(kfs)].copy_(torch.stack([kf["est_c2w"].to(self.device).float()[:4] for kf in kfs]))
        # (the warm-up is the setup itself: the engine's capacity buffers, the Adam state and torch's caches)
        g, (counts, n_samp), _ = self._graphs.graph(plan, body=lambda: self._run_setup(plan, eng, st),
                                                    warm=lambda: self._run_setup(plan, eng, st))
        g.replay()
        return self._optimizer(eng, plan.trainable), counts, n_samp

    def _stage_plans(self, num_joint_iters, lr_factor, win):
        """A call's schedule over the window `win` as StagePlans, one per run of a stage (Mapper.py:403-421)."""
        rates = self.cfg["mapping"]["stage"]
        trainable, record = self._trainable(), self.loss_history is not None
        camera = (int(self.H), int(self.W), (float(self.fx), float(self.fy), float(self.cx), float(self.cy)))
        plans = []
        for stage, iters in self._stage_runs(num_joint_iters):
            # device draws: the next iteration's gather + sampler run beside this one's render and backward
            # (engine prefetch); every run of one stage starts with its own batch (eng.drop_prefetch), so a
            # captured run holds its whole prefetch chain.  With BA the poses the rays come from move only in
            # the colour stage (the cameras' lr is 0 before it, Mapper.py:420-421: their Adam state advances,
            # the 7-vectors do not), so only colour-stage BA iterations draw their rays serially.
            prefetch = win.ar is None and (not win.ncam or stage != "color")
            plans.append(StagePlan(
                "stage", stage, iters, win.F, win.n_per, win.c0, win.ncam,
                tuple(rates[stage][name + "_lr"] * lr_factor for name in _STAGE_GROUPS),
                float(self.BA_cam_lr) if (win.ncam and stage == "color") else 0.0,
                trainable, record, not plans and win.ncam > 0, prefetch, *camera, int(self._draw_seed)))
        return plans

    @staticmethod
    def _set_stage_lr(plan, opt, win, zero=False):
        """The run's learning rates (Mapper.py:413-421), or all zero."""
        for group, lr in zip(opt.param_groups, plan.lrs):
            group["lr"] = 0.0 if zero else lr
        if plan.ncam:
            win.copt.param_groups[0]["lr"] = 0.0 if zero else plan.cam_lr

    @staticmethod
    def _fused_iteration(plan, eng, opt, win, record=None, generator=None):
        """One mapping iteration of `plan` on the engine over the window `win`; record(ray_loss) when given.
        generator: of the select_uv draws (a window with eager draws, win.ar)."""
        n_per = plan.n_per
        pix = None
        if win.ar is not None:  # select_uv per frame, in optimize_frame order (Mapper.py:437-467)
            ar = win.ar
            pix = torch.empty(plan.F * n_per, dtype=torch.int64, device=ar.device)
            for fr in win.optimize_frame:
                s = win.order.index(fr)
                pix[s * n_per:(s + 1) * n_per] = _common.select_uv(ar, ar, n_per, ar, ar.view(-1, 1).expand(-1, 3),
                                                                   device=ar.device, generator=generator)[0]
        ray_loss, _ = eng.iteration(plan.stage, win.frames, pix, n_per, (plan.H, plan.W), plan.intrinsics, opt,
                                    trainable_decoders=plan.trainable, use_gt_in_sampler=plan.stage != "coarse",
                                    seed=plan.seed, post_bwd=win.post_bwd if plan.ncam else None,
                                    prefetch=plan.prefetch)
        if record is not None:
            record(ray_loss)

    @staticmethod
    def _run_stage(plan, eng, opt, win, record=None, hook=None, generator=None):
        """The run `plan`, as the eager path executes and a stage graph captures it: its rates, its own first
        batch, the BA cameras' set-up when it is the call's first run, then the iterations — hook(i) before
        and record(i, ray_loss) after the i-th.  Every host value comes from the plan."""
        Mapper._set_stage_lr(plan, opt, win)
        eng.drop_prefetch()
        if plan.first:
            win.cams_init()
        for i in range(plan.iters):
            if hook is not None:
                hook(i)
            Mapper._fused_iteration(plan, eng, opt, win, None if record is None else functools.partial(record, i),
                                    generator)

    def _stage_graph(self, plan, eng, opt, win):
        """The run `plan` as a cached hipGraph → (graph, its losses [iters] or None, captured now).  Its
        warm-up is one zero-lr eager iteration: the maps do not move, but the Adam state advances and BA
        rewrites the slots' poses, which the caller resets after a capture."""
        draws = eng.draws(plan.seed)
        losses = None

        def warm():
            nonlocal losses
            if plan.ncam:
                win.cams_init()
            self._set_stage_lr(plan, opt, win, zero=True)
            eng.drop_prefetch()
            self._fused_iteration(plan, eng, opt, win)
            if plan.record:  # (made before the capture: not from the graph's pool, no fill in the graph)
                losses = torch.zeros(plan.iters, dtype=torch.float64, device=eng.device)

        def body():
            self._run_stage(plan, eng, opt, win, None if losses is None else (lambda i, rl: losses[i].copy_(rl.sum())))
            return losses, draws  # (draws: kept with the graph that advances it, ops.GraphCache)

        g, (losses, _), captured = self._graphs.graph(plan, body, warm, rewind=[draws.counter])
        return g, losses, captured

    def _optimize_map_fused(self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w,
                            keyframe_dict, keyframe_list, cur_c2w):
        """optimize_map on the fused engine, in the numbered steps below (see the module docstring)."""
        dev = self.device
        tm = {"t0": time.perf_counter(), "ev": {}} if self.timing is not None else None
        cur_gt_depth = cur_gt_depth.to(dev).float()
        cur_gt_color = cur_gt_color.to(dev).float()
        cur_c2w = cur_c2w.to(dev).float()
        eng = self.engine()
        for d in eng.decs.values():  # parameters may have been assigned since the last call
            d.repack()
        device_draws = _common.device_draws(self.generator)
        use_graphs = _common.replays_graphs(self)
        # 1. Everything that does not depend on the keyframe selection is enqueued first: the selection reads
        # its overlap scores back to the host (the reference's numpy ranking), and what is queued before
        # that read overlaps the previous call's iterations still running on the device.
        overlap_here = (use_graphs and self.keyframe_selection_method == "overlap" and len(keyframe_dict) > 1
                        and "keyframe_selection_overlap" not in self.__dict__)
        opt, counts, n_samp = self._fused_setup(eng, use_graphs, overlap_here, cur_gt_color, cur_gt_depth, cur_c2w,
                                                keyframe_dict)
        self._mark(tm, "masks")
        # 2. the window: from the captured overlap counts (one read-back; Mapper.py:256-272) or selected here
        if overlap_here:
            selected = self._rank_keyframes([int(c) / n_samp for c in counts.cpu()], self.mapping_window_size - 2)
        else:
            selected = self._select_keyframes(keyframe_dict, cur_gt_color, cur_gt_depth, cur_c2w)
        optimize_frame, oldest_frame = self._window_of(selected, keyframe_list)
        self._mark(tm, "selected")
        self._record_selected(idx, optimize_frame, keyframe_dict, keyframe_list, gt_cur_c2w, cur_c2w)
        # 3. its frames in the persistent slots, and the BA cameras
        win = _Window(self, optimize_frame, oldest_frame, keyframe_dict, cur_gt_depth, cur_gt_color, cur_c2w,
                      device_draws)
        # 4. the schedule: one plan per stage run; 5. with graphs, each plan's graph
        plans = self._stage_plans(num_joint_iters, lr_factor, win)
        hist = self.loss_history
        if use_graphs:
            graphs = [self._stage_graph(plan, eng, opt, win) for plan in plans]
            if any(captured for _, _, captured in graphs):  # (what the warm-up iterations moved)
                opt.reset_state()
                win.restore_poses()
        self._mark(tm, "window")
        # 6. the iterations: replayed, or eagerly with the hook before each (Mapper.py:426-428)
        if use_graphs:
            for plan, (g, losses, _) in zip(plans, graphs):
                self.stage = plan.stage
                g.replay()
                if hist is not None:
                    hist.extend(losses.clone().unbind())
        else:
            done = 0
            for plan in plans:
                self.stage = plan.stage
                hook = self._iter_hook
                self._run_stage(plan, eng, opt, win, None if hist is None else (lambda i, rl: hist.append(rl.sum())),
                                None if hook is None else (lambda i, done=done: hook(done + i)), self.generator)
                done += plan.iters
        self._mark(tm, "iterations")
        if tm is not None:
            self.timing.append(tm)
        # 7. BA write-back (Mapper.py:521-540)
        return win.write_back(keyframe_dict, cur_c2w) if win.ncam else None

    # -- optimize_map under autograd: the NICE drop-in and iMAP* -----------------------------------
    def _autograd_window(self, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w, keyframe_dict, keyframe_list, cur_c2w):
        """The current frame on the device and the call's window (Mapper.py:240-287)."""
        cur = (cur_gt_depth.to(self.device), cur_gt_color.to(self.device).float(), cur_c2w.to(self.device))
        optimize_frame, oldest_frame = self._window_of(self._select_keyframes(keyframe_dict, cur[1], cur[0], cur[2]),
                                                       keyframe_list)
        self._record_selected(idx, optimize_frame, keyframe_dict, keyframe_list, gt_cur_c2w, cur[2])
        return cur, optimize_frame, oldest_frame

    def _ba_cameras(self, optimize_frame, oldest_frame, keyframe_dict, cur_c2w):
        """The 7-vector leaves of the window's cameras but the oldest (Mapper.py:349-363); none without BA."""
        cam_tensors = []
        if self.BA:
            for frame in optimize_frame:
                if frame != oldest_frame:
                    c2w = keyframe_dict[frame]["est_c2w"] if frame != -1 else cur_c2w
                    cam_tensors.append(get_tensor_from_camera(c2w).to(self.device).requires_grad_(True))
        return cam_tensors

    def _window_rays(self, optimize_frame, oldest_frame, keyframe_dict, cam_tensors, cur, pixs_per_image):
        """An iteration's ray batch (Mapper.py:437-467): pixs_per_image draws per frame in optimize_frame order,
        through the BA leaves where a frame has one.  cur = (depth, colour, c2w) of the current frame."""
        H, W, fx, fy, cx, cy = self.H, self.W, self.fx, self.fy, self.cx, self.cy
        device = self.device
        batch = []
        cam_id = 0
        for frame in optimize_frame:
            if frame != -1:
                gt_depth, gt_color = self._frame_images(keyframe_dict[frame])
                if self.BA and frame != oldest_frame:
                    c2w = get_camera_from_tensor(cam_tensors[cam_id])
                    cam_id += 1
                else:
                    c2w = keyframe_dict[frame]["est_c2w"].to(device)
            else:
                gt_depth, gt_color = cur[0], cur[1]
                c2w = get_camera_from_tensor(cam_tensors[cam_id]) if self.BA else cur[2]
            batch.append([t.float() for t in get_samples(0, H, 0, W, pixs_per_image, H, W, fx, fy, cx, cy, c2w,
                                                         gt_depth, gt_color, device, generator=self.generator)])
        return [torch.cat(ts) for ts in zip(*batch)]  # rays_o, rays_d, gt_depth, gt_color

    def _ba_write_back(self, optimize_frame, oldest_frame, keyframe_dict, cam_tensors, cur_c2w):
        """Mapper.py:521-540: the optimised poses into keyframe_dict; returns the current frame's (None without BA)."""
        if not self.BA:
            return None
        cam_id = 0
        for frame in optimize_frame:
            if frame != -1:
                if frame != oldest_frame:
                    c2w = get_camera_from_tensor(cam_tensors[cam_id].detach())
                    keyframe_dict[frame]["est_c2w"] = pose4(c2w).clone()
                    cam_id += 1
            else:
                cur_c2w = pose4(get_camera_from_tensor(cam_tensors[-1].detach())).clone()
        return cur_c2w

    def _optimize_map_autograd(self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w,
                               keyframe_dict, keyframe_list, cur_c2w):
        """The autograd drop-in of optimize_map (Mapper.py:230-540 line for line, HIP ops under autograd)."""
        c, cfg, device = self.c, self.cfg, self.device
        cur, optimize_frame, oldest_frame = self._autograd_window(idx, cur_gt_color, cur_gt_depth, gt_cur_c2w,
                                                                  keyframe_dict, keyframe_list, cur_c2w)
        pixs_per_image = self.mapping_pixels // len(optimize_frame)

        groups = {name: [] for name in _STAGE_GROUPS}
        masked = {}
        for key, val in c.items():
            if self.frustum_feature_selection:
                mask = self.get_mask_from_c2w(cur[2], key, val.shape[2:], cur[0])
                mask = mask.permute(2, 1, 0)[None, None].expand(1, val.shape[1], -1, -1, -1)
                vg = val.detach()[mask].clone().requires_grad_(True)
                masked[key] = (vg, mask)
                groups[key[5:]].append(vg)
            else:
                val = val.detach().requires_grad_(True)
                c[key] = val
                groups[key[5:]].append(val)
        trainable = []
        if not self.fix_fine:
            trainable += list(self.decoders.fine_decoder.parameters())
        if not self.fix_color:
            trainable += list(self.decoders.color_decoder.parameters())
        groups["decoders"] = trainable
        saved_rg = {p: p.requires_grad for p in self.decoders.parameters()}
        ids = {id(p) for p in trainable}
        for p in self.decoders.parameters():
            p.requires_grad_(id(p) in ids)

        cam_tensors = self._ba_cameras(optimize_frame, oldest_frame, keyframe_dict, cur[2])
        pg = [{"params": groups[name], "lr": 0} for name in _STAGE_GROUPS]
        if self.BA:
            pg.append({"params": cam_tensors, "lr": 0})
        optimizer = torch.optim.Adam(pg)

        bound = self.bound.to(device)
        for joint_iter in range(num_joint_iters):
            if self.frustum_feature_selection:
                for key, val in c.items():
                    if (self.coarse_mapper and "coarse" in key) or (not self.coarse_mapper and "coarse" not in key):
                        vg, mask = masked[key]
                        val = val.detach()
                        val[mask] = vg
                        c[key] = val
            self.stage = self._stage_of(joint_iter, num_joint_iters)
            st = cfg["mapping"]["stage"][self.stage]
            for gi, name in enumerate(_STAGE_GROUPS):
                optimizer.param_groups[gi]["lr"] = st[name + "_lr"] * lr_factor
            if self.BA and self.stage == "color":
                optimizer.param_groups[5]["lr"] = self.BA_cam_lr
            if self._iter_hook is not None:
                self._iter_hook(joint_iter)

            optimizer.zero_grad()
            rays_o, rays_d, gt_d, gt_c = self._window_rays(optimize_frame, oldest_frame, keyframe_dict, cam_tensors,
                                                           cur, pixs_per_image)
            keep = inside_mask(rays_o, rays_d, gt_d, bound)  # Mapper.py:469-481
            rays_o, rays_d, gt_d, gt_c = rays_o[keep], rays_d[keep], gt_d[keep], gt_c[keep]
            depth, uncertainty, color = self.renderer.render_batch_ray(
                c, self.decoders, rays_d, rays_o, device, self.stage, gt_depth=None if self.coarse_mapper else gt_d)
            dm = gt_d > 0
            loss = torch.abs(gt_d[dm] - depth[dm]).sum()
            if self.stage == "color":
                loss = loss + self.w_color_loss * torch.abs(gt_c - color).sum()
            loss.backward(retain_graph=False)
            if self.loss_history is not None:
                self.loss_history.append(loss.detach())
            optimizer.step()
            optimizer.zero_grad()
            if self.frustum_feature_selection:
                for key, val in c.items():
                    if (self.coarse_mapper and "coarse" in key) or (not self.coarse_mapper and "coarse" not in key):
                        vg, mask = masked[key]
                        val = val.detach()
                        val[mask] = vg.detach()
                        c[key] = val

        for p, rg in saved_rg.items():
            p.requires_grad_(rg)
        return self._ba_write_back(optimize_frame, oldest_frame, keyframe_dict, cam_tensors, cur[2])

    def _optimize_map_imap(self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w,
                           keyframe_dict, keyframe_list, cur_c2w):
        """optimize_map for iMAP* (the nice=False branches of Mapper.py:230-540), HIP ops under autograd: no
        grids and no inside mask; every iteration is stage 'color' with the colour loss and the 0.0005 |sigma|
        regulation term (Mapper.py:490-503); one Adam group over all decoder parameters at imap_decoders_lr
        under StepLR(200, 0.8), plus the BA cameras at BA_cam_lr (Mapper.py:342-345, 380-389, 420-424)."""
        device = self.device
        cur, optimize_frame, oldest_frame = self._autograd_window(idx, cur_gt_color, cur_gt_depth, gt_cur_c2w,
                                                                  keyframe_dict, keyframe_list, cur_c2w)
        pixs_per_image = self.mapping_pixels // len(optimize_frame)
        cam_tensors = self._ba_cameras(optimize_frame, oldest_frame, keyframe_dict, cur[2])
        pg = [{"params": list(self.decoders.parameters()), "lr": 0}]
        if self.BA:
            pg.append({"params": cam_tensors, "lr": 0})
        optimizer = torch.optim.Adam(pg)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=200, gamma=0.8)
        for joint_iter in range(num_joint_iters):
            self.stage = "color"
            optimizer.param_groups[0]["lr"] = self.cfg["mapping"]["imap_decoders_lr"]
            if self.BA:
                optimizer.param_groups[1]["lr"] = self.BA_cam_lr
            if self._iter_hook is not None:
                self._iter_hook(joint_iter)
            rays_o, rays_d, gt_d, gt_c = self._window_rays(optimize_frame, oldest_frame, keyframe_dict, cam_tensors,
                                                           cur, pixs_per_image)
            depth, uncertainty, color = self.renderer.render_batch_ray(self.c, self.decoders, rays_d, rays_o, device,
                                                                       self.stage, gt_depth=gt_d)
            dm = gt_d > 0
            loss = torch.abs(gt_d[dm] - depth[dm]).sum()
            loss = loss + self.w_color_loss * torch.abs(gt_c - color).sum()
            sigma = self.renderer.regulation(self.c, self.decoders, rays_d, rays_o, gt_d, device, self.stage,
                                             generator=self.generator, t_rand=self._next_t_rand(gt_d.shape[0]))
            loss = loss + 0.0005 * torch.abs(sigma).sum()
            loss.backward(retain_graph=False)
            if self.loss_history is not None:
                self.loss_history.append(loss.detach())
            optimizer.step()
            scheduler.step()
            optimizer.zero_grad()
        return self._ba_write_back(optimize_frame, oldest_frame, keyframe_dict, cam_tensors, cur[2])

    # -- the frame loop (Mapper.run, Mapper.py:542-657) --------------------------------------------
    _iter_hook = None  # map_frame(): called as hook(joint_iter) before each mapping iteration (the visualiser)
    save_selected_keyframes_info = False  # (attach_run reads the config's)

    def _record_selected(self, idx, optimize_frame, keyframe_dict, keyframe_list, gt_cur_c2w, cur_c2w):
        """Mapper.py:274-287: the call's window as selected_keyframes[idx]."""
        if not self.save_selected_keyframes_info:
            return
        info = []
        for frame in optimize_frame:
            if frame != -1:
                info.append({"idx": keyframe_list[frame], "gt_c2w": keyframe_dict[frame]["gt_c2w"],
                             "est_c2w": keyframe_dict[frame]["est_c2w"]})
            else:
                info.append({"idx": idx, "gt_c2w": gt_cur_c2w, "est_c2w": cur_c2w})
        self.selected_keyframes[idx] = info

    def attach_run(self, slam):
        """What Mapper.__init__ (Mapper.py:23-92) takes from `slam` and cfg for the frame loop, and the mapping
        visualiser.  NICE_SLAM calls it once; optimize_map alone does not need it."""
        from .visualizer import Visualizer
        cfg, m = self.cfg, self.cfg["mapping"]
        self.idx = slam.idx
        self.logger = slam.logger
        self.mesher = slam.mesher
        self.output = slam.output
        self.verbose = slam.verbose
        self.low_gpu_mem = slam.low_gpu_mem
        self.mapping_idx = slam.mapping_idx
        self.mapping_cnt = slam.mapping_cnt
        self.mapping_first_frame = slam.mapping_first_frame
        self.n_img = slam.n_img
        self.pose_work = slam.pose_work
        self.mirror_poses = slam.mirror_poses
        self.sync_method = cfg["sync_method"]
        self.eval_rec = cfg["meshing"]["eval_rec"]
        self.clean_mesh = cfg["meshing"]["clean_mesh"]
        self.mesh_coarse_level = cfg["meshing"]["mesh_coarse_level"]
        self.mesh_freq, self.ckpt_freq = m["mesh_freq"], m["ckpt_freq"]
        self.every_frame, self.keyframe_every = m["every_frame"], m["keyframe_every"]
        self.color_refine = m["color_refine"]
        self.no_vis_on_first_frame = m["no_vis_on_first_frame"]
        self.no_log_on_first_frame = m["no_log_on_first_frame"]
        self.no_mesh_on_first_frame = m["no_mesh_on_first_frame"]
        self.save_selected_keyframes_info = m["save_selected_keyframes_info"]
        if self.save_selected_keyframes_info:
            self.selected_keyframes = {}
        self.visualizer = None
        if "Demo" not in self.output:  # Mapper.py:87-91: no mapping visualiser in the demo
            self.visualizer = Visualizer(freq=m["vis_freq"], inside_freq=m["vis_inside_freq"],
                                         vis_dir=os.path.join(self.output, "mapping_vis"), renderer=self.renderer,
                                         verbose=self.verbose, device=self.device)
        self._init = True

    def map_frame(self, idx, gt_color, gt_depth, gt_c2w):
        """One pass of Mapper.run's loop body (Mapper.py:572-654) for frame idx; True when it was the last.

        The colour-refinement pass mutates the live Mapper as the reference does (window ×2, both ratios 0,
        fix_color, frustum selection off).  Every one of these is in the plans that key the graphs and the
        optimiser, so the pass gets graphs and an optimiser of its own; the window slots regrow by size.

        On a frame whose mapping visualisation fires, optimize_map runs its eager fused path with the visualiser
        called before every iteration, where Mapper.py:426-428 has it; the first frame's one-off schedule
        (iters_first) runs eagerly too; every other frame replays the graphs."""
        import shutil
        idx = int(idx)
        cfg = self.cfg
        est = self.pose_work
        if self.verbose:
            print(("Coarse " if self.coarse_mapper else "") + "Mapping Frame ", idx)
        if idx == 0 and self._init:
            est[0] = gt_c2w.to(est.device)  # Mapper.py:546
        if not self._init:
            lr_factor = cfg["mapping"]["lr_factor"]
            num_joint_iters = cfg["mapping"]["iters"]
            if idx == self.n_img - 1 and self.color_refine and not self.coarse_mapper:
                outer_joint_iters = 5
                self.mapping_window_size *= 2
                self.middle_iter_ratio = 0.0
                self.fine_iter_ratio = 0.0
                num_joint_iters *= 5
                self.fix_color = True
                self.frustum_feature_selection = False
            else:
                outer_joint_iters = 1 if self.nice else 3
        else:
            outer_joint_iters = 1
            lr_factor = cfg["mapping"]["lr_first_factor"]
            num_joint_iters = cfg["mapping"]["iters_first"]
        cur_c2w = est[idx].to(self.device).clone()
        num_joint_iters = num_joint_iters // outer_joint_iters
        vis = self.visualizer
        if vis is not None and not (idx == 0 and self.no_vis_on_first_frame) and idx % vis.freq == 0:
            self._iter_hook = lambda it: vis.vis(idx, it, gt_depth, gt_color, self._hook_c2w, self.c, self.decoders)
        graphs = self.graphs
        if self._init:  # the first frame's schedule (iters_first) runs once: a graph of it would never be replayed
            self.graphs = False
        try:
            for outer_joint_iter in range(outer_joint_iters):
                self.BA = (len(self.keyframe_list) > 4) and cfg["mapping"]["BA"] and (not self.coarse_mapper)
                self._hook_c2w = cur_c2w
                _ = self.optimize_map(num_joint_iters, lr_factor, idx, gt_color, gt_depth, gt_c2w, self.keyframe_dict,
                                      self.keyframe_list, cur_c2w=cur_c2w)
                if self.BA:
                    cur_c2w = _
                    est[idx] = cur_c2w.to(est.device)
                if outer_joint_iter == outer_joint_iters - 1:
                    if (idx % self.keyframe_every == 0 or idx == self.n_img - 2) and idx not in self.keyframe_list:
                        self.keyframe_list.append(idx)
                        self.keyframe_dict.append({"gt_c2w": gt_c2w.cpu(), "idx": idx, "color": gt_color.cpu(),
                                                   "depth": gt_depth.cpu(), "est_c2w": cur_c2w.clone()})
        finally:
            self._iter_hook = None
            self.graphs = graphs
        if self.low_gpu_mem:
            torch.cuda.empty_cache()
        self._init = False
        self.mapping_first_frame[0] = 1
        last = idx == self.n_img - 1
        if not self.coarse_mapper:
            if ((not (idx == 0 and self.no_log_on_first_frame)) and idx % self.ckpt_freq == 0) or last:
                self.mirror_poses()
                self.logger.log(idx, self.keyframe_dict, self.keyframe_list,
                                selected_keyframes=self.selected_keyframes if self.save_selected_keyframes_info
                                else None)
            self.mapping_idx[0] = idx
            self.mapping_cnt[0] += 1
            out = f"{self.output}/mesh"
            kw = dict(clean_mesh=self.clean_mesh, get_mask_use_all_frames=False)
            if (idx % self.mesh_freq == 0) and (not (idx == 0 and self.no_mesh_on_first_frame)):
                self.mirror_poses()
                self.mesher.get_mesh(f"{out}/{idx:05d}_mesh.ply", self.c, self.decoders, self.keyframe_dict,
                                     self.estimate_c2w_list, idx, self.device, show_forecast=self.mesh_coarse_level, **kw)
            if last:
                self.mirror_poses()
                self.mesher.get_mesh(f"{out}/final_mesh.ply", self.c, self.decoders, self.keyframe_dict,
                                     self.estimate_c2w_list, idx, self.device, show_forecast=self.mesh_coarse_level, **kw)
                if os.path.exists(f"{out}/final_mesh.ply"):  # Mapper.py:649-650 (cp)
                    shutil.copyfile(f"{out}/final_mesh.ply", f"{out}/{idx:05d}_mesh.ply")
                if self.eval_rec:
                    self.mesher.get_mesh(f"{out}/final_mesh_eval_rec.ply", self.c, self.decoders, self.keyframe_dict,
                                         self.estimate_c2w_list, idx, self.device, show_forecast=False,
                                         clean_mesh=self.clean_mesh, get_mask_use_all_frames=True)
        return last

    def _next_t_rand(self, n_rays):
        return self.regulation_draws(n_rays) if self.regulation_draws is not None else None
