"""NICE_SLAM drop-in (src/NICE_SLAM.py): the SLAM system — point it at a sequence, get the trajectory,
checkpoints, meshes and visualisations.

`NICE_SLAM(cfg, args)` takes the reference's arguments and exposes its attributes (output, ckptsdir,
frame_reader, n_img, the shared lists and counters, renderer, mesher, logger, mapper, coarse_mapper when
cfg['coarse'], tracker) on top of slam.SlamState.

run() is a single-process, single-stream scheduler.  Under `sync_method: strict` the reference's three polling
processes never overlap: the tracker waits at frame idx (idx % every_frame == 1, or every_frame == 1) until
mapping_idx == idx-1 (Tracker.py:164-168), and the mapper waits until the tracker has published a frame with
idx % every_frame == 0, or the last one (Mapper.py:552-558).  The sequence they perform is therefore

    map(0); track(0); for idx in 1..n_img-1: track(idx); map(idx) when idx % every_frame == 0 or idx == n_img-1

which is what run() does, so nothing is lost against the reference.  Deviations:
  * `loose` and `free` run the same serial order (the reference lets the two processes drift there);
  * the coarse mapper maps every frame the mapper maps, right after it.  The reference's coarse process polls
    the same condition on its own clock, so which frames it catches depends on process timing and is not pinned;
  * one dataset reader serves tracker and mapper (the reference builds one per consumer): the frame comes once
    from frame_reader.prefetch() and the mapper reuses the tracker's frame; colour frames are float32 (the
    reference hands out float64 and its consumers convert);
  * the pose lists have a working copy on the device (pose_work, gt_pose_work) so that a tracked frame costs no
    host synchronisation; mirror_poses() copies them into the CPU tensors estimate_c2w_list / gt_c2w_list that
    Logger and Mesher read, before each log or mesh event and at the end.  On the CPU the working copies are
    the lists themselves.
Multi-process orchestration and CUDA-IPC sharing are out of scope.
"""
from __future__ import annotations

import os

import torch

from .datasets import get_dataset
from .logger import Logger
from .mapper import Mapper
from .slam import SlamState
from .tracker import Tracker


class NICE_SLAM(SlamState):
    def __init__(self, cfg, args):
        self.args = args
        device = cfg["mapping"]["device"]
        self.dataset = cfg["dataset"]
        self.scale = cfg["scale"]
        self.coarse_bound_enlarge = cfg["model"]["coarse_bound_enlarge"]
        self.frame_reader = self._frame_reader(cfg, args, device)
        self.n_img = len(self.frame_reader)
        self.prefetch = {}  # keywords of frame_reader.prefetch() in run() (workers, ahead)
        super().__init__(cfg, device=device, n_img=self.n_img, nice=args.nice)
        self.low_gpu_mem = cfg["low_gpu_mem"]
        self.verbose = cfg["verbose"]
        self.output = cfg["data"]["output"] if args.output is None else args.output
        self.ckptsdir = os.path.join(self.output, "ckpts")
        os.makedirs(self.output, exist_ok=True)
        os.makedirs(self.ckptsdir, exist_ok=True)
        os.makedirs(f"{self.output}/mesh", exist_ok=True)
        if self.nice:
            self.load_pretrain(cfg)
        if torch.device(device).type == "cpu":
            self.pose_work, self.gt_pose_work = self.estimate_c2w_list, self.gt_c2w_list
        else:
            self.pose_work = self.estimate_c2w_list.to(device)
            self.gt_pose_work = self.gt_c2w_list.to(device)
        self.logger = Logger(cfg, args, self)
        self.mapper = Mapper(cfg, args, self, coarse_mapper=False)
        self.mapper.attach_run(self)
        if self.coarse:
            self.coarse_mapper = Mapper(cfg, args, self, coarse_mapper=True)
            self.coarse_mapper.attach_run(self)
        self.tracker = Tracker(cfg, args, self)
        self.tracker.attach_run(self)
        self.print_output_desc()

    @staticmethod
    def _frame_reader(cfg, args, device):
        return get_dataset(cfg, args, cfg["scale"], device=device, color_dtype=torch.float32)

    def print_output_desc(self):
        """NICE_SLAM.py:96-108."""
        print(f"INFO: The output folder is {self.output}")
        if "Demo" in self.output:
            print("INFO: The GT, generated and residual depth/color images can be found under "
                  f"{self.output}/vis/")
        else:
            print("INFO: The GT, generated and residual depth/color images can be found under "
                  f"{self.output}/tracking_vis/ and {self.output}/mapping_vis/")
        print(f"INFO: The mesh can be found under {self.output}/mesh/")
        print(f"INFO: The checkpoint can be found under {self.output}/ckpt/")

    def load_pretrain(self, cfg):
        """NICE_SLAM.py:159-190: the pretrained ConvONet decoders.  Of ckpt['model'], the keys that contain
        'decoder' and not 'encoder': the coarse file's lose 'decoder.', the middle/fine file's
        'decoder_coarse.' go to the middle decoder and 'decoder_fine.' to the fine one.  A missing file is an
        error that names its config key: the system does not run on random decoders."""
        dev = cfg["mapping"]["device"]

        def load(key):
            path = cfg["pretrained_decoders"][key]
            if not os.path.isfile(path):
                raise FileNotFoundError(f"pretrained_decoders.{key}: {path!r} does not exist "
                                        "(the pretrained ConvONet decoders are required for --nice)")
            return torch.load(path, map_location=dev, weights_only=True)["model"]

        if self.coarse:
            coarse_dict = {}
            for key, val in load("coarse").items():
                if ("decoder" in key) and ("encoder" not in key):
                    coarse_dict[key[8:]] = val
            self.shared_decoders.coarse_decoder.load_state_dict(coarse_dict)
        middle_dict, fine_dict = {}, {}
        for key, val in load("middle_fine").items():
            if ("decoder" in key) and ("encoder" not in key):
                if "coarse" in key:
                    middle_dict[key[8 + 7:]] = val
                elif "fine" in key:
                    fine_dict[key[8 + 5:]] = val
        self.shared_decoders.middle_decoder.load_state_dict(middle_dict)
        self.shared_decoders.fine_decoder.load_state_dict(fine_dict)

    def mirror_poses(self):
        """The device working copies into the CPU lists Logger and Mesher read (a no-op on the CPU)."""
        if self.pose_work is not self.estimate_c2w_list:
            self.estimate_c2w_list.copy_(self.pose_work)
            self.gt_c2w_list.copy_(self.gt_pose_work)

    def _map(self, idx, frame):
        _, gt_color, gt_depth, gt_c2w = frame
        self.mapper.map_frame(idx, gt_color, gt_depth, gt_c2w)
        if self.coarse:
            self.coarse_mapper.map_frame(idx, gt_color, gt_depth, gt_c2w)

    def run(self):
        """The strict-sync sequence of the reference's tracking / mapping / coarse-mapping processes, serially
        (see the module docstring)."""
        every = self.cfg["mapping"]["every_frame"]
        for frame in self.frame_reader.prefetch(**self.prefetch):
            idx = int(frame[0])
            if idx == 0:  # tracking waits for the first frame's map (NICE_SLAM.py:262-266)
                self._map(0, frame)
                self.tracker.track(0, frame)
                continue
            self.tracker.track(idx, frame)
            if idx % every == 0 or idx == self.n_img - 1:
                self._map(idx, frame)
        self.mirror_poses()
