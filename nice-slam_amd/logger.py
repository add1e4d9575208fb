"""Logger drop-in (src/utils/Logger.py): checkpoints through datasets.save_checkpoint — the reference's keys,
file name ({idx:05d}.tar under ckptsdir) and legacy serialisation."""
from __future__ import annotations

import os

from .datasets import save_checkpoint


class Logger(object):
    def __init__(self, cfg, args, slam):
        self.verbose = slam.verbose
        self.ckptsdir = slam.ckptsdir
        self.shared_c = slam.shared_c
        self.gt_c2w_list = slam.gt_c2w_list
        self.shared_decoders = slam.shared_decoders
        self.estimate_c2w_list = slam.estimate_c2w_list

    def log(self, idx, keyframe_dict, keyframe_list, selected_keyframes=None):
        path = os.path.join(self.ckptsdir, "{:05d}.tar".format(int(idx)))
        save_checkpoint(path, self.shared_c, self.shared_decoders, self.gt_c2w_list, self.estimate_c2w_list,
                        keyframe_list, idx, selected_keyframes=selected_keyframes)
        if self.verbose:
            print("Saved checkpoints at", path)
