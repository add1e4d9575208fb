"""Visualizer drop-in (src/utils/Visualizer.py): depth / colour / residual images of a frame, on the device.

Same constructor arguments, same firing condition (`idx % freq == 0 and iter % inside_freq == 0`), same file
name (`{idx:05d}_{iter:04d}.jpg`), same six panels in the same order.  What differs: the output is not a
matplotlib figure (no titles, margins or resampling) but a pixel-exact uint8 mosaic [2H, 3W, 3]

    row 0:  input depth | generated depth | depth residual      (plasma, vmin 0, vmax = max(gt_depth))
    row 1:  input RGB   | generated RGB   | RGB residual

written by ONE kernel (nslam_vis_panels, csrc/nslam_vis.hip) from render_img's own output; vmax is an ordinary
torch reduction on the device, and the only host synchronisation of a call is the device-to-host copy of the
finished mosaic (18 bytes per pixel; the reference copies four float images, 44 bytes per pixel).  The JPEG is
Pillow's, with fixed parameters (JPEG_PARAMS).

`vis_panels_np` is the kernel's numpy twin, bit for bit the same contract (include/nslam.h):
  * depth panels follow matplotlib's Normalize(0, vmax) and Colormap.__call__(bytes=True) exactly, on the value
    as a float64: v == vmax takes the last colour, so does anything above, negatives the first, NaN is "bad"
    (black), and vmax == 0 maps everything (NaN included) to the first colour;
  * RGB panels are floor(255 * clip(v, 0, 1) + 0.5) in float32, NaN as 0 — this project's own rule, NOT pinned to
    matplotlib's internal image conversion (imshow resamples and converts RGB floats on its own path).
The 256 × 3 plasma table is csrc/nslam_plasma_lut.h, generated from matplotlib by tools/gen_plasma_lut.py; there
is no matplotlib import at run time.
"""
from __future__ import annotations

import io
import os
import re

import numpy as np
import torch

from .common import get_camera_from_tensor

JPEG_PARAMS = {"format": "JPEG", "quality": 90, "subsampling": 0, "optimize": False, "progressive": False}

_LUT = None


def plasma_lut():
    """The committed plasma table (csrc/nslam_plasma_lut.h) as uint8 [256, 3]."""
    global _LUT
    if _LUT is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "nslam_plasma_lut.h")
        with open(path) as f:
            rows = re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+)\}", f.read())
        lut = np.array(rows, dtype=np.int64).astype(np.uint8)
        if lut.shape != (256, 3):
            raise RuntimeError(f"{path}: expected 256 rows, found {lut.shape[0]}")
        _LUT = lut
    return _LUT


def _plasma_np(v, vmax):
    """Normalize(0, vmax) + Colormap.__call__(bytes=True) of plasma for a float64 array → uint8 [..., 3]."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = (np.zeros_like(v) if vmax == 0.0 else v / vmax) * 256.0
        bad = np.isnan(t)
        row = np.where(t >= 256.0, 255, np.where(t < 0.0, 0, np.where(bad, 0, t))).astype(np.int64)
    out = plasma_lut()[row]
    out[bad] = 0
    return out


def _rgb_np(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, np.minimum(v, np.float32(1)), np.float32(0)).astype(np.float32)
    return np.floor(np.float32(255) * c + np.float32(0.5)).astype(np.uint8)


def vis_panels_np(gt_depth, gt_color, depth, color, vmax=None):
    """The numpy twin of nslam_vis_panels: uint8 [2H, 3W, 3] from gt_depth [H, W] f32, gt_color [H, W, 3] f32,
    depth [H, W] f64, color [H, W, 3] f32; vmax defaults to max(gt_depth) (float32)."""
    gd = np.asarray(gt_depth, dtype=np.float32)
    gc = np.asarray(gt_color, dtype=np.float32)
    d = np.asarray(depth, dtype=np.float64)
    c = np.asarray(color, dtype=np.float32)
    H, W = gd.shape
    vmax = float(np.float32(np.max(gd) if vmax is None else vmax)) if gd.size else 0.0
    with np.errstate(invalid="ignore"):
        dres = np.abs(gd.astype(np.float64) - d)
        cres = np.abs(gc - c)
    dres[gd == 0] = 0.0
    cres[gd == 0] = 0.0
    out = np.empty((2 * H, 3 * W, 3), dtype=np.uint8)
    for k, img in enumerate((gd.astype(np.float64), d, dres)):
        out[:H, k * W:(k + 1) * W] = _plasma_np(img, vmax)
    for k, img in enumerate((gc, c, cres)):
        out[H:, k * W:(k + 1) * W] = _rgb_np(img)
    return out


def encode_jpeg(mosaic):
    """Pillow's JPEG of a uint8 [h, w, 3] array with the fixed JPEG_PARAMS → bytes."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(mosaic), "RGB").save(buf, **JPEG_PARAMS)
    return buf.getvalue()


class Visualizer(object):
    def __init__(self, freq, inside_freq, vis_dir, renderer, verbose, device="cuda:0"):
        self.freq = freq
        self.device = device
        self.vis_dir = vis_dir
        self.verbose = verbose
        self.renderer = renderer
        self.inside_freq = inside_freq
        os.makedirs(f"{vis_dir}", exist_ok=True)

    def fires(self, idx, iter):
        """Visualizer.py:40."""
        return int(idx) % self.freq == 0 and int(iter) % self.inside_freq == 0

    def panels(self, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders):
        """The mosaic of one visualisation as a uint8 device tensor [2H, 3W, 3] (no host synchronisation)."""
        from . import ops
        dev = self.device
        with torch.no_grad():
            if len(c2w_or_camera_tensor.shape) == 1:  # Visualizer.py:43-50
                bottom = torch.tensor([[0, 0, 0, 1.0]], dtype=torch.float32, device=dev)
                c2w = torch.cat([get_camera_from_tensor(c2w_or_camera_tensor.clone().detach()), bottom], dim=0)
            else:
                c2w = c2w_or_camera_tensor
            gt_depth = gt_depth.to(dev)
            depth, _, color = self.renderer.render_img(c, decoders, c2w, dev, stage="color", gt_depth=gt_depth)
            gd = gt_depth.float().contiguous()
            return ops.vis_panels(gd, gt_color.to(dev).float().contiguous(), depth.double().contiguous(),
                                  color.float().contiguous(), gd.max())

    def vis(self, idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders):
        """Visualizer.vis (Visualizer.py:25-107): writes {vis_dir}/{idx:05d}_{iter:04d}.jpg when it fires."""
        if not self.fires(idx, iter):
            return
        mosaic = self.panels(gt_depth, gt_color, c2w_or_camera_tensor, c, decoders)
        path = f"{self.vis_dir}/{int(idx):05d}_{int(iter):04d}.jpg"
        with open(path, "wb") as f:
            f.write(encode_jpeg(mosaic.cpu().numpy()))  # (the call's one host synchronisation)
        if self.verbose:
            print(f"Saved rendering visualization of color/depth image at {path}")
