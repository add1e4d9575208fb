"""The visualiser's panel mosaic, csrc/nslam_vis.hip."""
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._check import _expect


def vis_panels(gt_depth, gt_color, depth, color, vmax, out=None):
    """nslam_vis_panels: the visualiser's six panels as one uint8 device image [2H, 3W, 3] (include/nslam.h has
    the contract; visualizer.vis_panels_np is the numpy twin).  gt_depth [H, W] f32, gt_color [H, W, 3] f32, depth
    [H, W] f64, color [H, W, 3] f32, vmax a float32 device scalar; all contiguous.  One launch on the current
    stream, no host synchronisation."""
    if gt_depth.dim() != 2:
        raise ValueError("vis_panels: gt_depth must be [H, W]")
    H, W = gt_depth.shape
    _expect("vis_panels", [(gt_depth, torch.float32, (H, W)), (gt_color, torch.float32, (H, W, 3)),
                           (depth, torch.float64, (H, W)), (color, torch.float32, (H, W, 3)),
                           (vmax, torch.float32, vmax.shape)])
    if vmax.numel() != 1:
        raise ValueError("vis_panels: vmax must be a device scalar")
    if out is None:
        out = torch.empty(2 * H, 3 * W, 3, dtype=torch.uint8, device=gt_depth.device)
    _expect("vis_panels", [(out, torch.uint8, (2 * H, 3 * W, 3))])
    if H * W == 0:
        return out
    rc = lib().nslam_vis_panels(ptr(gt_depth), ptr(gt_color), ptr(depth), ptr(color), H, W, ptr(vmax), ptr(out),
                                stream_ptr(gt_depth.device))
    check(rc, "nslam_vis_panels")
    return out
