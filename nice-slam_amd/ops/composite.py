"""The ray compositor of csrc/nslam_composite.hip: occupancy, volume density, the fused rendering loss."""
import ctypes

import torch

from . import span
from .. import _lib
from .._lib import check, lib, ptr, stream_ptr


def _composite_call(which, raw, z, rd, tensors, last):
    """nslam_composite_<which>, or with rays_d nslam_composite_density_<which>: the same arguments plus rays_d
    after z and one more tensor (`last`) before the stream."""
    name = f"composite_{which}" if rd is None else f"composite_density_{which}"
    n, s = z.shape
    rays, extra = ((), ()) if rd is None else ((ptr(rd),), (ptr(last),))
    with span(name):
        rc = getattr(lib(), "nslam_" + name)(ptr(raw), ptr(z), *rays, n, s, *(ptr(t) for t in tensors), *extra,
                                             stream_ptr(raw.device))
    check(rc, "nslam_" + name)


class _Composite(torch.autograd.Function):
    """The ray compositor: occupancy mode (rays_d None), or volume density with rays_d [N,3], which adds the
    non-differentiable weights output and the gradient of rays_d."""

    @staticmethod
    def forward(ctx, raw, z, rays_d):
        raw = raw.detach().float().contiguous()
        z = z.detach().double().contiguous()
        rd = rays_d.detach().float().contiguous() if rays_d is not None else None
        n, s = z.shape
        dev = raw.device
        depth = torch.empty(n, dtype=torch.float64, device=dev)
        var = torch.empty(n, dtype=torch.float64, device=dev)
        color = torch.empty(n, 3, dtype=torch.float32, device=dev)
        weights = torch.empty(n, s, dtype=torch.float32, device=dev) if rd is not None else None
        if n:
            _composite_call("fwd", raw, z, rd, (depth, var, color), weights)
        ctx.save_for_backward(raw, z, rd)
        if rd is None:
            return depth, var, color
        ctx.mark_non_differentiable(weights)
        return depth, var, color, weights

    @staticmethod
    def backward(ctx, gd, gv, gc, _gw=None):
        raw, z, rd = ctx.saved_tensors
        g_raw = torch.empty_like(raw)
        g_rd = torch.zeros_like(rd) if rd is not None and ctx.needs_input_grad[2] else None
        if z.shape[0]:
            gd = gd.contiguous().double() if gd is not None else None
            gv = gv.contiguous().double() if gv is not None else None
            gc = gc.contiguous().float() if gc is not None else None
            _composite_call("bwd", raw, z, rd, (gd, gv, gc, g_raw), g_rd)
        return g_raw, None, g_rd


def composite(raw, z):
    """(depth f64 [N], var f64 [N], color f32 [N,3]) from raw [N,S,4] f32, z [N,S] f64."""
    return _Composite.apply(raw, z, None)


def composite_density(raw, z, rays_d):
    """(depth f64 [N], var f64 [N], color f32 [N,3], weights f32 [N,S]) of raw2outputs_nerf_color(occupancy=False);
    differentiable in raw and rays_d (the |rays_d| factor of dists); weights is for the sampler (no gradient)."""
    return _Composite.apply(raw, z, rays_d)


def render_loss(raw, z, gt_depth, gt_color, keep=None, mode="mapper", use_color=True, handle_dynamic=False,
                w_color=0.2, want_grad=True, occ_add=None):
    """Mapper/Tracker rendering loss fused with compositing and its backward (see nslam.h).

    raw [N,S,4] (or [N*S,4]) f32, z [N,S] f64.  Returns (depth f64 [N], var f64 [N],
    color f32 [N,3], ray_loss f64 [N], g_raw f32 like raw or None) where sum(ray_loss) is the loss
    and g_raw = dloss/draw.
    """
    z = z.detach().double().contiguous()
    n, s = z.shape
    dev = z.device
    raw = raw.detach().float().contiguous()
    cfg = _lib.NslamLossCfg(_lib.LOSS_MAPPER if mode == "mapper" else _lib.LOSS_TRACKER, int(bool(use_color)),
                            int(bool(handle_dynamic)), float(w_color), ptr(occ_add))
    depth = torch.empty(n, dtype=torch.float64, device=dev)
    var = torch.empty(n, dtype=torch.float64, device=dev)
    color = torch.empty(n, 3, dtype=torch.float32, device=dev)
    ray_loss = torch.empty(n, dtype=torch.float64, device=dev)
    g_raw = torch.empty_like(raw) if want_grad else None
    wsb = lib().nslam_render_loss_workspace_size(ctypes.byref(cfg), n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    gt_depth = gt_depth.detach().float().contiguous()
    gt_color = gt_color.detach().float().contiguous() if gt_color is not None else None
    keep = keep.contiguous() if keep is not None else None
    if n:
        with span("render_loss"):
            rc = lib().nslam_render_loss(ctypes.byref(cfg), ptr(raw), ptr(z), n, s, ptr(gt_depth), ptr(gt_color),
                                         ptr(keep), ptr(depth), ptr(var), ptr(color), ptr(ray_loss), ptr(g_raw),
                                         ptr(ws), wsb, stream_ptr(dev))
        check(rc, "nslam_render_loss")
    return depth, var, color, ray_loss, g_raw
