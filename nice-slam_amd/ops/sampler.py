"""The ray samplers of csrc/nslam_sampler.hip: stratified + surface samples, the hierarchical importance sampler."""
import ctypes

import torch

from . import span
from .._lib import check, lib, ptr, stream_ptr
from ._check import bound_list


_T_CACHE = {}


def _t_tables(device, s0, s1):
    key = (str(device), s0, s1)
    if key not in _T_CACHE:
        ts = torch.linspace(0.0, 1.0, s0).to(device)
        tu = torch.linspace(0.0, 1.0, max(s1, 1)).double().to(device)
        _T_CACHE[key] = (ts, tu)
    return _T_CACHE[key]


def sample_z(rays_o, rays_d, gt_depth, bound, n_strat, n_surf, lindisp=False, gt_max=None, out=None):
    """z_vals [N, n_strat(+n_surf)] float64 (surface samples only when gt_depth is given).

    gt_max: optional device float scalar = max(gt_depth) over the FULL batch (ray sharding).
    out: optional preallocated z tensor of that shape (persistent buffers of a captured loop).
    """
    ro = rays_o.detach().float().contiguous()
    rd = rays_d.detach().float().contiguous()
    n = ro.shape[0]
    s1 = n_surf if gt_depth is not None else 0
    if out is not None:
        if tuple(out.shape) != (n, n_strat + s1) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 [N, S] tensor")
        z = out
    else:
        z = torch.empty(n, n_strat + s1, dtype=torch.float64, device=ro.device)
    if n == 0:
        return z
    gt = gt_depth.detach().float().reshape(-1).contiguous() if gt_depth is not None else None
    ts, tu = _t_tables(ro.device, n_strat, n_surf)
    lo, hi = bound_list(bound)
    L = lib()
    wsb = L.nslam_workspace_size(0, n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=ro.device)
    with span("sample_rays"):
        gm = gt_max.detach().float().reshape(1).contiguous() if (gt_max is not None and gt is not None) else None
        rc = L.nslam_sample_rays(ptr(ro), ptr(rd), ptr(gt), ptr(gm), n, (ctypes.c_double * 3)(*lo),
                                 (ctypes.c_double * 3)(*hi), ptr(ts), n_strat, ptr(tu), s1, int(bool(lindisp)),
                                 ptr(z), ptr(ws), wsb, stream_ptr(ro.device))
    check(rc, "nslam_sample_rays")
    return z


def sample_importance(z, weights, n_importance, merged=True):
    """sort(cat(z, sample_pdf(z_mid, weights[..., 1:-1], n_importance, det=True))) → [N, S + n_importance] f64;
    merged=False: the n_importance new samples alone."""
    z = z.detach().double().contiguous()
    w = weights.detach().float().contiguous()
    n, s = z.shape
    if tuple(w.shape) != (n, s):
        raise ValueError("weights must have z's shape")
    key = (str(z.device), "u", n_importance)
    if key not in _T_CACHE:
        _T_CACHE[key] = torch.linspace(0.0, 1.0, steps=n_importance).to(z.device)
    u = _T_CACHE[key]
    out = torch.empty(n, (s if merged else 0) + n_importance, dtype=torch.float64, device=z.device)
    if n:
        with span("sample_importance"):
            rc = lib().nslam_sample_importance(ptr(z), ptr(w), ptr(u), n, s, n_importance,
                                               ptr(out) if merged else None, None if merged else ptr(out),
                                               stream_ptr(z.device))
        check(rc, "nslam_sample_importance")
    return out
