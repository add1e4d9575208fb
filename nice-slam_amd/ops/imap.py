"""iMAP*, csrc/nslam_imap.hip: the 256-wide Fourier MLP, points or rays, forward and backward."""
import ctypes
import math

import torch

from . import span
from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from ._check import bound_list


def imap_struct(B, ws, bs, wo, bo):
    s = _lib.NslamImapParams()
    s.B = B.data_ptr()
    for i in range(4):
        s.w[i] = ws[i].data_ptr()
        s.b[i] = bs[i].data_ptr()
    s.wo = wo.data_ptr()
    s.bo = bo.data_ptr()
    return s


_IMAP_SHAPES = ((3, 93), (256, 93), (256,), (256, 256), (256,), (256, 256), (256,), (256, 256), (256,), (4, 256), (4,))


def imap_query_struct(pts, rays, bound):
    q = _lib.NslamImapQuery()
    if rays is None:
        q.pts = pts.data_ptr()
    else:
        ro, rd, z = rays
        q.rays_o, q.rays_d, q.z_vals, q.n_samples = ro.data_ptr(), rd.data_ptr(), z.data_ptr(), z.shape[1]
    lo, hi = bound if bound is not None else ([-math.inf] * 3, [math.inf] * 3)
    for k in range(3):
        q.bound_lo[k], q.bound_hi[k] = lo[k], hi[k]
    return q


class _ImapQuery(torch.autograd.Function):
    """raw [n,4] of the iMAP* decoder; differentiable in the points and the eleven parameter tensors."""

    @staticmethod
    def forward(ctx, bound, rays, pts, *params):
        if len(params) != 11:
            raise ValueError("imap_query takes _B, four (weight, bias) pairs and output_linear's weight and bias")
        params = [p.detach().float().contiguous() for p in params]
        for p, shp in zip(params, _IMAP_SHAPES):
            if tuple(p.shape) != shp:
                raise ValueError(f"iMAP* parameter of shape {tuple(p.shape)}, expected {shp}")
        dev = params[0].device
        if rays is None:
            pts = pts.detach().to(torch.float64).contiguous()
            n = pts.shape[0]
        else:
            rays = (rays[0].detach().float().contiguous(), rays[1].detach().float().contiguous(),
                    rays[2].detach().double().contiguous())
            n = rays[2].numel()
        L = lib()
        ps = imap_struct(params[0], params[1:9:2], params[2:9:2], params[9], params[10])
        packed = torch.empty(L.nslam_imap_packed_size() // 4, dtype=torch.float32, device=dev)
        check(L.nslam_imap_pack(ctypes.byref(ps), ptr(packed), stream_ptr(dev)), "nslam_imap_pack")
        raw = torch.empty(n, 4, dtype=torch.float32, device=dev)
        tape = None
        if any(ctx.needs_input_grad):
            tape = torch.empty(L.nslam_imap_tape_size(n) // 4, dtype=torch.float32, device=dev)
        q = imap_query_struct(pts, rays, bound)
        if n:
            with span("imap_fwd"):
                rc = L.nslam_imap_fwd(ctypes.byref(ps), ptr(packed), ctypes.byref(q), n, ptr(raw), ptr(tape),
                                      stream_ptr(dev))
            check(rc, "nslam_imap_fwd")
        ctx.bound, ctx.rays, ctx.pts, ctx.params, ctx.packed, ctx.tape, ctx.n = bound, rays, pts, params, packed, tape, n
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        need = ctx.needs_input_grad
        params, n = ctx.params, ctx.n
        dev = params[0].device
        L = lib()
        grads = [torch.zeros_like(p) for p in params] if any(need[3:]) else None
        g_pts = torch.zeros(n, 3, dtype=torch.float64, device=dev) if need[2] else None
        if n:
            g_raw = g_raw.contiguous().float()
            ps = imap_struct(params[0], params[1:9:2], params[2:9:2], params[9], params[10])
            gs = imap_struct(grads[0], grads[1:9:2], grads[2:9:2], grads[9], grads[10]) if grads else None
            q = imap_query_struct(ctx.pts, ctx.rays, ctx.bound)
            wsb = L.nslam_imap_bwd_workspace_size(n)
            ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
            with span("imap_bwd"):
                rc = L.nslam_imap_bwd(ctypes.byref(ps), ptr(ctx.packed), ctypes.byref(q), n, ptr(g_raw),
                                      ptr(ctx.tape), ctypes.byref(gs) if gs is not None else None, ptr(g_pts),
                                      ptr(ws), wsb, stream_ptr(dev))
            check(rc, "nslam_imap_bwd")
        out = [None, None, g_pts]
        out += [g if nd else None for g, nd in zip(grads, need[3:])] if grads else [None] * 11
        return tuple(out)


def imap_params(mlp):
    """The iMAP* module's tensors in the kernel's order."""
    ps = [mlp.embedder._B]
    for lin in mlp.pts_linears:
        ps += [lin.weight, lin.bias]
    return ps + [mlp.output_linear.weight, mlp.output_linear.bias]


def imap_query(params, p, oob_bound=None):
    """raw [P,4] float32 of the iMAP* decoder for points p [P,3] (float64); params = imap_params(mlp).

    oob_bound ([3,2] tensor): Renderer.eval_points' rule, raw[:,3] = 100 outside, no density gradient there."""
    p = p.reshape(-1, 3)
    if p.dtype != torch.float64:
        p = p.double()
    return _ImapQuery.apply(None if oob_bound is None else bound_list(oob_bound), None, p, *params)


def imap_query_rays(params, rays_o, rays_d, z, oob_bound=None):
    """imap_query at the points rays_o + rays_d * z (float64) formed inside the kernel; forward only (the
    differentiable path passes points, so that autograd carries the rays)."""
    with torch.no_grad():
        return _ImapQuery.apply(None if oob_bound is None else bound_list(oob_bound), (rays_o, rays_d, z), None,
                                *params)
