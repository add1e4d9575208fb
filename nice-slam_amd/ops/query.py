"""The fused point query of csrc/nslam_query.hip: NICE.forward and one decoder alone, forward and backward."""
import ctypes
import math
import sys

import torch

from . import span
from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from ..packing import xyz_layout
from ._check import bound_list
from .grid import channels_last

_ops = sys.modules[__package__]  # the package, whose SPLIT_FWD switch query_fwd_launch reads at call time


DEC_FOR_STAGE = {
    "coarse": ("coarse",),
    "middle": ("middle",),
    "fine": ("middle", "fine"),
    "color": ("middle", "fine", "color"),
}
DEC_ID = {"coarse": _lib.DEC_COARSE, "middle": _lib.DEC_MIDDLE, "fine": _lib.DEC_FINE, "color": _lib.DEC_COLOR}
_GRID_KEYS = ("grid_coarse", "grid_middle", "grid_fine", "grid_color")


class QueryMeta:
    """Non-tensor configuration of one query call."""

    def __init__(self, stage, decs, packers, dec_bounds, oob_bound, n_params):
        self.stage = stage
        self.decs = decs                # tuple of decoder names used by the stage
        self.packers = packers          # name → DecoderPacker
        self.dec_bounds = dec_bounds    # name → ([lo]*3, [hi]*3) normalisation bound
        self.oob_bound = oob_bound      # ([lo]*3, [hi]*3) or None (= no OOB test)
        self.n_params = n_params        # name → number of parameter tensors


def fill_cfg(meta, grids, packed, dgrads, need_pts_grad):
    cfg = _lib.NslamQueryCfg()
    cfg.stage = _lib.STAGES[meta.stage]
    cfg.need_pts_grad = int(bool(need_pts_grad))
    if meta.oob_bound is None:
        lo, hi = [-math.inf] * 3, [math.inf] * 3
    else:
        lo, hi = meta.oob_bound
    for k in range(3):
        cfg.bound_lo[k], cfg.bound_hi[k] = lo[k], hi[k]
    for name in meta.decs:
        d = DEC_ID[name]
        g, gg = grids[d][:2]
        slot = grids[d][2] if len(grids[d]) > 2 else None
        cfg.grid[d].data = g.data_ptr()
        cfg.grid[d].grad = gg.data_ptr() if gg is not None else None
        cfg.grid[d].slot = slot.data_ptr() if slot is not None else None
        cfg.grid[d].dims[0], cfg.grid[d].dims[1], cfg.grid[d].dims[2] = g.shape[2], g.shape[3], g.shape[4]
        blo, bhi = meta.dec_bounds[name]
        for k in range(3):
            cfg.grid[d].lo[k], cfg.grid[d].hi[k] = blo[k], bhi[k]
        cfg.packed[d] = packed[name].data_ptr()
        cfg.dgrad[d] = meta.packers[name].grad_struct(dgrads.get(name))
    # the fine decoder also reads the middle grid (no gradient through it)
    if "fine" in meta.decs and "middle" not in meta.decs:
        raise ValueError("fine stage needs the middle decoder/grid")
    return cfg


class _Query(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, pts, g_coarse, g_middle, g_fine, g_color, *params):
        pts = pts.detach().to(torch.float64).contiguous()
        grids_in = (g_coarse, g_middle, g_fine, g_color)
        grids = [channels_last(g.detach()) if g is not None else None for g in grids_in]
        packed, off = {}, 0
        for name in meta.decs:
            n = meta.n_params[name]
            packed[name] = meta.packers[name].pack(params[off:off + n])
            off += n
        raw = torch.empty(pts.shape[0], 4, dtype=torch.float32, device=pts.device)
        cfg = fill_cfg(meta, [(g, None) if g is not None else (None, None) for g in grids], packed, {}, False)
        saved = tape = None
        if any(ctx.needs_input_grad):  # ReLU masks for the backward (grad mode is off inside forward)
            saved = torch.empty(lib().nslam_query_saved_size(pts.shape[0]), dtype=torch.uint8, device=pts.device)
            cfg.saved_masks = saved.data_ptr()
            if meta.stage == "color":  # colour weight gradients read the activation tape (ABI v9)
                first = 6 + sum(meta.n_params[n] for n in meta.decs[:meta.decs.index("color")])
                if any(ctx.needs_input_grad[first:first + meta.n_params["color"]]):
                    tape = torch.empty(lib().nslam_query_tape_size(pts.shape[0]) // 4, dtype=torch.float32,
                                       device=pts.device)
                    cfg.act_tape = tape.data_ptr()
        query_fwd_launch(cfg, pts, pts.shape[0], raw)
        ctx.meta = meta
        ctx.packed = packed
        ctx.grids = grids
        ctx.saved_masks = saved
        ctx.tape = tape
        ctx.save_for_backward(pts)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        meta = ctx.meta
        (pts,) = ctx.saved_tensors
        g_raw = g_raw.contiguous().float()
        need = ctx.needs_input_grad
        need_pts = bool(need[1])
        grid_grads = [None] * 4
        pairs = []
        for d in range(4):
            g = ctx.grids[d]
            if g is not None and need[2 + d]:
                grid_grads[d] = torch.zeros_like(g, memory_format=torch.channels_last_3d)
            pairs.append((g, grid_grads[d]) if g is not None else (None, None))
        dgrads, off, pidx = {}, 0, 6
        for name in meta.decs:
            n = meta.n_params[name]
            if any(need[pidx + off + i] for i in range(n)):
                dgrads[name] = torch.zeros(meta.packers[name].n_params, dtype=torch.float32, device=pts.device)
            off += n
        g_pts = torch.empty_like(pts) if need_pts else None
        cfg = fill_cfg(meta, pairs, ctx.packed, dgrads, need_pts)
        if ctx.saved_masks is not None:
            cfg.saved_masks = ctx.saved_masks.data_ptr()
        if ctx.tape is not None:
            cfg.act_tape = ctx.tape.data_ptr()
        wsb = lib().nslam_query_bwd_workspace_size(ctypes.byref(cfg), pts.shape[0])
        ws = torch.empty(wsb, dtype=torch.uint8, device=pts.device) if wsb else None
        with span("query_bwd"):
            rc = lib().nslam_query_bwd(ctypes.byref(cfg), ptr(pts), pts.shape[0], ptr(g_raw), ptr(g_pts), ptr(ws),
                                       wsb, stream_ptr(pts.device))
        check(rc, "nslam_query_bwd")
        out = [None, g_pts] + grid_grads
        for name in meta.decs:
            n = meta.n_params[name]
            if name in dgrads:
                out += meta.packers[name].split_grad(dgrads[name])
            else:
                out += [None] * n
        return tuple(out)


def query_points(nice, p, c_grid, stage, oob_bound=None):
    """raw [P,4] for points p [P,3] (float64) — NICE.forward (+ eval_points' OOB rule)."""
    if stage not in DEC_FOR_STAGE:
        raise ValueError(f"unknown stage {stage!r}")
    decs = DEC_FOR_STAGE[stage]
    packers, bounds, nparams, params = {}, {}, {}, []
    for name in decs:
        dec = nice.decoder(name)
        packers[name] = dec.packer()
        bounds[name] = bound_list(dec.bound)
        plist = list(dec.parameters())
        nparams[name] = len(plist)
        params += plist
    meta = QueryMeta(stage, decs, packers, bounds, None if oob_bound is None else bound_list(oob_bound), nparams)
    grids = []
    for d, key in enumerate(_GRID_KEYS):
        used = (d == _lib.DEC_COARSE and stage == "coarse") or (d == _lib.DEC_MIDDLE and stage != "coarse") or \
               (d == _lib.DEC_FINE and stage in ("fine", "color")) or (d == _lib.DEC_COLOR and stage == "color")
        grids.append(c_grid[key] if used else None)
    p = p.reshape(-1, 3)
    if p.dtype != torch.float64:
        p = p.double()
    return _Query.apply(meta, p, *grids, *params)


_ZERO_PACKED = {}


class _Stub:
    """Stands in for a decoder the kernel's stage evaluates beside the one asked for (its output is
    discarded): all-zero packed weights, no parameters, no gradient."""

    def __init__(self, nc, device):
        key = (nc, str(device))
        if key not in _ZERO_PACKED:
            _ZERO_PACKED[key] = torch.zeros(xyz_layout(nc)["total"], dtype=torch.float32, device=device)
        self.packed = _ZERO_PACKED[key]

    def pack(self, params):
        return self.packed

    def grad_struct(self, base):
        return _lib.NslamDecGrad()


class _OneDecoder(torch.autograd.Function):
    """The fine or colour decoder evaluated alone, through the stage that holds it (fine: middle |
    fine, colour: middle | fine | colour) with the other decoders as zero stubs: the fine
    occupancy comes from the forward's deferred-combine mode (raw[...,3] = fine only), the colour
    decoder's rgb from raw[..., :3], and its 4th output row (which NICE.forward overwrites,
    decoder.py:341) from the forward's activation tape h4 (returned as a second output so torch
    forms h4 @ Wo[3] + bo[3]).  Backward: that decoder's share only (nslam_query_bwd_decoder); the
    cotangent torch forms for h4 (the 4th row's Wo[3] g) enters the kernels' Woᵀg as
    nslam_query_cfg.g_h4 (ABI v17), so it reaches the hidden layers, the grid and the points."""

    @staticmethod
    def forward(ctx, meta, name, pts, g_own, g_middle, *params):
        ctx.set_materialize_grads(False)
        pts = pts.detach().to(torch.float64).contiguous()
        n = pts.shape[0]
        own = channels_last(g_own.detach())
        mid = channels_last(g_middle.detach()) if g_middle is not None else own
        d = DEC_ID[name]
        grids = [None] * 4
        grids[_lib.DEC_MIDDLE] = (mid, None)
        grids[_lib.DEC_FINE] = (own if name == "fine" else mid, None)
        grids[d] = (own, None)
        packed = {k: meta.packers[k].pack(params if k == name else ()) for k in meta.decs}
        cfg = fill_cfg(meta, grids, packed, {}, False)
        raw = torch.empty(n, 4, dtype=torch.float32, device=pts.device)
        saved = torch.empty(lib().nslam_query_saved_size(n), dtype=torch.uint8, device=pts.device)
        cfg.saved_masks = saved.data_ptr()
        tape = None
        if name == "color":
            tape = torch.empty(lib().nslam_query_tape_size(n) // 4, dtype=torch.float32, device=pts.device)
            cfg.act_tape = tape.data_ptr()
        if n:
            query_fwd_launch(cfg, pts, n, raw, split=True, defer_occ=name == "fine")
        ctx.meta, ctx.name, ctx.grids, ctx.packed = meta, name, grids, packed
        ctx.saved_masks, ctx.tape = saved, tape
        ctx.save_for_backward(pts)
        if name == "fine":
            return raw[:, 3].clone(), None
        # h4 of point i: tape [tile][layer][32 points][32 features], layer 4 (nslam.h act_tape)
        h4 = tape.view(-1, 5, 32, 32)[:, 4].reshape(-1, 32)[:n].clone()
        return raw[:, :3].clone(), h4

    @staticmethod
    def backward(ctx, g_out, g_h4):
        meta, name = ctx.meta, ctx.name
        (pts,) = ctx.saved_tensors
        need = ctx.needs_input_grad
        n = pts.shape[0]
        d = DEC_ID[name]
        g_raw = torch.zeros(n, 4, dtype=torch.float32, device=pts.device)
        if g_out is not None:
            if name == "fine":
                g_raw[:, 3] = g_out
            else:
                g_raw[:, :3] = g_out
        grids = list(ctx.grids)
        own = grids[d][0]
        g_grid = torch.zeros_like(own, memory_format=torch.channels_last_3d) if need[3] else None
        grids[d] = (own, g_grid)
        dgrad = torch.zeros(meta.packers[name].n_params, dtype=torch.float32, device=pts.device) \
            if any(need[5:]) else None
        g_pts = torch.empty_like(pts) if need[2] else None
        cfg = fill_cfg(meta, grids, ctx.packed, {name: dgrad} if dgrad is not None else {}, need[2])
        cfg.saved_masks = ctx.saved_masks.data_ptr()
        if ctx.tape is not None:
            cfg.act_tape = ctx.tape.data_ptr()
        if g_h4 is not None:  # d/dh4 of the 4th output row (decoder.py:198-203), [n, 32] float32
            g_h4 = g_h4.detach().to(torch.float32).contiguous()
            cfg.g_h4 = g_h4.data_ptr()
        if n and (g_grid is not None or dgrad is not None or g_pts is not None):
            wsb = lib().nslam_query_bwd_decoder_workspace_size(ctypes.byref(cfg), d, n)
            ws = torch.empty(wsb, dtype=torch.uint8, device=pts.device) if wsb else None
            rc = lib().nslam_query_bwd_decoder(ctypes.byref(cfg), d, 0, ptr(pts), n, ptr(g_raw), ptr(g_pts),
                                               ptr(ws), wsb, stream_ptr(pts.device))
            check(rc, "nslam_query_bwd_decoder")
        elif g_pts is not None:
            g_pts.zero_()
        grads = meta.packers[name].split_grad(dgrad) if dgrad is not None else [None] * meta.n_params[name]
        return (None, None, g_pts, g_grid, None, *grads)


def query_decoder(dec, p, c_grid):
    """One decoder's forward (MLP.forward / MLP_no_xyz.forward): coarse [P], middle [P], fine [P]
    (occupancy, out.squeeze(-1)), colour [P, 4] — the reference module's output for p [P, 3]."""
    name = dec.name
    p = p.reshape(-1, 3)
    if p.dtype != torch.float64:
        p = p.double()
    bl = bound_list(dec.bound)
    params = list(dec.parameters())
    if name in ("coarse", "middle"):
        meta = QueryMeta(name, (name,), {name: dec.packer()}, {name: bl}, None, {name: len(params)})
        grids = [None] * 4
        grids[DEC_ID[name]] = c_grid["grid_" + name]
        return _Query.apply(meta, p, *grids, *params)[:, 3]
    stage = name
    decs = DEC_FOR_STAGE[stage]
    packers = {k: (dec.packer() if k == name else _Stub(2 if k == "fine" else 1, p.device)) for k in decs}
    meta = QueryMeta(stage, decs, packers, {k: bl for k in decs}, None, {k: (len(params) if k == name else 0)
                                                                          for k in decs})
    own = c_grid["grid_" + name]
    out, h4 = _OneDecoder.apply(meta, name, p, own, c_grid.get("grid_middle"), *params)
    if name == "fine":
        return out
    W, b = dec.output_linear.weight, dec.output_linear.bias
    return torch.cat([out, (h4 @ W[3] + b[3])[:, None]], 1)


def query_fwd_launch(cfg, pts, n, raw, split=None, defer_occ=False):
    """nslam_query_fwd_ws (decoder-parallel) or nslam_query_fwd (one fused chain per wave).

    defer_occ: leave raw[...,3] = the fine occupancy and return the middle occupancy [n] float
    (or None when the stage has no split) for render_loss(occ_add=...) to add on read."""
    split = _ops.SPLIT_FWD if split is None else split
    wsb = lib().nslam_query_fwd_workspace_size(ctypes.byref(cfg), n) if split else 0
    occ = None
    with span("query_fwd"):
        if wsb:
            ws = torch.empty(wsb, dtype=torch.uint8, device=raw.device)
            cfg.defer_occ = int(bool(defer_occ))
            rc = lib().nslam_query_fwd_ws(ctypes.byref(cfg), ptr(pts), n, ptr(raw), ptr(ws), wsb,
                                          stream_ptr(raw.device))
            cfg.defer_occ = 0
            if defer_occ:
                occ = ws[:n * 4].view(torch.float32)
        else:
            rc = lib().nslam_query_fwd(ctypes.byref(cfg), ptr(pts), n, ptr(raw), stream_ptr(raw.device))
    check(rc, "nslam_query_fwd")
    return occ
