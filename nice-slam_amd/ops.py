"""torch.autograd operators over libnslam.so (HIP, gfx950).  No CPU fallback.

  sample_z        — Renderer.render_batch_ray's sampler (src/utils/Renderer.py:82-170), no grad
  query_points    — NICE.forward + eval_points (decoder.py:168-342, Renderer.py:23-61), fwd+bwd
  composite       — raw2outputs_nerf_color (src/common.py:204-245, occupancy), fwd+bwd
  grid_sample     — F.grid_sample(bilinear, border, align_corners=True) on a channels-last grid
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import math

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

class KernelTimer:
    """Optional live timing of the C-ABI launches with HIP events on the launching stream.

    ops.TIMER = KernelTimer() turns it on (bench.py does, for the timed region only); each entry
    point records an event pair around its launches; summary() synchronises and averages.
    """

    def __init__(self):
        self.events = {}

    def span(self, name):
        return _Span(self, name)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, pairs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in pairs]
            out[name] = {"calls": len(ms), "avg_ms": sum(ms) / max(len(ms), 1), "total_ms": sum(ms)}
        return out


class _Span:
    def __init__(self, timer, name):
        self.timer, self.name = timer, name

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()
        return self

    def __exit__(self, *exc):
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.timer.events.setdefault(self.name, []).append((self.a, b))
        return False


class _NoSpan:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


TIMER = None
_NOSPAN = _NoSpan()


def _span(name):
    return TIMER.span(name) if TIMER is not None else _NOSPAN


@contextlib.contextmanager
def capture(graph):
    """torch.cuda.graph(graph) with the garbage collector out of the way.  torch no longer collects before
    a capture, and an automatic collection inside one may free a dead cycle's device objects (an older
    graph, tensors of its pool) from the capturing thread, which the runtime does not allow while a stream
    captures: the process aborts.  So dead cycles are collected first and none is collected inside."""
    gc.collect()
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            yield
    finally:
        if enabled:
            gc.enable()


_DEC_FOR_STAGE = {
    "coarse": ("coarse",),
    "middle": ("middle",),
    "fine": ("middle", "fine"),
    "color": ("middle", "fine", "color"),
}
_DEC_ID = {"coarse": _lib.DEC_COARSE, "middle": _lib.DEC_MIDDLE, "fine": _lib.DEC_FINE, "color": _lib.DEC_COLOR}
_GRID_KEYS = ("grid_coarse", "grid_middle", "grid_fine", "grid_color")


def channels_last(g: torch.Tensor) -> torch.Tensor:
    """[1,C,Z,Y,X] grid as physically [Z][Y][X][C] (no copy when it already is)."""
    if g.dim() != 5 or g.shape[0] != 1 or g.shape[1] != 32:
        raise ValueError(f"feature grid must be [1,32,Z,Y,X], got {tuple(g.shape)}")
    if g.dtype != torch.float32:
        raise ValueError("feature grids are float32")
    if not g.is_contiguous(memory_format=torch.channels_last_3d):
        g = g.contiguous(memory_format=torch.channels_last_3d)
    return g


def _bound_list(b):
    b = b.detach().to("cpu", torch.float64)
    return [float(v) for v in b[:, 0]], [float(v) for v in b[:, 1]]


# ----------------------------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------------------------
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
    lo, hi = _bound_list(bound)
    L = lib()
    wsb = L.nslam_workspace_size(0, n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=ro.device)
    with _span("sample_rays"):
        gm = gt_max.detach().float().reshape(1).contiguous() if (gt_max is not None and gt is not None) else None
        rc = L.nslam_sample_rays(ptr(ro), ptr(rd), ptr(gt), ptr(gm), n, (ctypes.c_double * 3)(*lo),
                                 (ctypes.c_double * 3)(*hi), ptr(ts), n_strat, ptr(tu), s1, int(bool(lindisp)),
                                 ptr(z), ptr(ws), wsb, stream_ptr(ro.device))
    check(rc, "nslam_sample_rays")
    return z


# ----------------------------------------------------------------------------------------------
# fused point query
# ----------------------------------------------------------------------------------------------
class QueryMeta:
    """Non-tensor configuration of one query call."""

    def __init__(self, stage, decs, packers, dec_bounds, oob_bound, n_params):
        self.stage = stage
        self.decs = decs                # tuple of decoder names used by the stage
        self.packers = packers          # name → DecoderPacker
        self.dec_bounds = dec_bounds    # name → ([lo]*3, [hi]*3) normalisation bound
        self.oob_bound = oob_bound      # ([lo]*3, [hi]*3) or None (= no OOB test)
        self.n_params = n_params        # name → number of parameter tensors


def _fill_cfg(meta, grids, packed, dgrads, need_pts_grad):
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
        d = _DEC_ID[name]
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
        cfg = _fill_cfg(meta, [(g, None) if g is not None else (None, None) for g in grids], packed, {}, False)
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
        cfg = _fill_cfg(meta, pairs, ctx.packed, dgrads, need_pts)
        if ctx.saved_masks is not None:
            cfg.saved_masks = ctx.saved_masks.data_ptr()
        if ctx.tape is not None:
            cfg.act_tape = ctx.tape.data_ptr()
        wsb = lib().nslam_query_bwd_workspace_size(ctypes.byref(cfg), pts.shape[0])
        ws = torch.empty(wsb, dtype=torch.uint8, device=pts.device) if wsb else None
        with _span("query_bwd"):
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
    if stage not in _DEC_FOR_STAGE:
        raise ValueError(f"unknown stage {stage!r}")
    decs = _DEC_FOR_STAGE[stage]
    packers, bounds, nparams, params = {}, {}, {}, []
    for name in decs:
        dec = nice.decoder(name)
        packers[name] = dec.packer()
        bounds[name] = _bound_list(dec.bound)
        plist = list(dec.parameters())
        nparams[name] = len(plist)
        params += plist
    meta = QueryMeta(stage, decs, packers, bounds, None if oob_bound is None else _bound_list(oob_bound), nparams)
    grids = []
    for d, key in enumerate(_GRID_KEYS):
        used = (d == _lib.DEC_COARSE and stage == "coarse") or (d == _lib.DEC_MIDDLE and stage != "coarse") or \
               (d == _lib.DEC_FINE and stage in ("fine", "color")) or (d == _lib.DEC_COLOR and stage == "color")
        grids.append(c_grid[key] if used else None)
    p = p.reshape(-1, 3)
    if p.dtype != torch.float64:
        p = p.double()
    return _Query.apply(meta, p, *grids, *params)


# ----------------------------------------------------------------------------------------------
# one decoder alone: MLP.forward / MLP_no_xyz.forward (decoder.py:177-203, 262-274)
# ----------------------------------------------------------------------------------------------
_ZERO_PACKED = {}


class _Stub:
    """Stands in for a decoder the kernel's stage evaluates beside the one asked for (its output is
    discarded): all-zero packed weights, no parameters, no gradient."""

    def __init__(self, nc, device):
        from .packing import xyz_layout
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
        d = _DEC_ID[name]
        grids = [None] * 4
        grids[_lib.DEC_MIDDLE] = (mid, None)
        grids[_lib.DEC_FINE] = (own if name == "fine" else mid, None)
        grids[d] = (own, None)
        packed = {k: meta.packers[k].pack(params if k == name else ()) for k in meta.decs}
        cfg = _fill_cfg(meta, grids, packed, {}, False)
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
        d = _DEC_ID[name]
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
        cfg = _fill_cfg(meta, grids, ctx.packed, {name: dgrad} if dgrad is not None else {}, need[2])
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
    bl = _bound_list(dec.bound)
    params = list(dec.parameters())
    if name in ("coarse", "middle"):
        meta = QueryMeta(name, (name,), {name: dec.packer()}, {name: bl}, None, {name: len(params)})
        grids = [None] * 4
        grids[_DEC_ID[name]] = c_grid["grid_" + name]
        return _Query.apply(meta, p, *grids, *params)[:, 3]
    stage = name
    decs = _DEC_FOR_STAGE[stage]
    packers = {k: (dec.packer() if k == name else _Stub(2 if k == "fine" else 1, p.device)) for k in decs}
    meta = QueryMeta(stage, decs, packers, {k: bl for k in decs}, None, {k: (len(params) if k == name else 0)
                                                                          for k in decs})
    own = c_grid["grid_" + name]
    out, h4 = _OneDecoder.apply(meta, name, p, own, c_grid.get("grid_middle"), *params)
    if name == "fine":
        return out
    W, b = dec.output_linear.weight, dec.output_linear.bias
    return torch.cat([out, (h4 @ W[3] + b[3])[:, None]], 1)


# ----------------------------------------------------------------------------------------------
# compositing
# ----------------------------------------------------------------------------------------------
def _composite_call(which, raw, z, rd, tensors, last):
    """nslam_composite_<which>, or with rays_d nslam_composite_density_<which>: the same arguments plus rays_d
    after z and one more tensor (`last`) before the stream."""
    name = f"composite_{which}" if rd is None else f"composite_density_{which}"
    n, s = z.shape
    rays, extra = ((), ()) if rd is None else ((ptr(rd),), (ptr(last),))
    with _span(name):
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


# ----------------------------------------------------------------------------------------------
# standalone trilinear lookup
# ----------------------------------------------------------------------------------------------
class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, coords):
        g = channels_last(grid.detach())
        c = coords.detach().float().reshape(-1, 3).contiguous()
        out = torch.empty(c.shape[0], 32, dtype=torch.float32, device=c.device)
        dims = (ctypes.c_int32 * 3)(g.shape[2], g.shape[3], g.shape[4])
        if c.shape[0]:
            check(lib().nslam_grid_sample_fwd(ptr(g), dims, ptr(c), c.shape[0], ptr(out), stream_ptr(c.device)),
                  "nslam_grid_sample_fwd")
        ctx.save_for_backward(g, c)
        return out

    @staticmethod
    def backward(ctx, gout):
        g, c = ctx.saved_tensors
        gg = torch.zeros_like(g, memory_format=torch.channels_last_3d) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        dims = (ctypes.c_int32 * 3)(g.shape[2], g.shape[3], g.shape[4])
        if c.shape[0]:
            check(lib().nslam_grid_sample_bwd(ptr(g), dims, ptr(c), c.shape[0], ptr(gout.contiguous().float()),
                                              ptr(gg), ptr(gc), stream_ptr(c.device)), "nslam_grid_sample_bwd")
        return gg, gc


SPLIT_FWD = True  # decoder-parallel forward (nslam_query_fwd_ws); False: one wave runs every decoder


def query_fwd_launch(cfg, pts, n, raw, split=None, defer_occ=False):
    """nslam_query_fwd_ws (decoder-parallel) or nslam_query_fwd (one fused chain per wave).

    defer_occ: leave raw[...,3] = the fine occupancy and return the middle occupancy [n] float
    (or None when the stage has no split) for render_loss(occ_add=...) to add on read."""
    split = SPLIT_FWD if split is None else split
    wsb = lib().nslam_query_fwd_workspace_size(ctypes.byref(cfg), n) if split else 0
    occ = None
    with _span("query_fwd"):
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


def grid_sample_fwd(grid, coords, out):
    """nslam_grid_sample_fwd without autograd: out [M,32] = trilinear features of the normalised
    coords [M,3] in a channels-last grid (bench / bulk-query form; grid_sample() is the
    differentiable drop-in)."""
    if not grid.is_contiguous(memory_format=torch.channels_last_3d):
        raise ValueError("grid must be channels-last")
    dims = (ctypes.c_int32 * 3)(grid.shape[2], grid.shape[3], grid.shape[4])
    with _span("grid_fwd"):
        rc = lib().nslam_grid_sample_fwd(ptr(grid), dims, ptr(coords), coords.shape[0], ptr(out),
                                         stream_ptr(coords.device))
    check(rc, "nslam_grid_sample_fwd")


def grid_sample_bwd(grid, coords, gout, ggrid, gcoords=None):
    """nslam_grid_sample_bwd without autograd: ggrid += scatter of gout (atomics); gcoords = d/dcoords."""
    dims = (ctypes.c_int32 * 3)(grid.shape[2], grid.shape[3], grid.shape[4])
    with _span("grid_bwd"):
        rc = lib().nslam_grid_sample_bwd(ptr(grid), dims, ptr(coords), coords.shape[0], ptr(gout), ptr(ggrid),
                                         ptr(gcoords), stream_ptr(coords.device))
    check(rc, "nslam_grid_sample_bwd")


def grid_sample(grid, coords):
    """[M,32] trilinear features of normalised coords [M,3] (x,y,z) — F.grid_sample semantics."""
    return _GridSample.apply(grid, coords)


# ----------------------------------------------------------------------------------------------
# fused mapping / tracking iteration (ABI v4): pixel gather, render loss, ray-form query, Adam
# ----------------------------------------------------------------------------------------------
def gather_rays(frames, pix, n_per, H, W, window, fx, fy, cx, cy, bound=None, draw=None, n_kept=None, out=None):
    """get_samples (src/common.py:92-134) for every frame of a window in one launch, plus the
    inside-mask prefilter (Mapper.py:469-481) when `bound` is given.

    frames: list of (depth [H,W] f32, color [H,W,3] f32, c2w [3|4,4] f32) device tensors, or of
    (depth, color, c2w_out [3|4,4] f32, cam [7] f32): the pose formed in the kernel from the camera
    7-vector (nslam_cam_pose's values) and written to c2w_out's first three rows (ABI v21);
    pix: int64 [len(frames)*n_per] select_uv randint indices into each frame's window
    (h0, h1, w0, w1).  Returns rays_o, rays_d [N,3] f32, gt_depth [N] f32 (0 for dropped rays),
    gt_color [N,3] f32, keep [N] uint8.
    pix=None: draw the pixels on the device (`draw`: PixelDraws, ABI v7); n_kept: optional device
    int64 [1] incremented by the number of kept rays; out: optional preallocated
    (rays_o, rays_d, gt_depth, gt_color, keep) to write into.
    """
    nf = len(frames)
    if nf == 0 or nf > _lib.MAX_FRAMES:
        raise ValueError(f"1..{_lib.MAX_FRAMES} frames, got {nf}")
    if pix is None and draw is None:
        raise ValueError("pix or draw")
    dev = pix.device if pix is not None else draw.counter.device
    arr = (_lib.NslamFrame * nf)()
    keepalive = []
    for f, fr in enumerate(frames):
        d, c, m = fr[:3]
        cam = fr[3] if len(fr) > 3 else None
        d = d.detach().float().contiguous()
        c = c.detach().float().contiguous()
        if cam is None:
            m = m.detach().float().contiguous()
        elif m.dtype != torch.float32 or not m.is_contiguous() or cam.dtype != torch.float32 \
                or not cam.is_contiguous() or cam.numel() != 7:
            raise ValueError("a frame given by its camera: c2w_out contiguous f32 [3|4,4], cam contiguous f32 [7]")
        if tuple(d.shape) != (H, W) or tuple(c.shape) != (H, W, 3) or m.shape[-1] != 4 or m.shape[0] < 3:
            raise ValueError("frame tensors must be depth [H,W], color [H,W,3], c2w [3|4,4]")
        keepalive += [d, c, m]
        arr[f].depth, arr[f].color = ptr(d), ptr(c)
        if cam is None:
            arr[f].c2w = ptr(m)
        else:
            arr[f].cam, arr[f].c2w_out = ptr(cam.detach()), ptr(m)
    if pix is not None:
        pix = pix.to(torch.int64).contiguous()
    n = nf * n_per
    if out is not None:
        ro, rd, gd, gc, keep = out
        want = ((n, 3, torch.float32), (n, 3, torch.float32), (n, torch.float32), (n, 3, torch.float32),
                (n, torch.uint8))
        for t, w in zip(out, want):
            if tuple(t.shape) != tuple(w[:-1]) or t.dtype != w[-1] or not t.is_contiguous():
                raise ValueError("out tensors must match gather_rays' outputs")
    else:
        ro = torch.empty(n, 3, dtype=torch.float32, device=dev)
        rd = torch.empty(n, 3, dtype=torch.float32, device=dev)
        gd = torch.empty(n, dtype=torch.float32, device=dev)
        gc = torch.empty(n, 3, dtype=torch.float32, device=dev)
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
    h0, h1, w0, w1 = window
    if bound is not None:
        lo, hi = _bound_list(bound)
        blo, bhi = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*hi)
    else:
        blo = bhi = None
    with _span("gather_rays"):
        rc = lib().nslam_gather_rays(arr, nf, n_per, ptr(pix), H, W, h0, h1, w0, w1, fx, fy, cx, cy, blo, bhi,
                                     ptr(ro), ptr(rd), ptr(gd), ptr(gc), ptr(keep),
                                     ctypes.byref(draw.struct) if (pix is None) else None,
                                     ptr(n_kept) if n_kept is not None else None, stream_ptr(dev))
    check(rc, "nslam_gather_rays")
    return ro, rd, gd, gc, keep


class PixelDraws:
    """Device state of in-kernel pixel draws (nslam_draw, ABI v7): a seed and a device draw
    counter the gather kernel advances itself — no host RNG work per (graph-replayed) call.
    Uniform over the window like select_uv's torch.randint (common.py:113-134), but a different
    stream (counter-based splitmix64), so draws do not reproduce torch's sequence.

    Ray sharding (world > 1): every rank passes the same seed; the global batch holds
    n_per * world pixels per frame and this rank gathers slots [rank*n_per, (rank+1)*n_per) of
    each frame.  with_max: the kernel also leaves max(gt_depth) over the kept rays of the WHOLE
    global batch in self.gt_max (each rank re-draws the other ranks' slots) — the sampler's
    batch-global scalar (Renderer.py:107-111,144) without an all-reduce."""

    def __init__(self, seed, device, world=1, rank=0, with_max=False):
        if not (world >= 1 and 0 <= rank < world):
            raise ValueError(f"rank {rank} of world {world}")
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)
        self.world, self.rank = int(world), int(rank)
        self.gt_max = torch.zeros(1, dtype=torch.float32, device=device) if with_max else None
        self.key = torch.zeros(1, dtype=torch.int32, device=device) if with_max else None
        self.struct = _lib.NslamDraw(int(seed) & (2 ** 64 - 1), ptr(self.counter), ptr(self.ticket), self.world,
                                     self.rank, ptr(self.gt_max), ptr(self.key))


CAM_GRAD_WS_DOUBLES = 32 * 12  # NSLAM_CAM_GRAD_WS_DOUBLES


def _expect(fn, specs, msg=None):
    """Every (tensor, dtype, shape) of specs is a contiguous tensor of exactly that dtype and shape, else
    ValueError (fn: the caller's name; msg: its own wording instead of the expected / got line)."""
    for t, dt, shp in specs:
        if t.dtype != dt or tuple(t.shape) != tuple(shp) or not t.is_contiguous():
            raise ValueError(f"{fn}: " + (msg or f"expected contiguous {dt} {shp}, got {t.dtype} {tuple(t.shape)}"))


def cam_pose(cam, out):
    """nslam_cam_pose (ABI v8): out [3,4] f32 = get_camera_from_tensor(cam [7]) in one launch."""
    _expect("cam_pose", [(cam, torch.float32, (7,))], "cam must be a contiguous float32 [7]")
    _expect("cam_pose", [(out, torch.float32, (3, 4))], "out must be a contiguous float32 [3, 4]")
    check(lib().nslam_cam_pose(ptr(cam), ptr(out), stream_ptr(cam.device)), "nslam_cam_pose")
    return out


def cam_grad(cam, c2w, g_pts, z, rd, out):
    """nslam_cam_grad (ABI v8): out [7] f32 = d loss / d cam through pts = t + (R·dir)·z and
    get_camera_from_tensor (Renderer.py:172-174, common.py:137-176), from g_pts [N*S,3] f64,
    z [N,S] f64, rays_d [N,3] f32 and the c2w [3,4] f32 the rays were built with."""
    n, S = z.shape
    _expect("cam_grad", [(cam, torch.float32, (7,)), (c2w, torch.float32, (3, 4)), (g_pts, torch.float64, (n * S, 3)),
                         (z, torch.float64, (n, S)), (rd, torch.float32, (n, 3)), (out, torch.float32, (7,))])
    with _span("cam_grad"):
        rc = lib().nslam_cam_grad(ptr(cam), ptr(c2w), ptr(g_pts), ptr(z), ptr(rd), n, S, ptr(out), stream_ptr(cam.device))
    check(rc, "nslam_cam_grad")
    return out


def cam_grad_parts(cam, c2w, g_pts, z, rd, out, ws, ticket):
    """nslam_cam_grad_parts (ABI v15): cam_grad from the per-decoder d/dpts buffers g_pts (list of
    [N*S,3] f64, summed per point in list order inside the kernel) over several workgroups; ws: f64
    [NSLAM_CAM_GRAD_WS_DOUBLES], ticket: int32 [1] zeroed once (both persistent, one per caller)."""
    n, S = z.shape
    _expect("cam_grad_parts", [(cam, torch.float32, (7,)), (c2w, torch.float32, (3, 4)), (z, torch.float64, (n, S)),
                               (rd, torch.float32, (n, 3)), (out, torch.float32, (7,)),
                               (ws, torch.float64, (CAM_GRAD_WS_DOUBLES,)), (ticket, torch.int32, (1,))] +
            [(g, torch.float64, (n * S, 3)) for g in g_pts])
    bufs = (ctypes.c_void_p * len(g_pts))(*[ptr(g) for g in g_pts])
    with _span("cam_grad"):
        rc = lib().nslam_cam_grad_parts(ptr(cam), ptr(c2w), bufs, len(g_pts), ptr(z), ptr(rd), n, S, ptr(out), ptr(ws),
                                        ptr(ticket), stream_ptr(cam.device))
    check(rc, "nslam_cam_grad_parts")
    return out


def cam_grad_step(cam, c2w, g_pts, z, rd, g_cam, ws, ticket, adam, ray_loss, loss_out, best_loss=None, best=None,
                  lr_quat=None, best_before_step=False):
    """nslam_cam_grad_step (ABI v23): cam_grad_parts, then in its last workgroup the camera's Adam step in
    place (adam = (exp_avg [7], exp_avg_sq [7], step [1], lr, beta1, beta2, eps)), loss_out = the fixed-order
    sum of ray_loss and, with best_loss / best, the best-pose update — bit-identical to cam_grad_parts +
    FusedAdam.step + loss_sum_best, in one launch.
    lr_quat (a rate for elements 0..3) or best_before_step (best = the camera before the step) select
    nslam_cam_grad_step_lr2, the reference's seperate_LR loop (Tracker.py:202-247) on the same kernel."""
    n, S = z.shape
    ex, ex2, stp, lr, b1, b2, eps = adam
    checks = [(cam, torch.float32, (7,)), (c2w, torch.float32, (3, 4)), (z, torch.float64, (n, S)),
              (rd, torch.float32, (n, 3)), (g_cam, torch.float32, (7,)), (ws, torch.float64, (CAM_GRAD_WS_DOUBLES,)),
              (ticket, torch.int32, (1,)), (ex, torch.float32, (7,)), (ex2, torch.float32, (7,)),
              (stp, torch.float32, (1,)), (ray_loss, torch.float64, (ray_loss.numel(),)),
              (loss_out, torch.float64, ())]
    if best_loss is not None:
        checks += [(best_loss, torch.float64, ()), (best, torch.float32, (7,))]
    _expect("cam_grad_step", checks + [(g, torch.float64, (n * S, 3)) for g in g_pts])
    tail = _lib.NslamCamTail(ptr(cam), ptr(ex), ptr(ex2), ptr(stp), float(lr), float(b1), float(b2), float(eps),
                             ptr(ray_loss), ray_loss.numel(), ptr(loss_out), ptr(best_loss), ptr(best))
    bufs = (ctypes.c_void_p * len(g_pts))(*[ptr(g) for g in g_pts])
    fn, name = lib().nslam_cam_grad_step, "nslam_cam_grad_step"
    if lr_quat is not None or best_before_step:
        tail = _lib.NslamCamTailLr2(tail, float(lr if lr_quat is None else lr_quat), int(bool(best_before_step)))
        fn, name = lib().nslam_cam_grad_step_lr2, "nslam_cam_grad_step_lr2"
    with _span("cam_grad"):
        rc = fn(ctypes.byref(tail), ptr(c2w), bufs, len(g_pts), ptr(z), ptr(rd), n, S, ptr(g_cam), ptr(ws),
                ptr(ticket), stream_ptr(cam.device))
    check(rc, name)
    return loss_out


def undistort_u8(src, fx, fy, cx, cy, dist, out=None):
    """nslam_undistort_u8: cv2.undistort(src, K, dist) with its defaults (new camera matrix K, bilinear,
    zero border; 1/32-pixel positions, integer weights — include/nslam.h) for a contiguous uint8 device image
    [H, W, C] or [H, W], C in 1..4, and dist = (k1, k2, p1, p2, k3).  One launch on the current stream, no
    host synchronisation.  Returns a new image (or `out`, which may not be src)."""
    if src.dtype != torch.uint8 or src.dim() not in (2, 3) or not src.is_contiguous():
        raise ValueError("undistort_u8: src must be a contiguous uint8 [H, W] or [H, W, C]")
    C = 1 if src.dim() == 2 else src.shape[2]
    dist = [float(v) for v in dist]
    if len(dist) != 5:
        raise ValueError(f"undistort_u8: dist must be (k1, k2, p1, p2, k3), got {len(dist)} coefficients")
    if not 1 <= C <= 4:
        raise ValueError(f"undistort_u8: 1..4 channels, got {C}")
    if out is None:
        out = torch.empty_like(src)
    _expect("undistort_u8", [(out, torch.uint8, src.shape)])
    if out.data_ptr() == src.data_ptr() and src.numel():
        raise ValueError("undistort_u8: out may not alias src")
    if src.numel() == 0:
        return out
    rc = lib().nslam_undistort_u8(ptr(src), src.shape[0], src.shape[1], C, float(fx), float(fy), float(cx), float(cy),
                                  (ctypes.c_double * 5)(*dist), ptr(out), stream_ptr(src.device))
    check(rc, "nslam_undistort_u8")
    return out


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
    rc =lib().nslam_vis_panels(ptr(gt_depth), ptr(gt_color), ptr(depth), ptr(color), H, W, ptr(vmax), ptr(out),
                                stream_ptr(gt_depth.device))
    check(rc, "nslam_vis_panels")
    return out


def cam_vector_batch(c2w, out, copy=None):
    """nslam_cam_vector_batch (ABI v22): out[k] = get_tensor_from_camera(c2w[k]) for c2w [n, 3|4, 4] f32
    (common.camera_tensors' arithmetic, one launch); copy: optional second [n, 7] f32 receiving the same."""
    n = c2w.shape[0]
    if c2w.dtype != torch.float32 or c2w.dim() != 3 or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4 \
            or not c2w.is_contiguous() or not 1 <= n <= 64:
        raise ValueError("cam_vector_batch: c2w must be a contiguous float32 [n, 3|4, 4], 1 <= n <= 64")
    _expect("cam_vector_batch", [(t, torch.float32, (n, 7)) for t in ((out,) if copy is None else (out, copy))],
            "out / copy must be contiguous float32 [n, 7]")
    rc = lib().nslam_cam_vector_batch(ptr(c2w), c2w.shape[1] * 4, n, ptr(out), None if copy is None else ptr(copy),
                                      stream_ptr(c2w.device))
    check(rc, "nslam_cam_vector_batch")
    return out


def cam_pose_batch(cams, c2w):
    """nslam_cam_pose_batch (ABI v19): c2w[k, :3, :4] = get_camera_from_tensor(cams[k]) for cams [n, 7] f32
    and c2w [n, 3 or 4, 4] f32 (both contiguous), one launch."""
    n = cams.shape[0]
    _expect("cam_pose_batch", [(cams, torch.float32, (n, 7))], "cams must be a contiguous float32 [n, 7]")
    if (c2w.dtype != torch.float32 or c2w.dim() != 3 or c2w.shape[0] != n or c2w.shape[1] not in (3, 4)
            or c2w.shape[2] != 4 or not c2w.is_contiguous()):
        raise ValueError("cam_pose_batch: c2w must be a contiguous float32 [n, 3|4, 4]")
    with _span("cam_pose"):
        rc = lib().nslam_cam_pose_batch(ptr(cams), ptr(c2w), c2w.shape[1] * 4, n, stream_ptr(cams.device))
    check(rc, "nslam_cam_pose_batch")
    return c2w


def loss_sum_best(ray_loss, out, best_loss=None, cam=None, best=None):
    """nslam_loss_sum_best (ABI v21): out (float64 device scalar) = ray_loss.sum() in a fixed order (one
    workgroup: the same value on every call); with best_loss: if out < best_loss, best_loss = out and
    best = cam (the tracker's best-pose update, Tracker.py:245-247).  Returns out."""
    if ray_loss.dtype != torch.float64 or out.dtype != torch.float64 or not ray_loss.is_contiguous():
        raise ValueError("loss_sum_best: a contiguous float64 ray_loss and a float64 scalar out")
    if best_loss is not None and (best_loss.dtype != torch.float64 or cam.dtype != torch.float32
                                  or best.shape != cam.shape or not (cam.is_contiguous() and best.is_contiguous())):
        raise ValueError("loss_sum_best: a float64 best_loss and two contiguous float32 vectors of one shape")
    check(lib().nslam_loss_sum_best(ptr(ray_loss), ray_loss.numel(), ptr(out),
                                    ptr(best_loss) if best_loss is not None else None,
                                    ptr(cam) if best_loss is not None else None,
                                    ptr(best) if best_loss is not None else None,
                                    cam.numel() if best_loss is not None else 0, stream_ptr(ray_loss.device)),
          "nslam_loss_sum_best")
    return out


def cam_grad_batch(cams, c2w, ray_begin, n_per, g_pts, z, rd, out, ws, tickets):
    """nslam_cam_grad_batch (ABI v19): out [n, 7] = d loss / d cams [n, 7] of the bundle-adjustment cameras,
    camera k's rays being [ray_begin[k], ray_begin[k] + n_per) of the batch (z [N, S] f64, rd [N, 3] f32,
    g_pts: list of [N*S, 3] f64 d/dpts shares); c2w [n, 3|4, 4] the poses rendered with; ws f64
    [n * NSLAM_CAM_GRAD_WS_DOUBLES], tickets int32 [n] zeroed once (persistent per caller)."""
    n = cams.shape[0]
    N, S = z.shape
    _expect("cam_grad_batch", [(cams, torch.float32, (n, 7)), (z, torch.float64, (N, S)), (rd, torch.float32, (N, 3)),
                               (out, torch.float32, (n, 7)), (ws, torch.float64, (n * CAM_GRAD_WS_DOUBLES,)),
                               (tickets, torch.int32, (n,))] + [(g, torch.float64, (N * S, 3)) for g in g_pts])
    if c2w.dtype != torch.float32 or c2w.dim() != 3 or c2w.shape[0] != n or not c2w.is_contiguous():
        raise ValueError("cam_grad_batch: c2w must be a contiguous float32 [n, 3|4, 4]")
    rb = (ctypes.c_int64 * n)(*[int(r) for r in ray_begin])
    bufs = (ctypes.c_void_p * len(g_pts))(*[ptr(g) for g in g_pts])
    with _span("cam_grad"):
        rc = lib().nslam_cam_grad_batch(ptr(cams), ptr(c2w), c2w.shape[1] * 4, n, rb, int(n_per), bufs, len(g_pts),
                                        ptr(z), ptr(rd), N, S, ptr(out), ptr(ws), ptr(tickets), stream_ptr(cams.device))
    check(rc, "nslam_cam_grad_batch")
    return out


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
                            int(bool(handle_dynamic)), float(w_color), ptr(occ_add) if occ_add is not None else None)
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
        with _span("render_loss"):
            rc = lib().nslam_render_loss(ctypes.byref(cfg), ptr(raw), ptr(z), n, s, ptr(gt_depth), ptr(gt_color),
                                         ptr(keep), ptr(depth), ptr(var), ptr(color), ptr(ray_loss), ptr(g_raw),
                                         ptr(ws), wsb, stream_ptr(dev))
        check(rc, "nslam_render_loss")
    return depth, var, color, ray_loss, g_raw


def rows_pack(grid_flat, rows, tail, out):
    """nslam_rows_pack: out = [grid_flat.view(-1, 32)[rows], tail] (either part may be None)."""
    n = rows.numel() if rows is not None else 0
    nt = tail.numel() if tail is not None else 0
    with _span("rows_xfer"):
        rc = lib().nslam_rows_pack(ptr(grid_flat) if n else None, ptr(rows) if n else None, n, 32, ptr(tail), nt,
                                   ptr(out), stream_ptr(out.device))
    check(rc, "nslam_rows_pack")


def rows_unpack(buf, rows, grid_flat, tail):
    """nslam_rows_unpack: the inverse of rows_pack."""
    n = rows.numel() if rows is not None else 0
    nt = tail.numel() if tail is not None else 0
    with _span("rows_xfer"):
        rc = lib().nslam_rows_unpack(ptr(buf), ptr(rows) if n else None, n, 32, ptr(grid_flat) if n else None,
                                     ptr(tail), nt, stream_ptr(buf.device))
    check(rc, "nslam_rows_unpack")


class FusedAdam:
    """torch.optim.Adam (betas, eps; no weight decay / amsgrad) stepping every parameter segment
    in one HIP launch (nslam_adam_step).  Construction mirrors torch:

        FusedAdam([{"params": [...], "lr": 0.005}, {"params": [grid], "lr": 0.1, "rows": idx}, ...])

    A group's "rows" (int32 device tensor of voxel indices) restricts a channels-last grid to the
    frustum-selected voxels (Mapper.py:314-333): only those rows are updated, in place, with Adam
    state for them alone.  Parameters whose .grad is None are skipped like torch does (their step
    count does not advance); `grads` may map a parameter to an explicit gradient tensor instead.
    Step counts live on the device, so step() can be captured in a hipGraph.
    """

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8):
        self.param_groups = []
        self.betas, self.eps = betas, eps
        self.state = {}
        dev = None
        for g in groups:
            g = dict(g)
            g["params"] = list(g["params"])
            self.param_groups.append(g)
            for p in g["params"]:
                dev = p.device
        self.device = dev
        self._tickets = {}  # one step ticket per parameter subset (subsets may step concurrently)
        self.mirrors = {}

    def set_mirror(self, p, idx, dst):
        """After each update also store dense parameter p into dst at idx ([p.numel(), 2] int32,
        -1 = none): keeps a decoder's MFMA-packed copy current inside the Adam launch."""
        if idx.shape != (p.numel(), 2) or idx.dtype != torch.int32 or not idx.is_contiguous():
            raise ValueError("mirror index must be int32 [numel, 2]")
        self.mirrors[p] = (idx, dst)

    def _st(self, p, rows):
        st = self.state.get(p)
        if st is None:
            if rows is not None:
                n = rows.numel() * 32
                ex, ex2 = (torch.zeros(n, dtype=torch.float32, device=p.device) for _ in range(2))
            else:
                ex, ex2 = torch.zeros_like(p), torch.zeros_like(p)
            st = {"exp_avg": ex, "exp_avg_sq": ex2, "step": torch.zeros(1, dtype=torch.float32, device=p.device)}
            self.state[p] = st
        return st

    def segments(self, grads=None):
        segs = []
        for g in self.param_groups:
            rows = g.get("rows")
            for p in g["params"]:
                gr = grads.get(p) if grads is not None else p.grad
                if gr is None:
                    continue
                st = self._st(p, rows)
                s = _lib.NslamAdamSeg()
                s.param, s.grad = ptr(p.data), ptr(gr)
                s.exp_avg, s.exp_avg_sq, s.step = ptr(st["exp_avg"]), ptr(st["exp_avg_sq"]), ptr(st["step"])
                if rows is not None:
                    # grad: dense like the grid, or compact [n_rows][32] in row-list order (engine
                    # frustum-compacted gradients, ABI v6)
                    compact = gr.dim() == 2
                    if compact and not (gr.is_contiguous() and gr.shape == (rows.numel(), p.shape[1])):
                        raise ValueError("compact grid gradient must be [n_rows, 32] contiguous")
                    if not (p.is_contiguous(memory_format=torch.channels_last_3d) and
                            (compact or gr.is_contiguous(memory_format=torch.channels_last_3d))):
                        raise ValueError("row-masked Adam needs channels-last grid and grad")
                    s.rows, s.n, s.row_len = ptr(rows), rows.numel(), p.shape[1]
                    s.grad_rows = int(compact)
                    if g.get("n_live") is not None:  # ABI v19: rows sized for a capacity, live count on the device
                        s.n_live = ptr(g["n_live"])
                else:  # elementwise over storage: any dense layout shared by param, grad and state
                    dense = p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last_3d)
                    if not (dense and gr.stride() == p.stride() and st["exp_avg"].stride() == p.stride()):
                        raise ValueError("dense Adam segments need param, grad and state of one dense layout")
                    s.rows, s.n, s.row_len = None, p.numel(), 0
                    mi = self.mirrors.get(p)
                    if mi is not None:
                        s.mirror_idx, s.mirror = ptr(mi[0]), ptr(mi[1])
                s.lr = float(g["lr"])
                segs.append((s, p, gr))
        return segs

    @torch.no_grad()
    def step(self, grads=None, zero_grad=False):
        segs = self.segments(grads)
        if not segs:
            return
        if len(segs) > _lib.ADAM_MAX_SEGS:
            raise ValueError(f"at most {_lib.ADAM_MAX_SEGS} parameter tensors per step (flatten the decoders)")
        arr = (_lib.NslamAdamSeg * len(segs))(*[s for s, _, _ in segs])
        b1, b2 = self.betas
        key = tuple(id(p) for _, p, _ in segs)
        ticket = self._tickets.get(key)
        if ticket is None:
            # a ticket made during capture would come from the graph's private pool with its zero-fill
            # baked into the graph: every subset must step once eagerly first
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam: first step of a parameter subset inside graph capture; "
                                   "run one eager step of it before capturing")
            ticket = self._tickets[key] = torch.zeros(1, dtype=torch.int32, device=self.device)
        with _span("adam"):
            rc = lib().nslam_adam_step(arr, len(segs), b1, b2, self.eps, int(bool(zero_grad)), ptr(ticket),
                                       stream_ptr(self.device))
        check(rc, "nslam_adam_step")

    def group_of(self, p):
        """The parameter group holding p."""
        for g in self.param_groups:
            if any(q is p for q in g["params"]):
                return g
        raise KeyError("not a parameter of this optimiser")

    def state_of(self, p):
        """(exp_avg, exp_avg_sq, step) of p, created on first use (dense, or [n_rows * row_len] for a
        row-masked group, as step() keeps them)."""
        st = self._st(p, self.group_of(p).get("rows"))
        return st["exp_avg"], st["exp_avg_sq"], st["step"]

    @torch.no_grad()
    def step_segments(self, segs, key, zero_grad=False):
        """nslam_adam_step over explicit segments (NslamAdamSeg structs built by the caller — e.g. one
        rank's slices of the parameters, distributed.ShardedAdamExchange), with this optimiser's
        betas / eps and a ticket of its own per `key`.  A parameter's step count must appear in at
        most one segment of the call."""
        if not segs:
            return
        if len(segs) > _lib.ADAM_MAX_SEGS:
            raise ValueError(f"at most {_lib.ADAM_MAX_SEGS} segments per step")
        ticket = self._tickets.get(key)
        if ticket is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam: first step of a segment set inside graph capture; run one eager step")
            ticket = self._tickets[key] = torch.zeros(1, dtype=torch.int32, device=self.device)
        arr = (_lib.NslamAdamSeg * len(segs))(*segs)
        b1, b2 = self.betas
        with _span("adam"):
            rc = lib().nslam_adam_step(arr, len(segs), b1, b2, self.eps, int(bool(zero_grad)), ptr(ticket),
                                       stream_ptr(self.device))
        check(rc, "nslam_adam_step")

    def init_state(self):
        """Create every parameter's Adam state now (buffers a hipGraph captured later can hold by address)."""
        for g in self.param_groups:
            for p in g["params"]:
                self._st(p, g.get("rows"))

    @torch.no_grad()
    def reset_state(self):
        """Zero every parameter's Adam state (moments and step count) in place: the optimiser then behaves
        as a freshly built one (Mapper.optimize_map re-creates its Adam per call, Mapper.py:365-389), while
        the state buffers — which captured hipGraphs hold by address — stay where they are."""
        for st in self.state.values():
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
            st["step"].zero_()

    def prepare(self, grads=None):
        """Create (eagerly, outside any graph capture) the Adam state and the step ticket of the parameter
        subset a step(grads) would update, so the step can be captured in a hipGraph."""
        segs = self.segments(grads)
        key = tuple(id(p) for _, p, _ in segs)
        if segs and key not in self._tickets:
            self._tickets[key] = torch.zeros(1, dtype=torch.int32, device=self.device)

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        p.grad.zero_()


# ------------------------------------------------------------------------------------------------
# mesh extraction (csrc/nslam_mesh.hip)
# ------------------------------------------------------------------------------------------------
def _want(t, name, dtype, shape=None):
    """Dtype / contiguity / shape check of a tensor whose pointer is handed to a kernel."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: nice-slam_amd kernels run on the HIP device only; got a CPU tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None:
        if t.dim() != len(shape) or any(s is not None and int(d) != int(s) for d, s in zip(t.shape, shape)):
            raise ValueError(f"{name}: expected shape {list(shape)}, got {list(t.shape)}")
    return t


def point_masks(points, w2c, depth, H, W, fx, fy, cx, cy, depth_test, use_all_frames, points_batch_size):
    """nslam_point_masks → (seen, forecast, unseen) bool [N] on the device.

    points float32 [N,3]; w2c float32 [K,4,4]; depth float32 [K,H,W] (None with use_all_frames)."""
    _want(points, "points", torch.float32, (None, 3))
    n, dev = points.shape[0], points.device
    k = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float32, (k, 4, 4))
    if not use_all_frames:
        if depth is None:
            raise ValueError("point_masks: depth images are needed unless use_all_frames")
        _want(depth, "depth", torch.float32, (k, H, W))
    else:
        depth = None
    if int(points_batch_size) <= 0:
        raise ValueError("point_masks: points_batch_size must be positive")
    out = torch.empty(3, n, dtype=torch.uint8, device=dev)
    wsb = lib().nslam_point_masks_workspace_size(n, k, int(points_batch_size))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    rc = lib().nslam_point_masks(ptr(points), n, ptr(w2c), k, ptr(depth), int(H), int(W), float(fx), float(fy),
                                 float(cx), float(cy), int(bool(depth_test)), int(bool(use_all_frames)),
                                 int(points_batch_size), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), wsb,
                                 stream_ptr(dev))
    check(rc, "nslam_point_masks")
    return out[0].bool(), out[1].bool(), out[2].bool()


def marching_cubes(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """Indexed iso-surface of a float32 volume [nx,ny,nz] → (verts float64 [V,3], faces int32 [F,3]).

    One vertex per lattice edge with (a < level) != (b < level), at origin + (index + t)·spacing; vertices in
    owner-edge order, faces in cell order, normals toward decreasing values (nslam_mc_count / nslam_mc_emit)."""
    _want(volume, "volume", torch.float32, (None, None, None))
    nx, ny, nz = (int(v) for v in volume.shape)
    dev = volume.device
    n = nx * ny * nz
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("marching_cubes: origin and spacing have three entries")
    wsb = lib().nslam_mc_workspace_size(nx, ny, nz)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib().nslam_mc_count(ptr(volume), nx, ny, nz, float(level), ptr(ws), wsb, stream_ptr(dev))
    check(rc, "nslam_mc_count")
    flags, ntri = ws[:3 * n], ws[3 * n:]
    vinc = torch.cumsum(flags, 0, dtype=torch.int32)
    finc = torch.cumsum(ntri, 0, dtype=torch.int32)
    n_verts, n_faces = int(vinc[-1]), int(finc[-1])
    verts = torch.empty(n_verts, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    if n_verts == 0 and n_faces == 0:
        return verts, faces
    voff = (vinc - flags).contiguous()
    foff = (finc - ntri).contiguous()
    o = (ctypes.c_double * 3)(*[float(v) for v in origin])
    sp = (ctypes.c_double * 3)(*[float(v) for v in spacing])
    rc = lib().nslam_mc_emit(ptr(volume), nx, ny, nz, float(level), o, sp, ptr(voff), ptr(foff), n_verts, n_faces,
                             ptr(verts), ptr(faces), stream_ptr(dev))
    check(rc, "nslam_mc_emit")
    return verts, faces


def points_in_hull(points, planes):
    """nslam_points_in_hull → bool [N]: planes[k]·(p, 1) <= 0 for all k.  points float32/float64 [N,3]."""
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points: expected float32 or float64, got {points.dtype}")
    _want(points, "points", points.dtype, (None, 3))
    _want(planes, "planes", torch.float64, (None, 4))
    n, dev = points.shape[0], points.device
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib().nslam_points_in_hull(ptr(points), int(points.dtype == torch.float64), n, ptr(planes),
                                    int(planes.shape[0]), ptr(out), stream_ptr(dev))
    check(rc, "nslam_points_in_hull")
    return out.bool()


def mesh_face_cull(faces, vertex_mask):
    """nslam_mesh_face_cull → bool [F]: False for faces whose three vertices are all masked."""
    _want(faces, "faces", torch.int32, (None, 3))
    vm = vertex_mask.to(torch.uint8) if vertex_mask.dtype == torch.bool else vertex_mask
    _want(vm, "vertex_mask", torch.uint8, (None,))
    nf, nv = faces.shape[0], vm.shape[0]
    if nf and (nv == 0 or int(faces.max()) >= nv or int(faces.min()) < 0):
        raise ValueError("mesh_face_cull: a face indexes past the vertex mask")
    keep = torch.empty(nf, dtype=torch.uint8, device=faces.device)
    rc = lib().nslam_mesh_face_cull(ptr(faces), nf, ptr(vm), nv, ptr(keep), stream_ptr(faces.device))
    check(rc, "nslam_mesh_face_cull")
    return keep.bool()


def mesh_components(verts, faces):
    """nslam_mesh_components → (label int32 [V], area float64 [V]); area[l] is the area of component l."""
    _want(verts, "verts", torch.float64, (None, 3))
    _want(faces, "faces", torch.int32, (None, 3))
    nv, nf, dev = verts.shape[0], faces.shape[0], verts.device
    if nf and (nv == 0 or int(faces.max()) >= nv or int(faces.min()) < 0):
        raise ValueError("mesh_components: a face indexes past the vertices")
    label = torch.empty(nv, dtype=torch.int32, device=dev)
    area = torch.empty(nv, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = lib().nslam_mesh_components(ptr(verts), nv, ptr(faces), nf, ptr(label), ptr(area), ptr(flag), stream_ptr(dev))
    check(rc, "nslam_mesh_components")
    return label, area


def mesh_keep_components(verts, faces, largest, area_threshold=0.0):
    """trimesh's split + the reference's choice (Mesher.py:498-510): the largest component (largest=True) or
    every component with area > area_threshold, compacted → (verts, faces, vertex ids kept int64)."""
    label, area = mesh_components(verts, faces)
    nv, nf, dev = verts.shape[0], faces.shape[0], verts.device
    if nf == 0:
        return verts[:0], faces[:0], torch.zeros(0, dtype=torch.int64, device=dev)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    used = torch.zeros(nv, dtype=torch.uint8, device=dev)
    big = torch.argmax(area).reshape(1).contiguous() if largest else None
    rc = lib().nslam_mesh_select(ptr(faces), nf, ptr(label), ptr(area), ptr(big), float(area_threshold), ptr(keep),
                                 ptr(used), stream_ptr(dev))
    check(rc, "nslam_mesh_select")
    new_id = (torch.cumsum(used, 0, dtype=torch.int32) - used).contiguous()
    kept_faces = faces[keep.bool()].contiguous()
    out = torch.empty_like(kept_faces)
    rc = lib().nslam_mesh_remap(ptr(kept_faces), kept_faces.shape[0], ptr(new_id), ptr(out), stream_ptr(dev))
    check(rc, "nslam_mesh_remap")
    ids = torch.nonzero(used).reshape(-1)
    return verts[ids], out, ids


# ------------------------------------------------------------------------------------------------
# evaluation (csrc/nslam_eval.hip)
# ------------------------------------------------------------------------------------------------
def frustum_seen(vertices, w2c, H, W, fx, fy, cx, cy):
    """nslam_frustum_seen → bool [N]: the vertex projects into the image of any camera.

    vertices float64 [N,3]; w2c float32 [K,4,4] (inverted on the host by the caller)."""
    _want(vertices, "vertices", torch.float64, (None, 3))
    k = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float32, (k, 4, 4))
    n, dev = vertices.shape[0], vertices.device
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib().nslam_frustum_seen(ptr(vertices), n, ptr(w2c), k, int(H), int(W), float(fx), float(fy), float(cx),
                                  float(cy), ptr(out), stream_ptr(dev))
    check(rc, "nslam_frustum_seen")
    return out.bool()


def _want_mesh(vertices, faces, what):
    _want(vertices, "vertices", torch.float64, (None, 3))
    _want(faces, "faces", torch.int32, (None, 3))
    nv, nf = vertices.shape[0], faces.shape[0]
    if nf and (nv == 0 or int(faces.max()) >= nv or int(faces.min()) < 0):
        raise ValueError(f"{what}: a face indexes past the vertices")
    return nv, nf


def face_areas(vertices, faces):
    """nslam_face_areas → float64 [F]."""
    nv, nf = _want_mesh(vertices, faces, "face_areas")
    area = torch.empty(nf, dtype=torch.float64, device=vertices.device)
    rc = lib().nslam_face_areas(ptr(vertices), nv, ptr(faces), nf, ptr(area), stream_ptr(vertices.device))
    check(rc, "nslam_face_areas")
    return area


def sample_surface(vertices, faces, count, seed, cdf=None):
    """nslam_sample_surface → (points float64 [count,3], face_id int32 [count], cdf float64 [F]).

    Area-weighted samples from the counter-based stream (seed, sample, k); cdf = cumsum(face areas) unless given."""
    nv, nf = _want_mesh(vertices, faces, "sample_surface")
    dev = vertices.device
    count = int(count)
    if count < 0:
        raise ValueError("sample_surface: count must not be negative")
    if nf == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    if cdf is None:
        cdf = torch.cumsum(face_areas(vertices, faces), 0)
    _want(cdf, "cdf", torch.float64, (nf,))
    total = float(cdf[-1])
    if not (total > 0.0 and total < float("inf")):
        raise ValueError(f"sample_surface: the mesh's area is {total}")
    points = torch.empty(count, 3, dtype=torch.float64, device=dev)
    face_id = torch.empty(count, dtype=torch.int32, device=dev)
    rc = lib().nslam_sample_surface(ptr(vertices), nv, ptr(faces), ptr(cdf), nf, count,
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(points), ptr(face_id), stream_ptr(dev))
    check(rc, "nslam_sample_surface")
    return points, face_id, cdf


NN_MAX_CELLS = 1 << 24
NN_PER_CELL = 2.0  # targets aimed at per occupied cell


def nn_cell_grid(lo, hi, m):
    """Cell edge and cell counts (host) of the grid over the box lo..hi for m targets, taken as samples of a
    surface: about NN_PER_CELL targets per occupied cell on the box's own surface area; an axis of zero extent
    gets one cell, every axis at least one, at most NN_MAX_CELLS in all."""
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0])
    if area > 0.0:
        cell = (NN_PER_CELL * area / m) ** 0.5
    elif max(ext) > 0.0:
        cell = NN_PER_CELL * max(ext) / m
    else:
        cell = 1.0
    cell = max(cell, max(ext) * 2.0 ** -20, 2.0 ** -1000)
    while True:
        dims = [int(e / cell) + 1 for e in ext]
        if dims[0] * dims[1] * dims[2] <= NN_MAX_CELLS:
            return cell, dims
        cell *= 1.25


class NNGrid:
    """The targets of nn_query sorted into a uniform cell grid (nslam_nn_build): built once per target set."""

    def __init__(self, targets):
        _want(targets, "targets", torch.float64, (None, 3))
        m, dev = targets.shape[0], targets.device
        if m == 0:
            raise ValueError("NNGrid: no targets")
        lo_t, hi_t = targets.min(0).values, targets.max(0).values
        box = torch.stack([lo_t, hi_t]).cpu().tolist()
        if not all(abs(v) < float("inf") for row in box for v in row):  # NaN fails the comparison too
            raise ValueError("NNGrid: a target is not finite")
        self.cell, dims = nn_cell_grid(box[0], box[1], m)
        self.lo = (ctypes.c_double * 3)(*box[0])
        self.dims = (ctypes.c_int32 * 3)(*dims)
        self.cells = dims[0] * dims[1] * dims[2]
        keys = torch.empty(m, dtype=torch.int32, device=dev)
        rc = lib().nslam_nn_build(ptr(targets), m, self.lo, self.cell, self.dims, ptr(keys), stream_ptr(dev))
        check(rc, "nslam_nn_build")
        skeys, order = torch.sort(keys, stable=True)
        self.orig = order.to(torch.int32).contiguous()
        self.sorted = targets[order].contiguous()
        self.start = torch.searchsorted(skeys, torch.arange(self.cells + 1, dtype=torch.int32, device=dev)) \
            .to(torch.int32).contiguous()
        self.targets, self.m = targets, m

    def query(self, queries, max_dist=None):
        """nslam_nn_query → (dist float64 [N], idx int32 [N] into the original targets; inf / -1 past max_dist)."""
        _want(queries, "queries", torch.float64, (None, 3))
        n, dev = queries.shape[0], queries.device
        if n and not bool(torch.isfinite(queries).all()):
            raise ValueError("nn_query: a query is not finite")
        md = -1.0 if max_dist is None else float(max_dist)
        if max_dist is not None and not md >= 0.0:
            raise ValueError("nn_query: max_dist must be >= 0")
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        rc = lib().nslam_nn_query(ptr(queries), n, ptr(self.sorted), ptr(self.orig), self.m, ptr(self.start),
                                  self.start.shape[0], self.lo, self.cell, self.dims, md, ptr(dist), ptr(idx),
                                  stream_ptr(dev))
        check(rc, "nslam_nn_query")
        return dist, idx


def transform_points(points, matrix):
    """nslam_transform_points → float64 [N,3]: R p + t for the host 4x4 (or 3x4) `matrix`."""
    _want(points, "points", torch.float64, (None, 3))
    flat = [float(matrix[r][c]) for r in range(3) for c in range(4)]
    out = torch.empty_like(points)
    rc = lib().nslam_transform_points(ptr(points), points.shape[0], (ctypes.c_double * 12)(*flat), ptr(out),
                                      stream_ptr(points.device))
    check(rc, "nslam_transform_points")
    return out


def kabsch_sums(src, idx, targets):
    """nslam_kabsch_sums → numpy float64 [17]: count, Σa, Σb, Σabᵀ, Σ|a-b|² over the pairs
    (src[i], targets[idx[i]]) with idx[i] >= 0.  The workgroup partials are read back (ICP's one small copy per
    iteration) and added in index order on the host, so the sums are the same on every run."""
    _want(src, "src", torch.float64, (None, 3))
    n, dev = src.shape[0], src.device
    _want(idx, "idx", torch.int32, (n,))
    _want(targets, "targets", torch.float64, (None, 3))
    wgs = lib().nslam_kabsch_partials(n)
    partials = torch.empty(max(wgs, 1), 17, dtype=torch.float64, device=dev)
    if wgs == 0:
        return partials.zero_()[0].cpu().numpy()
    rc = lib().nslam_kabsch_sums(ptr(src), ptr(idx), n, ptr(targets), targets.shape[0], ptr(partials), wgs,
                                 stream_ptr(dev))
    check(rc, "nslam_kabsch_sums")
    return partials.cpu().numpy().cumsum(0)[-1]  # numpy's cumsum is one sequential chain per column


# ------------------------------------------------------------------------------------------------
# depth L1 (csrc/nslam_raster.hip, csrc/nslam_eval.hip)
# ------------------------------------------------------------------------------------------------
RASTER_CLEAR, RASTER_SMALL, RASTER_BIG, RASTER_RESOLVE, RASTER_ALL = 1, 2, 4, 8, 15
RASTER_SMALL_MAX_PIXELS = 64     # a larger pixel box goes to the list pass (how it was chosen)
RASTER_WS_BYTES = 64 << 20       # the list's byte budget: 8 M items of 8 bytes
RASTER_MAX_VIEWS = 65535         # views per launch (one grid row each)


def raster_workspace(capacity, device):
    """A workspace for render_depth whose list of large items holds `capacity` entries (uint8 tensor)."""
    return torch.empty(lib().nslam_raster_workspace_size(int(capacity)), dtype=torch.uint8, device=device)


def render_depth(vertices, faces, w2c, H, W, fx, fy, cx, cy, z_near, z_far, small_max_pixels=None, ws=None,
                 passes=RASTER_ALL, out=None):
    """nslam_raster_depth → float32 [B,H,W]: the camera-space z of the nearest triangle along the ray through every
    pixel centre, 0 where nothing is hit.

    vertices float64 [V,3]; faces int32 [F,3]; w2c float64 [B,3,4] or [B,4,4] (the camera looks along +z, x right,
    y down).  small_max_pixels: the largest pixel box a (face, view) thread tests itself (None: the default);
    ws: a raster_workspace (None: one of RASTER_WS_BYTES).  The image does not depend on either.  passes / out:
    run single passes on an image kept between calls (tools/eval_bench.py's per-stage timing)."""
    nv, nf = _want_mesh(vertices, faces, "render_depth")
    dev = vertices.device
    if not isinstance(w2c, torch.Tensor) or not w2c.is_cuda:
        raise RuntimeError("w2c: nice-slam_amd kernels run on the HIP device only; got a CPU tensor")
    if w2c.dim() == 3 and tuple(w2c.shape[1:]) == (4, 4):
        w2c = w2c[:, :3, :].contiguous()
    b = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float64, (b, 3, 4))
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or not float(fx) > 0 or not float(fy) > 0:
        raise ValueError("render_depth: H, W, fx and fy must be positive")
    if not (0.0 <= float(z_near) < float(z_far)):
        raise ValueError(f"render_depth: need 0 <= z_near < z_far, got {z_near}, {z_far}")
    small = RASTER_SMALL_MAX_PIXELS if small_max_pixels is None else int(small_max_pixels)
    if small < 0:
        raise ValueError("render_depth: small_max_pixels must not be negative")
    if out is None:
        out = torch.empty(b, H, W, dtype=torch.float32, device=dev)
        if nf == 0:
            out.zero_()
    _want(out, "out", torch.float32, (b, H, W))
    if b == 0 or nf == 0:
        return out
    if ws is None:
        ws = torch.empty(RASTER_WS_BYTES, dtype=torch.uint8, device=dev)
    _want(ws, "ws", torch.uint8, (None,))
    for v0 in range(0, b, RASTER_MAX_VIEWS):
        v1 = min(b, v0 + RASTER_MAX_VIEWS)
        rc = lib().nslam_raster_depth(ptr(vertices), nv, ptr(faces), nf, ptr(w2c[v0:v1]), v1 - v0, H, W, float(fx),
                                      float(fy), float(cx), float(cy), float(z_near), float(z_far), small,
                                      int(passes), ptr(out[v0:v1]), ptr(ws), ws.numel(), stream_ptr(dev))
        check(rc, "nslam_raster_depth")
    return out


def raster_list_length(ws):
    """The number of items the last SMALL pass appended to (or, past the capacity, drew instead of) the list."""
    return int(ws[:8].view(torch.int64)[0])


SCENE_POINTS, SCENE_ALL = 16, 31
CULL_MODES = {"none": 0, "back": 1, "front": 2}
SCENE_MAX_POINT_SIZE = 64


def scene_workspace(capacity, n_views, H, W, device):
    """A workspace for render_scene: a list of `capacity` large items and the keys of n_views images (uint8 tensor)."""
    n = lib().nslam_scene_workspace_size(int(capacity), int(n_views), int(H), int(W))
    return torch.empty(n, dtype=torch.uint8, device=device)


def _rgb3(c, name):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise ValueError(f"render_scene: {name} must be three values in 0..255")
    return (ctypes.c_uint8 * 3)(*c)


def render_scene(vertices, faces, vertex_colors, normals, points, point_colors, w2c, H, W, fx, fy, cx, cy, z_near,
                 z_far, point_size=4, cull="none", background=(255, 255, 255), grey=(178, 178, 178), ambient=0.3,
                 small_max_pixels=None, ws=None, passes=SCENE_ALL, out=None, want_depth=True, want_ids=True):
    """nslam_scene_render → (colour uint8 [B,H,W,3], depth float32 [B,H,W] or None, ids int32 [B,H,W] or None): a
    mesh with vertex colours under a head light and depth-tested point sprites, from render_depth's cameras.

    vertices float64 [V,3], faces int32 [F,3], vertex_colors uint8 [V,3] or None (every vertex `grey`), normals
    float32 or float64 [V,3] (unit; not read when F == 0, then all four may be None); points float64 [P,3] and
    point_colors uint8 [P,3] (both None: no points); w2c float64 [B,3,4] or [B,4,4].  ids: a face index, -2 - the
    point's index, -1 for background.  cull: "none" | "back" | "front".  small_max_pixels / ws (a scene_workspace
    for the views of one call; None: a list of RASTER_WS_BYTES): the images do not depend on either.  passes /
    out (the three images of an earlier call): single passes on a workspace kept between calls
    (tools/replay_bench.py's per-stage timing)."""
    if not isinstance(w2c, torch.Tensor) or not w2c.is_cuda:
        raise RuntimeError("w2c: nice-slam_amd kernels run on the HIP device only; got a CPU tensor")
    dev = w2c.device
    if w2c.dim() == 3 and tuple(w2c.shape[1:]) == (4, 4):
        w2c = w2c[:, :3, :].contiguous()
    b = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float64, (b, 3, 4))
    nv = nf = 0
    if faces is not None and faces.shape[0] > 0:
        nv, nf = _want_mesh(vertices, faces, "render_scene")
        if vertex_colors is not None:
            _want(vertex_colors, "vertex_colors", torch.uint8, (nv, 3))
        if not isinstance(normals, torch.Tensor) or normals.dtype not in (torch.float32, torch.float64):
            raise TypeError("normals: expected a float32 or float64 tensor")
        _want(normals, "normals", normals.dtype, (nv, 3))
    else:
        vertices = faces = vertex_colors = normals = None
    n_pts = 0
    if points is not None and points.shape[0] > 0:
        _want(points, "points", torch.float64, (None, 3))
        n_pts = int(points.shape[0])
        _want(point_colors, "point_colors", torch.uint8, (n_pts, 3))
    else:
        points = point_colors = None
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or not float(fx) > 0 or not float(fy) > 0:
        raise ValueError("render_scene: H, W, fx and fy must be positive")
    if not (0.0 <= float(z_near) < float(z_far)):
        raise ValueError(f"render_scene: need 0 <= z_near < z_far, got {z_near}, {z_far}")
    if cull not in CULL_MODES:
        raise ValueError(f"render_scene: cull must be one of {sorted(CULL_MODES)}, got {cull!r}")
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError("render_scene: ambient must lie in [0, 1]")
    if not 0.0 < float(point_size) <= SCENE_MAX_POINT_SIZE:
        raise ValueError(f"render_scene: point_size must lie in (0, {SCENE_MAX_POINT_SIZE}]")
    small = RASTER_SMALL_MAX_PIXELS if small_max_pixels is None else int(small_max_pixels)
    if small < 0:
        raise ValueError("render_scene: small_max_pixels must not be negative")
    bg, gr = _rgb3(background, "background"), _rgb3(grey, "grey")
    if out is None:
        out = (torch.empty(b, H, W, 3, dtype=torch.uint8, device=dev),
               torch.empty(b, H, W, dtype=torch.float32, device=dev) if want_depth else None,
               torch.empty(b, H, W, dtype=torch.int32, device=dev) if want_ids else None)
    color, depth, ids = out
    _want(color, "out[0]", torch.uint8, (b, H, W, 3))
    if depth is not None:
        _want(depth, "out[1]", torch.float32, (b, H, W))
    if ids is not None:
        _want(ids, "out[2]", torch.int32, (b, H, W))
    if b == 0:
        return color, depth, ids
    per = min(b, RASTER_MAX_VIEWS)
    if ws is None:
        ws = torch.empty(RASTER_WS_BYTES + 8 * per * H * W, dtype=torch.uint8, device=dev)
    _want(ws, "ws", torch.uint8, (None,))
    for v0 in range(0, b, RASTER_MAX_VIEWS):
        v1 = min(b, v0 + RASTER_MAX_VIEWS)
        rc = lib().nslam_scene_render(
            ptr(vertices), nv, ptr(faces), nf, ptr(vertex_colors), ptr(normals),
            int(normals is not None and normals.dtype == torch.float64), gr, ptr(points), ptr(point_colors), n_pts,
            float(point_size), ptr(w2c[v0:v1]), v1 - v0, H, W, float(fx), float(fy), float(cx), float(cy),
            float(z_near), float(z_far), CULL_MODES[cull], bg, float(ambient), small, int(passes), ptr(color[v0:v1]),
            ptr(None if depth is None else depth[v0:v1]), ptr(None if ids is None else ids[v0:v1]), ptr(ws),
            ws.numel(), stream_ptr(dev))
        check(rc, "nslam_scene_render")
    return color, depth, ids


def views_see_any(points, w2c, H, W, fx, fy, cx, cy):
    """nslam_views_see_any → bool [B]: the view's image holds some point of the cloud (frustum_seen's test).

    points float64 [N,3]; w2c float32 [B,4,4] (inverted on the host by the caller)."""
    _want(points, "points", torch.float64, (None, 3))
    b = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float32, (b, 4, 4))
    n, dev = points.shape[0], points.device
    out = torch.zeros(b, dtype=torch.uint8, device=dev)
    for v0 in range(0, b, RASTER_MAX_VIEWS):
        v1 = min(b, v0 + RASTER_MAX_VIEWS)
        rc = lib().nslam_views_see_any(ptr(points), n, ptr(w2c[v0:v1]), v1 - v0, int(H), int(W), float(fx), float(fy),
                                       float(cx), float(cy), ptr(out[v0:v1]), stream_ptr(dev))
        check(rc, "nslam_views_see_any")
    return out.bool()


def depth_l1(a, b):
    """nslam_depth_l1 → float64 [B]: the mean over a view's pixels of |a - b| (float32 [B,H,W] each)."""
    _want(a, "a", torch.float32, (None, None, None))
    _want(b, "b", torch.float32, tuple(a.shape))
    nb, npix = int(a.shape[0]), int(a.shape[1]) * int(a.shape[2])
    if nb and npix == 0:
        raise ValueError("depth_l1: the images have no pixels")
    out = torch.empty(nb, dtype=torch.float64, device=a.device)
    rc = lib().nslam_depth_l1(ptr(a), ptr(b), nb, npix, ptr(out), stream_ptr(a.device))
    check(rc, "nslam_depth_l1")
    return out


# ----------------------------------------------------------------------------------------------
# iMAP*: the 256-wide Fourier MLP, volume-density compositing, the hierarchical sampler
# ----------------------------------------------------------------------------------------------
def _imap_struct(B, ws, bs, wo, bo):
    s = _lib.NslamImapParams()
    s.B = B.data_ptr()
    for i in range(4):
        s.w[i] = ws[i].data_ptr()
        s.b[i] = bs[i].data_ptr()
    s.wo = wo.data_ptr()
    s.bo = bo.data_ptr()
    return s


_IMAP_SHAPES = ((3, 93), (256, 93), (256,), (256, 256), (256,), (256, 256), (256,), (256, 256), (256,), (4, 256), (4,))


def _imap_query_struct(pts, rays, bound):
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
        ps = _imap_struct(params[0], params[1:9:2], params[2:9:2], params[9], params[10])
        packed = torch.empty(L.nslam_imap_packed_size() // 4, dtype=torch.float32, device=dev)
        check(L.nslam_imap_pack(ctypes.byref(ps), ptr(packed), stream_ptr(dev)), "nslam_imap_pack")
        raw = torch.empty(n, 4, dtype=torch.float32, device=dev)
        tape = None
        if any(ctx.needs_input_grad):
            tape = torch.empty(L.nslam_imap_tape_size(n) // 4, dtype=torch.float32, device=dev)
        q = _imap_query_struct(pts, rays, bound)
        if n:
            with _span("imap_fwd"):
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
            ps = _imap_struct(params[0], params[1:9:2], params[2:9:2], params[9], params[10])
            gs = _imap_struct(grads[0], grads[1:9:2], grads[2:9:2], grads[9], grads[10]) if grads else None
            q = _imap_query_struct(ctx.pts, ctx.rays, ctx.bound)
            wsb = L.nslam_imap_bwd_workspace_size(n)
            ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
            with _span("imap_bwd"):
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
    return _ImapQuery.apply(None if oob_bound is None else _bound_list(oob_bound), None, p, *params)


def imap_query_rays(params, rays_o, rays_d, z, oob_bound=None):
    """imap_query at the points rays_o + rays_d * z (float64) formed inside the kernel; forward only (the
    differentiable path passes points, so that autograd carries the rays)."""
    with torch.no_grad():
        return _ImapQuery.apply(None if oob_bound is None else _bound_list(oob_bound), (rays_o, rays_d, z), None,
                                *params)


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
        with _span("sample_importance"):
            rc = lib().nslam_sample_importance(ptr(z), ptr(w), ptr(u), n, s, n_importance,
                                               ptr(out) if merged else None, None if merged else ptr(out),
                                               stream_ptr(z.device))
        check(rc, "nslam_sample_importance")
    return out


# ------------------------------------------------------------------------------------------------
# TSDF fusion (csrc/nslam_tsdf.hip); the volume itself is tsdf.TSDFVolume
# ------------------------------------------------------------------------------------------------
def _i3(v, name):
    if len(v) != 3:
        raise ValueError(f"{name}: three block indices expected")
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


def _tsdf_frames(depth, c2w, H, W):
    _want(depth, "depth", torch.float32, (None, int(H), int(W)))
    k = int(depth.shape[0])
    _want(c2w, "c2w", torch.float64, (k, 4, 4))
    return k


def tsdf_block_range(depth, c2w, H, W, fx, fy, cx, cy, stride, depth_trunc, voxel, trunc):
    """nslam_tsdf_block_range → (bounds int32 [6]: min x, y, z, max x, y, z; n_valid int64 [1]), on the device.

    depth float32 [K,H,W]; c2w float64 [K,4,4] (+z forward)."""
    k = _tsdf_frames(depth, c2w, H, W)
    dev = depth.device
    bounds = torch.empty(6, dtype=torch.int32, device=dev)
    n_valid = torch.empty(1, dtype=torch.int64, device=dev)
    rc = lib().nslam_tsdf_block_range(ptr(depth), ptr(c2w), k, int(H), int(W), float(fx), float(fy), float(cx),
                                      float(cy), int(stride), float(depth_trunc), float(voxel), float(trunc),
                                      ptr(bounds), ptr(n_valid), stream_ptr(dev))
    check(rc, "nslam_tsdf_block_range")
    return bounds, n_valid


def tsdf_touch(depth, c2w, H, W, fx, fy, cx, cy, stride, depth_trunc, voxel, trunc, block_lo, block_hi):
    """nslam_tsdf_touch → (mask int32 [cells]: bit f = frame f's samples reach the block, in table order;
    n_outside int64 [1]), on the device.  At most 32 frames."""
    k = _tsdf_frames(depth, c2w, H, W)
    dev = depth.device
    lo, hi = _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi")
    cells = max(0, hi[0] - lo[0]) * max(0, hi[1] - lo[1]) * max(0, hi[2] - lo[2])
    if not 0 < cells <= 1 << 27:
        raise ValueError(f"tsdf_touch: the block table [{list(lo)}, {list(hi)}) must hold 1 to 2^27 cells")
    mask = torch.empty(cells, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    rc = lib().nslam_tsdf_touch(ptr(depth), ptr(c2w), k, int(H), int(W), float(fx), float(fy), float(cx), float(cy),
                                int(stride), float(depth_trunc), float(voxel), float(trunc), lo, hi, ptr(mask),
                                ptr(n_out), stream_ptr(dev))
    check(rc, "nslam_tsdf_touch")
    return mask, n_out


def tsdf_integrate(depth, color, w2c, H, W, fx, fy, cx, cy, depth_trunc, voxel, trunc, block_lo, block_hi, list_key,
                   list_id, list_mask, n_pool, tsdf, weight, color_pool):
    """nslam_tsdf_integrate, in place on tsdf / weight [cap,4096] and color_pool [3,cap,4096] (or None).

    depth float32 [K,H,W]; color uint8 [K,H,W,3] or None; w2c float32 [K,4,4]; list_* int32 [n_list]."""
    _want(depth, "depth", torch.float32, (None, int(H), int(W)))
    k = int(depth.shape[0])
    _want(w2c, "w2c", torch.float32, (k, 4, 4))
    n_list = int(list_key.shape[0])
    for name, t in (("list_key", list_key), ("list_id", list_id), ("list_mask", list_mask)):
        _want(t, name, torch.int32, (n_list,))
    cap = int(tsdf.shape[0])
    if not 0 <= int(n_pool) <= cap:
        raise ValueError("tsdf_integrate: n_pool exceeds the pool's capacity")
    _want(tsdf, "tsdf", torch.float32, (cap, 4096))
    _want(weight, "weight", torch.float32, (cap, 4096))
    if color_pool is not None:
        _want(color_pool, "color_pool", torch.float32, (3, cap, 4096))
        if color is None:
            raise ValueError("tsdf_integrate: a volume with colour needs colour images")
        _want(color, "color", torch.uint8, (k, int(H), int(W), 3))
    else:
        color = None
    dev = depth.device
    rc = lib().nslam_tsdf_integrate(ptr(depth), ptr(color), ptr(w2c), k, int(H), int(W), float(fx), float(fy),
                                    float(cx), float(cy), float(depth_trunc), float(voxel), float(trunc),
                                    _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi"), ptr(list_key),
                                    ptr(list_id), ptr(list_mask), n_list, int(n_pool), ptr(tsdf), ptr(weight),
                                    ptr(color_pool), cap * 4096, stream_ptr(dev))
    check(rc, "nslam_tsdf_integrate")


def tsdf_marching_cubes(tsdf, weight, color_pool, pool_key, n_pool, table, block_lo, block_hi, voxel):
    """nslam_tsdf_mc_count / nslam_tsdf_mc_emit over the first n_pool blocks → (verts float64 [V,3], faces int32
    [F,3], colors uint8 [V,3] or None), vertices in pool / owner-edge order, faces in pool / cell order."""
    cap, n_pool = int(tsdf.shape[0]), int(n_pool)
    if not 0 <= n_pool <= cap:
        raise ValueError("tsdf_marching_cubes: n_pool exceeds the pool's capacity")
    _want(tsdf, "tsdf", torch.float32, (cap, 4096))
    _want(weight, "weight", torch.float32, (cap, 4096))
    if color_pool is not None:
        _want(color_pool, "color_pool", torch.float32, (3, cap, 4096))
    _want(pool_key, "pool_key", torch.int32, (None,))
    if int(pool_key.shape[0]) < n_pool:
        raise ValueError("tsdf_marching_cubes: pool_key is shorter than the pool")
    lo, hi = _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi")
    cells = max(0, hi[0] - lo[0]) * max(0, hi[1] - lo[1]) * max(0, hi[2] - lo[2])
    _want(table, "table", torch.int32, (cells,))
    dev = tsdf.device
    n = n_pool * 4096
    verts = torch.empty(0, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    colors = None if color_pool is None else torch.empty(0, 3, dtype=torch.uint8, device=dev)
    if n == 0:
        return verts, faces, colors
    flags = torch.empty(3 * n, dtype=torch.uint8, device=dev)
    ntri = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib().nslam_tsdf_mc_count(ptr(tsdf), ptr(weight), ptr(pool_key), n_pool, ptr(table), lo, hi, ptr(flags),
                                   ptr(ntri), stream_ptr(dev))
    check(rc, "nslam_tsdf_mc_count")
    vinc = torch.cumsum(flags, 0, dtype=torch.int32)
    finc = torch.cumsum(ntri, 0, dtype=torch.int32)
    n_verts, n_faces = int(vinc[-1]), int(finc[-1])
    if n_verts == 0 and n_faces == 0:
        return verts, faces, colors
    verts = torch.empty(n_verts, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    if color_pool is not None:
        colors = torch.empty(n_verts, 3, dtype=torch.uint8, device=dev)
    voff = (vinc - flags).contiguous()
    foff = (finc - ntri).contiguous()
    rc = lib().nslam_tsdf_mc_emit(ptr(tsdf), ptr(weight), ptr(color_pool), cap * 4096, ptr(pool_key), n_pool,
                                  ptr(table), lo, hi, float(voxel), ptr(flags), ptr(ntri), ptr(voff), ptr(foff),
                                  n_verts, n_faces, ptr(verts), ptr(colors), ptr(faces), stream_ptr(dev))
    check(rc, "nslam_tsdf_mc_emit")
    return verts, faces, colors


# ------------------------------------------------------------------------------------------------
# depth odometry (csrc/nslam_odometry.hip); the tracker itself is odometry.DepthOdometry
# ------------------------------------------------------------------------------------------------
def _pose16(m, name):
    """A 4x4 pose (tensor or array) as the HOST float64 [16] the odometry entry points read."""
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().tolist()
    flat = [float(x) for row in m for x in row]
    if len(flat) != 16:
        raise ValueError(f"{name}: a 4x4 matrix expected")
    return (ctypes.c_double * 16)(*flat)


def depth_maps(depth, fx, fy, cx, cy, depth_trunc, max_jump):
    """nslam_depth_maps → (vertex, normal) float32 [H,W,3] in the camera frame (+z forward), NaN where invalid.

    depth float32 [H,W]."""
    _want(depth, "depth", torch.float32, (None, None))
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if H < 1 or W < 1:
        raise ValueError("depth_maps: an empty image")
    dev = depth.device
    vertex = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    rc = lib().nslam_depth_maps(ptr(depth), H, W, float(fx), float(fy), float(cx), float(cy), float(depth_trunc),
                                float(max_jump), ptr(vertex), ptr(normal), stream_ptr(dev))
    check(rc, "nslam_depth_maps")
    return vertex, normal


def tsdf_raycast(table, pool_key, tsdf, weight, n_pool, block_lo, block_hi, voxel, trunc, c2w, H, W, fx, fy, cx, cy,
                 near, far):
    """nslam_tsdf_raycast over the first n_pool blocks → (vertex, normal) float32 [H,W,3] in the world frame, NaN
    where a ray hits nothing.  c2w: a 4x4 pose (+z forward), read on the host."""
    cap, n_pool = int(tsdf.shape[0]), int(n_pool)
    if not 0 <= n_pool <= cap:
        raise ValueError("tsdf_raycast: n_pool exceeds the pool's capacity")
    _want(tsdf, "tsdf", torch.float32, (cap, 4096))
    _want(weight, "weight", torch.float32, (cap, 4096))
    _want(pool_key, "pool_key", torch.int32, (None,))
    if int(pool_key.shape[0]) < n_pool:
        raise ValueError("tsdf_raycast: pool_key is shorter than the pool")
    lo, hi = _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi")
    cells = max(0, hi[0] - lo[0]) * max(0, hi[1] - lo[1]) * max(0, hi[2] - lo[2])
    _want(table, "table", torch.int32, (cells,))
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("tsdf_raycast: an empty image")
    dev = table.device
    vertex = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    rc = lib().nslam_tsdf_raycast(ptr(table), ptr(pool_key), ptr(tsdf), ptr(weight), n_pool, lo, hi, float(voxel),
                                  float(trunc), _pose16(c2w, "c2w"), H, W, float(fx), float(fy), float(cx), float(cy),
                                  float(near), float(far), ptr(vertex), ptr(normal), stream_ptr(dev))
    check(rc, "nslam_tsdf_raycast")
    return vertex, normal


def icp_sums(src_vertex, src_normal, T, model_vertex, model_normal, w2c, fx, fy, cx, cy, stride, dist_th, cos_th,
             return_mask=False):
    """nslam_icp_sums → float64 [29] on the device: the upper triangle of sum J J^T (21), sum J r (6), sum r^2 and
    the inlier count of the projective point-to-plane association (with return_mask also uint8 [Hs,Ws]: the
    accepted source pixels).

    src_* float32 [Hs,Ws,3] (camera frame); model_* float32 [Hm,Wm,3] (world frame, seen by the camera whose
    world-to-camera matrix is w2c); T, w2c: 4x4 poses read on the host."""
    _want(src_vertex, "src_vertex", torch.float32, (None, None, 3))
    Hs, Ws = int(src_vertex.shape[0]), int(src_vertex.shape[1])
    _want(src_normal, "src_normal", torch.float32, (Hs, Ws, 3))
    _want(model_vertex, "model_vertex", torch.float32, (None, None, 3))
    Hm, Wm = int(model_vertex.shape[0]), int(model_vertex.shape[1])
    _want(model_normal, "model_normal", torch.float32, (Hm, Wm, 3))
    if min(Hs, Ws, Hm, Wm) < 1 or int(stride) < 1:
        raise ValueError("icp_sums: non-empty maps and stride >= 1 expected")
    dev = src_vertex.device
    groups = int(lib().nslam_icp_partials(Hs, Ws, int(stride)))
    partial = torch.empty(groups, 29, dtype=torch.float64, device=dev)
    out = torch.empty(29, dtype=torch.float64, device=dev)
    mask = torch.empty(Hs, Ws, dtype=torch.uint8, device=dev) if return_mask else None
    rc = lib().nslam_icp_sums(ptr(src_vertex), ptr(src_normal), Hs, Ws, int(stride), _pose16(T, "T"),
                              ptr(model_vertex), ptr(model_normal), Hm, Wm, _pose16(w2c, "w2c"), float(fx), float(fy),
                              float(cx), float(cy), float(dist_th), float(cos_th), ptr(partial), groups, ptr(out),
                              ptr(mask), stream_ptr(dev))
    check(rc, "nslam_icp_sums")
    return (out, mask) if return_mask else out
