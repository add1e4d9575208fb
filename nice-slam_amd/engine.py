"""Fused NICE-SLAM mapping iteration on the HIP kernels, without autograd.

One iteration of Mapper.optimize_map's inner loop (src/Mapper.py:421-519) is

    randint pixels → get_samples + inside-mask     nslam_gather_rays        (1 launch)
    sampler                                         nslam_sample_rays        (2-3 launches)
    pts = o + d·z, grids + decoders → raw          nslam_query_fwd, ray form
    compositing + mapping loss + their backward    nslam_render_loss        (1 launch)
    zero gradients                                  one memset over a flat buffer
    decoders + grids backward                      nslam_query_bwd, ray form
    [ray-sharded: RCCL all-reduce of the gradients]
    Adam over frustum-masked grid rows + decoders  nslam_adam_step          (1 launch)
    re-pack the optimised decoder                   one gather

with every buffer persistent, so the whole iteration can be captured in a hipGraph.  The maths
is the reference's: the inside-mask drops rays by zero loss weight instead of compaction (their
gradients are exactly zero and the sampler's batch max only sees kept rays), and Adam updates
the frustum-selected voxels in place instead of through masked copies (Mapper.py:314-333,
394-401, 511-519) — the same elementwise update.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
import functools
import os
import weakref

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, lib, ptr, stream_ptr

_GRID_OF = {"coarse": "grid_coarse", "middle": "grid_middle", "fine": "grid_fine", "color": "grid_color"}


def _env_choice(name, default, allowed):
    """An engine topology knob from the environment, checked against its allowed values (a typo raises
    instead of silently selecting another stream topology)."""
    v = os.environ.get(name, default)
    if v not in allowed:
        raise ValueError(f"{name}={v!r}: expected one of {sorted(allowed)}")
    return v


def env_knobs():
    """The MappingEngine attributes that take their default from the environment."""
    return {
        # concurrent backward: enqueue the colour weight-gradient branch before the grid-gradient one
        # (its workgroups are dispatched first and hold one slot per CU; the lean launch fills the rest)
        "wgrad_first": _env_choice("NSLAM_WGRAD_FIRST", "1", ("0", "1")) == "1",
        # the ray prefetch's stream: the backward's first side stream ("lean", default: one side queue
        # fewer in a captured iteration) or its own ("own"); and one Adam call for the whole update on that
        # stream once both backward branches are done (NSLAM_ADAM_MERGE=1, default) instead of one per
        # branch (0).  A/B: profiles/r05_experiments/ab_defaults.txt
        "prefetch_stream": _env_choice("NSLAM_PREFETCH_STREAM", "lean", ("lean", "own")),
        "adam_merge": _env_choice("NSLAM_ADAM_MERGE", "1", ("0", "1")) == "1",
        # live-point lists (nslam_live_points): the mask-only backward of a mapping iteration without d/dpts
        # runs only the points that touch a frustum-selected voxel of the decoder's grid — with compacted
        # grid gradients the others add nothing.  The lists ride with the ray batch.  0: every point, as
        # nslam_query_bwd_decoders.  Measured on the synthetic room0 window only (about half of the kept
        # points are dead there); the dead share of a real sequence has not been measured.
        "live_points": _env_choice("NSLAM_LIVE_POINTS", "1", ("0", "1")) == "1",
    }


BackwardPlan = collections.namedtuple("BackwardPlan", "units streams has_wgrad merge_adam")


def backward_plan(decs, dec_grads, *, masks, tape, n, merge=True, wgrad_first=True, adam_merge=True,
                  concurrent=True, has_on_branch=True, ordered=False):
    """Which launches the backward of a stage's decoders `decs` consists of, and where each runs — no tensor,
    no stream.  dec_grads: the decoders with parameter gradients; masks / tape: the forward left ReLU masks / the
    colour decoder's activation tape; n: points; merge, wgrad_first, adam_merge, concurrent: the engine's
    knobs; has_on_branch: the caller updates per branch; ordered: its branch work must keep one order
    (query_bwd ordered_branches).  Returns
      units       ((kind, decoder names), ...) in enqueue order, kind =
                    "wgrad"  the colour decoder's parameter gradients from the tape (nslam_color_wgrad),
                    "lean"   the named decoders' grid gradients (and d/dpts) from the masks, one launch,
                    "one"    a decoder's whole backward by itself (nslam_query_bwd_decoder);
      streams     per unit: 0 = the caller's stream, k = the k-th side stream;
      has_wgrad   a "wgrad" unit exists (the colour grid and decoder are then updated after it AND "lean");
      merge_adam  the whole update is one call on the lean launch's stream once both units are done."""
    wgt = [d for d in decs if d in dec_grads]
    tape_color = "color" in wgt and masks and tape
    lean = tuple(d for d in decs if merge and masks and (d not in wgt or (d == "color" and tape_color)))
    units = []
    if "color" in lean and "color" in wgt and n > 0:
        units.append(("wgrad", ("color",)))
    if lean:
        units.append(("lean", lean))
    units += [("one", (d,)) for d in decs if d not in lean]
    if not wgrad_first:
        units.sort(key=lambda u: u[0] == "wgrad")
    has_wgrad = any(kind == "wgrad" for kind, _ in units)
    merge_adam = bool(adam_merge and has_wgrad and has_on_branch and not ordered and wgrad_first and concurrent
                      and len(units) == 2 and units[1][0] == "lean")
    par = concurrent and len(units) > 1
    return BackwardPlan(tuple(units), tuple(i if par else 0 for i in range(len(units))), has_wgrad, merge_adam)


def _dec_table(names, ptr_of):
    """(4-slot pointer table indexed by NSLAM_DEC_*, bit mask of `names`): slot of a name = ptr_of(name)."""
    tab, mask = (ctypes.c_void_p * 4)(), 0
    for name in names:
        d = ops.DEC_ID[name]
        mask |= 1 << d
        tab[d] = ptr_of(name)
    return tab, mask


def _live_tables(decs, names, idx, nl):
    """The tables of `names` into live_lists' (idx [decoders of the stage `decs`, N*S], nl [4]), and their mask."""
    ips, mask = _dec_table(names, lambda name: idx[decs.index(name)].data_ptr())
    return ips, _dec_table(names, lambda name: nl[ops.DEC_ID[name]:].data_ptr())[0], mask


@dataclasses.dataclass
class RayBatch:
    """The rays of one iteration: gather_rays' outputs, the sampler's z and, with live-point lists, live_lists'
    (per decoder of the stage the indices of its live points, and their counts by NSLAM_DEC_*)."""
    ro: torch.Tensor
    rd: torch.Tensor
    gd: torch.Tensor
    gc: torch.Tensor
    keep: torch.Tensor
    z: torch.Tensor
    live_idx: torch.Tensor = None
    n_live: torch.Tensor = None

    @property
    def live(self):
        return None if self.live_idx is None else (self.live_idx, self.n_live)

    def empty_like(self):
        return RayBatch(*(t if t is None else torch.empty_like(t) for t in vars(self).values()))


class PrefetchRing:
    """The two persistent ray batches that prefetching iterations alternate between (MappingEngine._parity:
    which one holds this iteration's): a hipGraph of an even and one of an odd iteration replay in turn with
    no copies.  A prefetched batch is valid only for its key and the very frames (images and poses, unmodified)
    it was gathered from: held by weak reference (identity — a new tensor at a freed one's address is not the
    same frame) and version counter; a call with other frames or poses changed in place draws its own batch.
    The version check cannot see a kernel's writes: a caller whose camera step can move the poses passes
    prefetch=False (Mapper: bundle adjustment's colour stage, where the cameras' lr is not 0).
    live_gen[k]: the (layout_gen, rows_gen) set k's live-point lists were formed at; a set whose lists are older
    than the slot maps (set_rows, bind_masks, Mapper._bind_frustum) keeps its rays and gets new lists before
    use.  A captured hipGraph of prefetching iterations replays the lists of its capture-time ordering: rebind
    rows only before a replay whose first iteration draws its own batch (Mapper.optimize_map's graphs do)."""

    def __init__(self):
        self.stream = None  # (survives drop(): a captured graph and the next one share it)
        self.drop()

    def drop(self):
        self.key, self.frames, self.sets, self.live_gen = None, [], [None, None], [None, None]

    def valid_for(self, key, ftens):
        return (self.key is not None and self.key == key and len(self.frames) == len(ftens)
                and all(r() is t and v == t._version for (r, v), t in zip(self.frames, ftens)))

    def start(self, key, ftens, first, gen):
        """A new run: `first` is its first iteration's batch (set 0); set 1 has the same shapes."""
        self.key, self.frames = key, [(weakref.ref(t), t._version) for t in ftens]
        self.sets, self.live_gen = [first, first.empty_like()], [gen, None]

    def current(self, parity):
        return self.sets[parity]

    def next(self, parity):
        return self.sets[1 - parity]

    def side_stream(self, eng):
        """The stream the next batch is drawn on, chosen on first use."""
        if self.stream is None:
            if eng.prefetch_stream == "lean" and eng.wgrad_first and eng.concurrent:
                # the mask-only launch's stream: the prefetch is done long before that stream's backward work.
                # In any other topology that side stream carries the weight-gradient branch
                if not eng._side:
                    eng._side.append(torch.cuda.Stream(eng.device))
                self.stream = eng._side[0]
            else:
                self.stream = torch.cuda.Stream(eng.device)
        return self.stream


class FlatDecoder:
    """A decoder's parameters re-bound as views of one flat float32 buffer (named_parameters
    order = the nslam_dec_grad layout) with a trailing zero slot, so packing is one gather into a
    persistent buffer and Adam sees one dense segment.  Parameter identity (and state_dict keys)
    is unchanged."""

    def __init__(self, dec):
        self.dec = dec
        self.packer = dec.packer()
        params = list(dec.parameters())
        n = sum(p.numel() for p in params)
        dev = params[0].device
        flat = torch.zeros(n + 1, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + k].view_as(p)
                off += k
        self.flat = flat
        self.param = flat[:n]                       # Adam segment
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.packed = torch.empty(self.packer.index.shape[0], dtype=torch.float32, device=dev)
        self.idx = self.packer.device_index(dev)
        # inverse of the packing gather: the (at most two) packed slots of each parameter, so Adam
        # can store an updated parameter straight into the packed copy (FusedAdam.set_mirror)
        idx = self.packer.index
        slots = np.full((n, 2), -1, dtype=np.int32)
        pos = np.nonzero(idx >= 0)[0]
        order = np.argsort(idx[pos], kind="stable")
        src, dst = idx[pos][order], pos[order]
        first = np.ones(src.size, dtype=bool)
        first[1:] = src[1:] != src[:-1]
        slots[src[first], 0] = dst[first]
        slots[src[~first], 1] = dst[~first]
        self.mirror_idx = torch.from_numpy(slots).to(dev)
        self.repack()

    def repack(self):
        torch.index_select(self.flat, 0, self.idx, out=self.packed)


class MappingEngine:
    """Fused mapping iterations over shared grids `c` (dict of [1,32,Z,Y,X] channels-last grids)
    and a NICE decoder stack, for the stage schedule of Mapper.optimize_map."""

    def __init__(self, nice, c, bound, n_strat, n_surf, lindisp=False, w_color=0.2, device="cuda", grid_grads=True,
                 rows=None):
        self.nice, self.c, self.bound = nice, c, bound
        self.n_strat, self.n_surf, self.lindisp, self.w_color = n_strat, n_surf, lindisp, w_color
        self.device = torch.device(device)
        names = [n for n in ("coarse", "middle", "fine", "color") if hasattr(nice, n + "_decoder")]
        self.decs = {n: FlatDecoder(nice.decoder(n)) for n in names}
        self.dec_bounds = {n: ops.bound_list(nice.decoder(n).bound) for n in names}
        self.oob = ops.bound_list(bound)
        self._saved = None  # ReLU masks of the last query_fwd (read by query_bwd)
        self._tape = None   # colour-decoder activation tape of the last query_fwd (ABI v9)
        self.occ_add = None  # middle occupancy of the last deferred-combine query_fwd
        self._draws = None   # (seed, ops.PixelDraws) of in-kernel pixel draws
        self.ring = PrefetchRing()  # the ray batches of a prefetching run of iterations
        self._parity = 0     # which of its two sets holds this iteration's batch
        self._side = []     # side streams of the concurrent decoder backward
        self.concurrent = True
        # every mask-only decoder backward as ONE launch (ABI v10); False: one nslam_query_bwd_decoder
        # launch per decoder (the library then runs a colour tape backward's two kernels in sequence)
        self.merge = True
        self._lean_ev = self._wg_ev = None  # persistent events (never destroyed mid-capture), made on first use
        knobs = env_knobs()
        self.wgrad_first, self.adam_merge = knobs["wgrad_first"], knobs["adam_merge"]
        self.prefetch_stream, self.live_points = knobs["prefetch_stream"], knobs["live_points"]
        self.rows_gen = 0  # bumped whenever a slot map is rewritten in place (bind_masks, Mapper._bind_frustum)
        for k, v in c.items():
            if not v.is_contiguous(memory_format=torch.channels_last_3d):
                raise ValueError(f"{k} must be channels-last (ops.channels_last)")
        self.grid_grads = grid_grads
        self.layout_gen = 0  # bumped by set_rows: consumers holding views of the buffers re-check it
        self.pad_rows = 1
        self.set_rows(rows)

    def set_rows(self, rows, pad_rows=None):
        """Grid-gradient layout.  rows=None: dense gradients (one flat buffer for every grid, so
        zeroing is a single memset).  rows={grid key: int32 voxel rows} (the frustum selection of
        Mapper.py:314-333, the FusedAdam group "rows"): those grids accumulate a COMPACT gradient
        [n_rows][32] in row-list order through a voxel→slot map (ABI v6 nslam_grid.slot); the
        scatter skips every other voxel, whose gradient the reference never forms (it optimises
        the masked vector, Mapper.py:394-401).  Adam then reads the compact rows directly and the
        ray-sharded exchange sums them as they are.
        pad_rows: every compact grid's rows and every decoder's gradient are padded (with entries
        nothing writes) to a multiple of pad_rows rows / elements, so a stage's gradient span splits
        into equal whole-row shards (distributed.ShardedAdamExchange: pad_rows = world size); None keeps
        the current padding.  Every call reallocates the gradient buffers and bumps self.layout_gen: an
        optimiser's compact Adam state and an exchange built for the old rows are invalid afterwards
        (the exchanges raise; rebuild both for the new rows)."""
        c = self.c
        pad = max(1, int(self.pad_rows if pad_rows is None else pad_rows))
        self.layout_gen += 1
        rup = lambda n: -(-n // pad) * pad  # noqa: E731
        drup = lambda n: -(-n // (32 * pad)) * 32 * pad  # noqa: E731  (decoders: whole rows per shard too)
        self.rows = dict(rows) if rows else {}
        self.pad_rows = pad
        self.slot = {}
        sizes = {}
        for k, v in c.items():
            n = self.rows[k].numel() if k in self.rows else v.numel() // 32  # rows (voxels)
            sizes[k] = 0 if not self.grid_grads else rup(n) * 32
        # one flat gradient buffer: the grids (c order), then the decoders' gradients (colour first, so
        # the colour stage's whole exchange payload — middle/fine/colour rows + colour decoder — is
        # one contiguous span of it: all-reduced in place, distributed.SparseGradExchange)
        dorder = [n for n in ("color", "fine", "middle", "coarse") if n in self.decs]
        gsum = sum(sizes.values())
        self.gall = torch.zeros(gsum + sum(drup(self.decs[n].param.numel()) for n in dorder), dtype=torch.float32,
                                device=self.device)
        self.gbuf = self.gall[:gsum]
        off = gsum
        self.dgrad_pad = {}  # decoder -> its gradient with the padding
        for n in dorder:
            k = self.decs[n].param.numel()
            self.decs[n].grad = self.gall[off:off + k]
            self.dgrad_pad[n] = self.gall[off:off + drup(k)]
            off += drup(k)
        self._clean = False  # every gradient the next iteration accumulates into is known zero
        self.ggrad, self.ggrad_pad, off = {}, {}, 0  # ggrad_pad: flat, with the padding
        for k, v in c.items():
            if not self.grid_grads:  # tracking: grids are constants (Tracker.py:138-141)
                continue
            Z, Y, X = v.shape[2:]
            if k in self.rows:
                r = self.rows[k]
                slot = torch.full((Z * Y * X,), -1, dtype=torch.int32, device=self.device)
                slot[r.long()] = torch.arange(r.numel(), dtype=torch.int32, device=self.device)
                self.slot[k] = slot
                self.ggrad[k] = self.gbuf[off:off + r.numel() * 32].view(-1, 32)
            else:
                self.ggrad[k] = self.gbuf[off:off + v.numel()].view(1, Z, Y, X, 32).permute(0, 4, 1, 2, 3)
            self.ggrad_pad[k] = self.gbuf[off:off + sizes[k]]
            off += sizes[k]

    def bind_masks(self, masks):
        """Per-call frustum selection on the device, without a host read-back and without moving any
        buffer (Mapper.optimize_map's fused path: Mapper.py:314-333 each call).

        masks: {grid key: bool [X, Y, Z] (mapper.frustum_mask) or None = every voxel}.  On the first call
        (or a new key set) every listed grid gets a compact gradient sized for its CAPACITY (all of its
        voxels) plus a persistent row list, slot map and live row count; every call then rewrites those
        three in place from the masks (a cumsum compaction).  Adam segments carry the live count (ABI v19
        nslam_adam_seg.n_live, FusedAdam group "n_live"), so nothing an iteration launches depends on the
        selection's size: a hipGraph captured for one call replays for the next.  The compact gradients
        stay zero between iterations (the backward writes only live rows, Adam zeroes every row it reads).
        Returns {grid key: live row count (device int64 [1])}."""
        keys = tuple(sorted(masks))
        if getattr(self, "_cap_keys", None) != keys:
            self._cap = {}
            rows = {}
            for k in keys:
                n = self.c[k].numel() // 32
                full = torch.empty(n + 1, dtype=torch.int32, device=self.device)  # [n]: the dummy target
                full[:n] = torch.arange(n, dtype=torch.int32, device=self.device)
                self._cap[k] = (full, torch.full((1,), n, dtype=torch.int64, device=self.device),
                                torch.arange(n, dtype=torch.int32, device=self.device))
                rows[k] = full[:n]
            self.set_rows(rows, pad_rows=1)
            self._cap_keys = keys
            self.gall.zero_()
            self._clean = True
        self.rows_gen += 1  # live-point lists formed from the old slot maps are stale
        for k in keys:
            full, n_live, ar = self._cap[k]
            n = ar.numel()
            m = masks[k]
            if m is None:
                full[:n].copy_(ar)
                self.slot[k].copy_(ar)
                n_live.fill_(n)
                continue
            m = m.permute(2, 1, 0).reshape(-1)  # [X, Y, Z] -> channels-last voxel order z*Y*X + y*X + x
            idx = torch.cumsum(m, 0, dtype=torch.int32) - 1
            self.slot[k].copy_(torch.where(m, idx, torch.full_like(idx, -1)))
            full.scatter_(0, torch.where(m, idx, torch.full_like(idx, n)).long(), ar)
            n_live.copy_(idx[-1:].to(torch.int64) + 1)
        return {k: self._cap[k][1] for k in keys}

    def live_rows(self, key):
        """(row list, live count) of a grid bound by bind_masks: the FusedAdam group's "rows" / "n_live"."""
        full, n_live, ar = self._cap[key]
        return full[:ar.numel()], n_live

    # -- query in ray form ---------------------------------------------------------------------
    def _cfg(self, stage, ro, rd, z, grid_grads, dec_grads, masks=None, tape=None):
        """The query descriptor of a ray batch; masks / tape: the forward's ReLU masks and activation tape
        (written by query_fwd, read by query_bwd; live_lists needs neither)."""
        decs = ops.DEC_FOR_STAGE[stage]
        meta = ops.QueryMeta(stage, decs, {n: self.decs[n].packer for n in decs},
                             {n: self.dec_bounds[n] for n in decs}, self.oob, None)
        pairs = [(None, None, None)] * 4
        for n in decs:
            key = _GRID_OF[n]
            gg = key in grid_grads
            pairs[ops.DEC_ID[n]] = (self.c[key], self.ggrad[key] if gg else None, self.slot.get(key) if gg else None)
        packed = {n: self.decs[n].packed for n in decs}
        dg = {n: self.decs[n].grad for n in decs if n in dec_grads}
        cfg = ops.fill_cfg(meta, pairs, packed, dg, False)
        cfg.rays_o, cfg.rays_d, cfg.z_vals, cfg.n_samples = ptr(ro), ptr(rd), ptr(z), z.shape[1]
        cfg.saved_masks = ptr(masks)
        cfg.act_tape = ptr(tape)
        return cfg

    def live_lists(self, stage, ro, rd, z, out=None):
        """(live_idx int32 [decoders of the stage, N*S], n_live int64 [4, by NSLAM_DEC_*]) of a ray batch
        against the current slot maps (nslam_live_points), on the current stream: per decoder the ascending
        indices of the points with a frustum-selected corner in its grid and their count.  Valid until a
        slot map changes (set_rows, bind_masks).  out: (live_idx, n_live) to write into."""
        decs = ops.DEC_FOR_STAGE[stage]
        n = z.numel()
        if out is None:
            out = (torch.empty(len(decs), n, dtype=torch.int32, device=z.device),
                   torch.zeros(4, dtype=torch.int64, device=z.device))
        idx, nl = out
        keys = tuple(_GRID_OF[d] for d in decs) if self.grid_grads else ()
        cfg = self._cfg(stage, ro, rd, z, keys, ())
        ips, nps, mask = _live_tables(decs, decs, idx, nl)
        wsb = lib().nslam_live_points_workspace_size(n)
        ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=z.device)
        with ops.span("live_points"):
            rc = lib().nslam_live_points(ctypes.byref(cfg), mask, None, n, ips, nps, ptr(ws), wsb, stream_ptr(z.device))
        check(rc, "nslam_live_points")
        return idx, nl

    def query_fwd(self, stage, ro, rd, z, defer_occ=False, tape=False):
        """raw [N*S, 4]; also saves the ReLU masks the backward of frozen decoders uses.
        defer_occ: raw[...,3] holds the fine occupancy only and self.occ_add the middle one (None
        when the stage has a single occupancy decoder) — render_loss(occ_add=...) adds it.
        tape: also keep the colour decoder's hidden activations for its weight-gradient backward."""
        n = z.numel()
        raw = torch.empty(n, 4, dtype=torch.float32, device=z.device)
        self._saved = torch.empty(lib().nslam_query_saved_size(n), dtype=torch.uint8, device=z.device)
        self._tape = None
        if tape and stage == "color":
            self._tape = torch.empty(lib().nslam_query_tape_size(n) // 4, dtype=torch.float32, device=z.device)
        cfg = self._cfg(stage, ro, rd, z, (), (), masks=self._saved, tape=self._tape)
        self.occ_add = ops.query_fwd_launch(cfg, None, n, raw, defer_occ=defer_occ)
        return raw

    def query_bwd(self, stage, ro, rd, z, g_raw, grid_grads, dec_grads, concurrent=None, pts_grad=False,
                  on_branch=None, pts_parts=False, ordered_branches=False, on_pts=None, live=None):
        """Backward into the engine's gradient buffers, as the independent launches ("branches", writing disjoint
        buffers) that backward_plan lists.  Here they are forked off the caller's stream, enqueued — each followed by
        the update that may start after it — and joined; with `concurrent` on separate streams (parallel branches of
        a captured hipGraph).
        pts_grad: also return d loss / d pts [N*S, 3] float64 (tracking, bundle adjustment): every decoder writes
        its share into its own buffer and the shares are summed afterwards (or returned as a list with pts_parts).
        on_branch(names, part): called on a branch's stream once what it updates is complete — "grids": the grids of
        the lean launch's decoders but the colour one; "all": the colour grid and the colour decoder, on the
        weight-gradient branch after it AND the lean launch (k_color_wgrad reads the colour grid: it is not
        rewritten before that kernel is done); "unit": a per-decoder launch's grid and parameters — the per-branch
        Adam of the mapping iteration.
        ordered_branches: the weight-gradient branch's on_branch starts only after the lean branch's on_branch work
        (not just the lean launch) — for collectives issued there on two communicators, which every rank must then
        run in the same order (distributed.ShardedAdamExchange).
        on_pts(parts): with pts_grad, called once every decoder's d/dpts share is written — on the lean launch's
        stream right after it when that launch forms all of them (bundle adjustment's camera gradient then runs
        beside the weight gradients, not after the join), else on the caller's stream after the join.
        live: live_lists() of this very batch and the current slot maps — the lean launch then runs each decoder's
        live points only (nslam_query_bwd_decoders_live; ignored with pts_grad, which needs every point)."""
        n = z.numel()
        self._clean = False
        live = None if pts_grad else live
        cfg = self._cfg(stage, ro, rd, z, grid_grads, dec_grads, masks=self._saved, tape=self._tape)
        cfg.need_pts_grad = int(bool(pts_grad))
        decs = list(ops.DEC_FOR_STAGE[stage])
        plan = backward_plan(decs, dec_grads, masks=self._saved is not None, tape=self._tape is not None, n=n,
                             merge=self.merge, wgrad_first=self.wgrad_first, adam_merge=self.adam_merge,
                             concurrent=self.concurrent if concurrent is None else concurrent,
                             has_on_branch=on_branch is not None, ordered=ordered_branches)
        gp = {d: torch.empty(n, 3, dtype=torch.float64, device=z.device) for d in decs} if pts_grad else None
        main = torch.cuda.current_stream(z.device)
        while len(self._side) < max(plan.streams):
            self._side.append(torch.cuda.Stream(z.device))
        streams = [main] + self._side[:max(plan.streams)]
        if plan.has_wgrad and self._lean_ev is None:
            self._lean_ev = torch.cuda.Event()
        if plan.merge_adam and self._wg_ev is None:
            self._wg_ev = torch.cuda.Event()
        wgrad_st = None
        with ops.span("query_bwd"):
            for st in streams[1:]:  # fork: every branch starts from the same point of the main stream
                st.wait_stream(main)
                for t in (ro, rd, z, g_raw, self._saved, self._tape) + (tuple(live) if live else ()):
                    if t is not None:
                        t.record_stream(st)
            for (kind, names), si in zip(plan.units, plan.streams):
                st = streams[si]
                with torch.cuda.stream(st):
                    if kind == "wgrad":
                        self._launch_wgrad(cfg, n, g_raw, st)
                        wgrad_st = st  # (its update waits for the lean launch: below)
                        if plan.merge_adam:
                            self._wg_ev.record(st)
                    elif kind == "lean":
                        self._launch_lean(cfg, decs, names, n, g_raw, st, gp, live)
                        if on_pts is not None and pts_grad and set(names) == set(decs):
                            on_pts([gp[d] for d in decs])
                            on_pts = None
                        if plan.has_wgrad and not ordered_branches:
                            self._lean_ev.record(st)
                        if on_branch is not None and plan.merge_adam:
                            # merged Adam: every update of the iteration in one call on this stream, once the
                            # weight-gradient branch (its slab reduction; its colour-grid gathers) is done
                            st.wait_event(self._wg_ev)
                            on_branch(list(names), part="all")
                        elif on_branch is not None:
                            # per-branch Adam: the grids of this launch — but the colour grid, which
                            # k_color_wgrad reads and which is updated on that branch once both are done.  A
                            # trainable decoder here (no points: no weight-gradient branch) still takes its step
                            own = [d for d in names if not (d == "color" and plan.has_wgrad)]
                            dec_here = not plan.has_wgrad and any(d in dec_grads for d in own)
                            if own:
                                on_branch(own, part="all" if dec_here else "grids")
                        if plan.has_wgrad and ordered_branches:
                            self._lean_ev.record(st)  # ordered variant: after this branch's on_branch work too
                    else:
                        self._launch_one(cfg, names[0], n, g_raw, st, gp)
                        if on_branch is not None:  # per-branch Adam of a per-decoder launch
                            on_branch(list(names), part="unit")
                if pts_grad and st is not main:
                    for name in names:
                        gp[name].record_stream(st)  # (allocated on the caller's stream)
            if plan.has_wgrad and on_branch is not None and not plan.merge_adam:
                # colour update: the colour grid and decoder, on the weight-gradient branch after its kernel and
                # the lean launch (no Adam may rewrite the grid while k_color_wgrad still gathers from it)
                with torch.cuda.stream(wgrad_st):
                    wgrad_st.wait_event(self._lean_ev)
                    on_branch(["color"], part="all")
            for st in streams[1:]:  # join
                main.wait_stream(st)
            if on_pts is not None and pts_grad:
                on_pts([gp[d] for d in decs])
        if not pts_grad:
            return None
        parts = [gp[d] for d in decs]  # (pts_parts: the per-decoder shares, for a consumer that sums them itself)
        return parts if pts_parts else functools.reduce(torch.Tensor.add_, parts)

    # -- the backward's launches: each enqueues one unit of backward_plan on `st`, none schedules an update --
    def _launch_wgrad(self, cfg, n, g_raw, st):
        wsb = lib().nslam_query_bwd_decoder_workspace_size(ctypes.byref(cfg), _lib.DEC_COLOR, n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=g_raw.device)
        with ops.span("query_bwd.color_wgrad"):
            rc = lib().nslam_color_wgrad(ctypes.byref(cfg), None, n, ptr(g_raw), ptr(ws), wsb, st.cuda_stream)
        check(rc, "nslam_color_wgrad")

    def _launch_lean(self, cfg, decs, names, n, g_raw, st, gp=None, live=None):
        """gp: {decoder: its d/dpts buffer} (plain form); live: live_lists() of the batch (live-point form)."""
        lc = _lib.NslamQueryCfg.from_buffer_copy(cfg)  # grids (and d/dpts) only
        for name in names:
            lc.dgrad[ops.DEC_ID[name]] = _lib.NslamDecGrad()
        with ops.span("query_bwd." + "+".join(names)):
            if live is not None:
                ips, nps, mask = _live_tables(decs, names, *live)
                rc = lib().nslam_query_bwd_decoders_live(ctypes.byref(lc), mask, None, n, ptr(g_raw), ips, nps,
                                                         st.cuda_stream)
            else:
                gps, mask = _dec_table(names, lambda name: ptr(gp[name]) if gp else None)
                rc = lib().nslam_query_bwd_decoders(ctypes.byref(lc), mask, None, n, ptr(g_raw), gps,
                                                    st.cuda_stream)
        check(rc, "nslam_query_bwd_decoders")

    def _launch_one(self, cfg, name, n, g_raw, st, gp=None):
        d = ops.DEC_ID[name]
        wsb = lib().nslam_query_bwd_decoder_workspace_size(ctypes.byref(cfg), d, n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=g_raw.device) if wsb else None
        with ops.span("query_bwd." + name):
            rc = lib().nslam_query_bwd_decoder(ctypes.byref(cfg), d, 0, None, n, ptr(g_raw),
                                               ptr(gp[name]) if gp else None, ptr(ws), wsb, st.cuda_stream)
        check(rc, "nslam_query_bwd_decoder")

    # -- one iteration ---------------------------------------------------------------------------
    def draws(self, seed, world=1, rank=0):
        """The in-kernel pixel draws (ops.PixelDraws) of stream `seed`, made on first use."""
        key = (seed, world, rank)
        if self._draws is None or self._draws[0] != key:
            self._draws = (key, ops.PixelDraws(seed, self.device, world, rank, with_max=world > 1))
        return self._draws[1]

    def grads_for(self, stage, trainable_decoders):
        """(grid keys, decoder names) that receive gradients in `stage` (Mapper.py:335-341)."""
        decs = ops.DEC_FOR_STAGE[stage]
        keys = tuple(_GRID_OF[n] for n in decs)
        return keys, tuple(n for n in decs if n in trainable_decoders)

    def adam_grads(self, stage, trainable_decoders):
        """{parameter: its gradient buffer} of the stage (compact grids: [n_rows, 32], no padding)."""
        keys, dnames = self.grads_for(stage, trainable_decoders)
        g = {self.c[k]: self.ggrad[k] for k in keys}
        g.update({self.decs[n].param: self.decs[n].grad for n in dnames})
        return g

    def iteration(self, stage, frames, pix, n_per, hw, intrinsics, optimizer, trainable_decoders=("color",),
                  gt_max=None, allreduce=None, use_gt_in_sampler=True, exchange=None, n_kept=None, seed=0,
                  world=1, rank=0, prefetch=False, post_bwd=None):
        """One mapping iteration; returns (ray_loss f64 [N], keep uint8 [N]) as device tensors.

        frames: [(depth, color, c2w)] of the window; pix: int64 [len(frames)*n_per] randint indices over the full
        image, or None: drawn in the gather kernel (ops.PixelDraws keyed by `seed`, advanced on the device — no host
        RNG work per hipGraph replay; with world > 1 every rank passes the same seed, gathers its slice of a global
        batch of n_per*world pixels per frame and gets the global batch's max(gt_depth) from the gather kernel — no
        collective before the sampler); hw = (H, W); intrinsics = (fx, fy, cx, cy); n_kept: optional device
        int64 [1] += kept rays.
        gt_max: callable(gt_depth) → device scalar for a ray-sharded job (all-reduced max);
        allreduce: callable(list of grads) run before Adam (ray sharding, dense);
        exchange: callable(grid keys, decoder names) run before Adam instead — the frustum-compacted exchange
        (distributed.SparseGradExchange).
        prefetch (device draws only): the pixel gather and sampler of the NEXT iteration run on a side stream while
        this one renders and back-propagates — they depend only on the frames and the device draw counter, not on
        the map (PrefetchRing: when a prefetched batch is valid).  Each call still draws, samples, renders and
        updates one batch; the first call draws its own batch first.  With prefetch the returned `keep` is a
        persistent buffer, valid until the next iteration() call (which overwrites it): clone it to keep it longer.
        post_bwd(g_pts parts, rays_o, rays_d, z): the backward also forms d loss / d pts (every decoder's share, a
        list of [N*S, 3] float64) and this runs as soon as they are written (on the mask-only launch's stream,
        beside the weight gradients; query_bwd on_pts) — bundle adjustment's camera gradients and camera step
        (Mapper.py:346-363, 503-504).  Its work is ordered before the next iteration by the join (it runs on a
        stream the join covers)."""
        keys, dnames = self.grads_for(stage, trainable_decoders)
        if exchange is not None and hasattr(exchange, "validate"):
            exchange.validate(self, keys, dnames)  # raises before anything of the iteration is enqueued
        # live-point lists: a mapping iteration without d/dpts whose grids (some of them) accumulate a
        # frustum-compacted gradient; they ride with the ray batch
        use_live = (self.live_points and post_bwd is None and self.grid_grads and self.merge
                    and any(k in self.slot for k in keys))
        rays = functools.partial(self._rays, stage, frames, pix, n_per, hw, intrinsics, n_kept=n_kept, gt_max=gt_max,
                                 draw=self.draws(seed, world, rank) if pix is None else None,
                                 use_gt=use_gt_in_sampler, use_live=use_live)
        side = None
        if prefetch and pix is None:
            key = (stage, n_per, hw, use_gt_in_sampler, seed, world, rank, use_live)
            batch, side = self._prefetched(rays, key, [t for f in frames for t in f], stage, use_live)
        else:
            batch = rays()
        ro, rd, z = batch.ro, batch.rd, batch.z
        mirror = hasattr(optimizer, "set_mirror")
        raw = self.query_fwd(stage, ro, rd, z, defer_occ=True, tape="color" in dnames)
        _, _, _, ray_loss, g_raw = ops.render_loss(raw, z, batch.gd, batch.gc, batch.keep, mode="mapper",
                                                   use_color=stage == "color", w_color=self.w_color,
                                                   occ_add=self.occ_add)
        if not self._clean:
            self.gall.zero_()  # grid and decoder gradients: one memset
        # Adam resets every gradient entry it reads.  With compact gradients for every grid of the
        # stage that is every entry the backward wrote, so the next iteration needs no memsets.
        clean = all(k in self.rows for k in keys)
        if mirror:  # Adam stores updated decoder parameters straight into their packed copies
            for n in dnames:
                d = self.decs[n]
                if d.param not in optimizer.mirrors:
                    optimizer.set_mirror(d.param, d.mirror_idx, d.packed)
        grads = self.adam_grads(stage, trainable_decoders)
        on_branch = None
        sharded = exchange is not None and hasattr(exchange, "branch")
        if sharded:
            # ZeRO-style exchange (distributed.ShardedAdamExchange): each backward branch's gradients are
            # reduce-scattered, this rank's shard stepped by Adam and the updated values all-gathered,
            # on that branch's stream as soon as it finishes — the exchange does the optimiser step
            def on_branch(names, part=None):
                exchange.branch(names, part, keys, dnames)
        elif exchange is None and allreduce is None and mirror:
            # one rank: each backward branch updates what it completes on its own stream — the lean
            # launch the middle / fine grid rows, the weight-gradient branch (once the lean launch is
            # done too) the colour grid and the colour decoder — so no Adam waits for the whole backward
            def on_branch(names, part=None):  # the decoders of one launch: one Adam call for their grids
                params = [self.c[_GRID_OF[nm]] for nm in names if _GRID_OF[nm] in keys]
                if part != "grids":  # ... and their own parameters
                    params += [self.decs[nm].param for nm in names if nm in dnames]
                sub = {p: grads[p] for p in params}
                if sub:
                    optimizer.step(grads=sub, zero_grad=clean)

        on_pts = (lambda parts: post_bwd(parts, ro, rd, z)) if post_bwd is not None else None
        self.query_bwd(stage, ro, rd, z, g_raw, keys, dnames, on_branch=on_branch, ordered_branches=sharded,
                       pts_grad=post_bwd is not None, pts_parts=True, on_pts=on_pts,
                       live=batch.live if use_live else None)
        if exchange is not None and not sharded:  # frustum-compacted all-reduce (distributed.SparseGradExchange)
            exchange(keys, dnames)
        elif allreduce is not None and not sharded:  # the grid gradients as one flat buffer, plus the decoder gradients
            allreduce([self.gbuf] + [self.decs[n].grad for n in dnames])
        if side is not None:  # join: the next call reads the prefetched set
            torch.cuda.current_stream(self.device).wait_stream(side)
        if on_branch is None:
            optimizer.step(grads=grads, zero_grad=clean)
        self._clean = clean and (not sharded or exchange.leaves_clean)
        if not mirror:
            for n in dnames:
                self.decs[n].repack()
        return ray_loss, batch.keep

    def _rays(self, stage, frames, pix, n_per, hw, intrinsics, *, draw, n_kept, gt_max, use_gt, use_live, out=None):
        """The iteration's RayBatch (into `out` when given): pixels → rays + inside mask, then the sampler
        (Mapper.py:457-484, Renderer.py:82-174), then the live-point lists, all on the current stream."""
        H, W = hw
        into = None if out is None else (out.ro, out.rd, out.gd, out.gc, out.keep)
        ro, rd, gd, gc, keep = ops.gather_rays(frames, pix, n_per, H, W, (0, H, 0, W), *intrinsics, self.bound,
                                               draw=draw, n_kept=n_kept, out=into)
        gsamp = gd if (use_gt and stage != "coarse") else None
        gm = None
        if gsamp is not None and draw is not None and draw.gt_max is not None:
            gm = draw.gt_max  # global batch max from the gather kernel
        elif gsamp is not None and gt_max is not None:
            gm = gt_max(gd)
        z = ops.sample_z(ro, rd, gsamp, self.bound, self.n_strat, self.n_surf, self.lindisp, gt_max=gm,
                         out=None if out is None else out.z)
        if out is None:
            out = RayBatch(ro, rd, gd, gc, keep, z)
        if use_live:
            out.live_idx, out.n_live = self.live_lists(stage, ro, rd, z, out=out.live)
        return out

    def _prefetched(self, rays, key, ftens, stage, use_live):
        """(this iteration's batch from the ring, the ring's side stream), after enqueuing the next one's there.
        A ring of another key or other frames is started over: this call then draws its own batch first."""
        ring = self.ring
        gen = (self.layout_gen, self.rows_gen)
        if not ring.valid_for(key, ftens):
            ring.start(key, ftens, rays(), gen)
            self._parity = 0
        par = self._parity
        cur, nxt = ring.current(par), ring.next(par)
        self._parity ^= 1
        if use_live and ring.live_gen[par] != gen:
            # (ordered after the side stream's writes of this set by the previous iteration's join)
            self.live_lists(stage, cur.ro, cur.rd, cur.z, out=cur.live)
            ring.live_gen[par] = gen
        side = ring.side_stream(self)
        side.wait_stream(torch.cuda.current_stream(self.device))  # the previous iteration's backward has released `nxt`
        with torch.cuda.stream(side):
            rays(out=nxt)  # the next iteration's batch, beside this iteration's render + backward
        ring.live_gen[1 - par] = gen
        return cur, side

    def drop_prefetch(self):
        """Forget the prefetched batch: the next prefetching iteration draws its own first."""
        self.ring.drop()


class TrackingEngine:
    """Tracker.optimize_cam_in_batch (src/Tracker.py:71-128) on the HIP kernels, without host
    synchronisation: one camera iteration is

        c2w = get_camera_from_tensor(cam)              (autograd on the 7-vector only)
        pixels → rays + inside mask                    nslam_gather_rays
        sampler, decoders (ray form, ReLU masks saved) nslam_sample_rays, nslam_query_fwd_ws
        compositing + tracker loss + their backward    nslam_render_loss (mode TRACKER, median)
        d loss / d pts, frozen decoders                nslam_query_bwd_decoder (mask-only, 3 branches)
        pts → rays → c2w → cam                         nslam_cam_grad_step (closed form, include/nslam.h),
        Adam on the camera, loss sum, best pose          whose last workgroup also steps the camera (FusedAdam's
                                                       update, device step count) and keeps the best pose

    so `iters` iterations can be captured in one hipGraph.  Grids and decoders are constants
    (Tracker.py:138-141): no grid or weight gradients are formed.  As in the reference, dropped
    rays (inside mask) carry no loss and the handle_dynamic median is over kept rays only.
    """

    def __init__(self, nice, c, bound, n_strat, n_surf, hw, intrinsics, ignore_edge=(20, 20), w_color=0.5,
                 handle_dynamic=True, use_color=True, device="cuda"):
        self.eng = MappingEngine(nice, c, bound, n_strat, n_surf, device=device, grid_grads=False)
        self.bound, self.n_strat, self.n_surf = bound, n_strat, n_surf
        self.H, self.W = hw
        self.intr = intrinsics
        he, we = ignore_edge
        self.window = (he, self.H - he, we, self.W - we)
        self.w_color, self.handle_dynamic, self.use_color = w_color, handle_dynamic, use_color
        self.device = torch.device(device)
        self._c2w = self._cam_ws = self._cam_ticket = self._loss = None  # (_buffers)
        # ABI v15 nslam_cam_grad_parts: the frozen decoders' d/dpts buffers summed inside a
        # multi-workgroup camera-gradient kernel (no torch adds, no single-workgroup reduction)
        self.cam_parts = True
        # ABI v23 nslam_cam_grad_step: with a FusedAdam over the camera alone, its step, the loss sum and the
        # best pose run in the camera-gradient launch's last workgroup (two launches fewer per iteration)
        self.cam_tail = True

    def n_window(self):
        h0, h1, w0, w1 = self.window
        return (h1 - h0) * (w1 - w0)

    @staticmethod
    def _tail_ok(optimizer, cam):
        """The fused camera tail applies to a FusedAdam stepping exactly this dense camera tensor."""
        if not isinstance(optimizer, ops.FusedAdam):
            return False
        ps = [p for g in optimizer.param_groups for p in g["params"]]
        return (len(ps) == 1 and ps[0] is cam and optimizer.param_groups[0].get("rows") is None
                and cam not in optimizer.mirrors and cam.is_contiguous() and cam.numel() == 7)

    def iteration(self, cam, depth, color, pix, optimizer, n=None, seed=0, best=None, lr_quat=None,
                  best_before_step=False):
        """One camera iteration on frame (depth [H,W], color [H,W,3]) with pixel draws `pix`
        (int64 [n], select_uv indices into the edge-cropped window), or pix=None: n pixels drawn inside
        the gather kernel (uniform over the window, stream `seed`; capturable in a hipGraph).  cam: [7]
        leaf tensor whose .grad the optimizer reads.  Returns the loss (device f64 scalar) of the pose
        BEFORE the step: the kept rays' losses summed in a fixed order (nslam_loss_sum_best; a buffer the
        next call overwrites), which with best = (best_loss, best_cam) also keeps the best pose
        (Tracker.py:245-247) in the same launch.
        lr_quat / best_before_step: the reference's seperate_LR loop (Tracker.py:202-247) — the quaternion
        (elements 0..3) steps with lr_quat, the translation with the optimizer's lr, and the best pose kept is
        the camera BEFORE the step (that loop rebuilds camera_tensor from its two leaves before each
        iteration).  Both live in the fused camera tail (nslam_cam_grad_step_lr2) only: with cam_tail or
        cam_parts off, or an optimizer the tail does not apply to, the call raises, it does not step with one
        rate."""
        tail = self.cam_parts and self.cam_tail and self._tail_ok(optimizer, cam)
        if (lr_quat is not None or best_before_step) and not tail:
            raise RuntimeError("TrackingEngine.iteration: lr_quat / best_before_step need the fused camera tail "
                               "(cam_parts and cam_tail on, a FusedAdam over the camera 7-vector alone)")
        n = pix.numel() if pix is not None else int(n)
        draw = self.eng.draws(seed) if pix is None else None
        # get_camera_from_tensor inside the gather (ABI v21), which also leaves the pose in c2w for the
        # camera gradient
        c2w = self._buffers(cam)
        ro, rd, gd, gc, keep = ops.gather_rays([(depth, color, c2w, cam.detach())], pix, n, self.H, self.W,
                                               self.window, *self.intr, self.bound, draw=draw)
        z = ops.sample_z(ro, rd, gd, self.bound, self.n_strat, self.n_surf)
        # the fine + middle occupancy sum is formed by the loss kernel as it reads raw (no combine pass)
        raw = self.eng.query_fwd("color", ro, rd, z, defer_occ=True)
        _, _, _, ray_loss, g_raw = ops.render_loss(raw, z, gd, gc, keep, mode="tracker", use_color=self.use_color,
                                                   handle_dynamic=self.handle_dynamic, w_color=self.w_color,
                                                   occ_add=self.eng.occ_add)
        g_pts = self.eng.query_bwd("color", ro, rd, z, g_raw, (), (), pts_grad=True, pts_parts=self.cam_parts)
        bl, bc = (None, None) if best is None else (best[0], best[1])
        if tail:  # camera gradient, Adam step, loss sum and best pose in one launch (ABI v23)
            ex, ex2, stp = optimizer.state_of(cam)
            adam = (ex, ex2, stp, optimizer.group_of(cam)["lr"], *optimizer.betas, optimizer.eps)
            ops.cam_grad_step(cam.detach(), c2w, g_pts, z, rd, cam.grad, self._cam_ws, self._cam_ticket, adam,
                              ray_loss, self._loss, bl, bc, lr_quat=lr_quat, best_before_step=best_before_step)
            return self._loss
        elif self.cam_parts:  # the decoders' d/dpts shares summed inside the multi-workgroup cam_grad (ABI v15)
            ops.cam_grad_parts(cam.detach(), c2w, g_pts, z, rd, cam.grad, self._cam_ws, self._cam_ticket)
        else:  # the shares summed by torch; the whole pts → rays → c2w → 7-vector chain in one launch
            ops.cam_grad(cam.detach(), c2w, g_pts, z, rd, cam.grad)
        optimizer.step()
        # the loss of the pose before the step (its rays' losses) and, with `best`, the best-pose update in
        # one launch: the candidate is the 7-vector right after that step, as the reference keeps it
        # (optimize_cam_in_batch steps before Tracker.py:245-247 compares)
        ops.loss_sum_best(ray_loss, self._loss, bl, cam.detach(), bc)
        return self._loss

    def _buffers(self, cam):
        """The pose buffer; with it, on the first call, the iteration's other persistent buffers: the camera
        gradient's workspace and ticket, the loss (device f64 scalar, overwritten by the next call), cam.grad."""
        if self._c2w is None:
            self._c2w = torch.empty(3, 4, dtype=torch.float32, device=cam.device)
            self._cam_ws = torch.zeros(ops.CAM_GRAD_WS_DOUBLES, dtype=torch.float64, device=cam.device)
            self._cam_ticket = torch.zeros(1, dtype=torch.int32, device=cam.device)
            self._loss = torch.empty((), dtype=torch.float64, device=cam.device)
        if cam.grad is None:
            cam.grad = torch.empty_like(cam)
        return self._c2w


def frustum_rows(mask_xyz: torch.Tensor) -> torch.Tensor:
    """int32 voxel rows (z*Y*X + y*X + x, channels-last) of a get_mask_from_c2w mask [X, Y, Z]."""
    m = mask_xyz.permute(2, 1, 0).reshape(-1)
    return torch.nonzero(m).reshape(-1).to(torch.int32)
