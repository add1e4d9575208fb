"""The mapping / tracking iteration's own launches of csrc/nslam_mapping.hip: pixel gather, row transfer, Adam."""
import ctypes

import torch

from . import span
from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from ._check import bound_list


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
    want = ((n, 3, torch.float32), (n, 3, torch.float32), (n, torch.float32), (n, 3, torch.float32), (n, torch.uint8))
    if out is not None:
        ro, rd, gd, gc, keep = out
        for t, w in zip(out, want):
            if tuple(t.shape) != tuple(w[:-1]) or t.dtype != w[-1] or not t.is_contiguous():
                raise ValueError("out tensors must match gather_rays' outputs")
    else:
        ro, rd, gd, gc, keep = (torch.empty(w[:-1], dtype=w[-1], device=dev) for w in want)
    h0, h1, w0, w1 = window
    if bound is not None:
        lo, hi = bound_list(bound)
        blo, bhi = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*hi)
    else:
        blo = bhi = None
    with span("gather_rays"):
        rc = lib().nslam_gather_rays(arr, nf, n_per, ptr(pix), H, W, h0, h1, w0, w1, fx, fy, cx, cy, blo, bhi,
                                     ptr(ro), ptr(rd), ptr(gd), ptr(gc), ptr(keep),
                                     ctypes.byref(draw.struct) if (pix is None) else None,
                                     ptr(n_kept), stream_ptr(dev))
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


def rows_pack(grid_flat, rows, tail, out):
    """nslam_rows_pack: out = [grid_flat.view(-1, 32)[rows], tail] (either part may be None)."""
    n = rows.numel() if rows is not None else 0
    nt = tail.numel() if tail is not None else 0
    with span("rows_xfer"):
        rc = lib().nslam_rows_pack(ptr(grid_flat) if n else None, ptr(rows) if n else None, n, 32, ptr(tail), nt,
                                   ptr(out), stream_ptr(out.device))
    check(rc, "nslam_rows_pack")


def rows_unpack(buf, rows, grid_flat, tail):
    """nslam_rows_unpack: the inverse of rows_pack."""
    n = rows.numel() if rows is not None else 0
    nt = tail.numel() if tail is not None else 0
    with span("rows_xfer"):
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

    def _launch(self, segs, key, zero_grad, too_many, in_capture):
        """nslam_adam_step over the NslamAdamSeg structs segs, with the step ticket kept under key."""
        if not segs:
            return
        if len(segs) > _lib.ADAM_MAX_SEGS:
            raise ValueError(f"at most {_lib.ADAM_MAX_SEGS} {too_many}")
        ticket = self._tickets.get(key)
        if ticket is None:
            # a ticket made during capture would come from the graph's private pool with its zero-fill
            # baked into the graph: every subset must step once eagerly first
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"FusedAdam: first step of a {in_capture}")
            ticket = self._tickets[key] = torch.zeros(1, dtype=torch.int32, device=self.device)
        arr = (_lib.NslamAdamSeg * len(segs))(*segs)
        b1, b2 = self.betas
        with span("adam"):
            rc = lib().nslam_adam_step(arr, len(segs), b1, b2, self.eps, int(bool(zero_grad)), ptr(ticket),
                                       stream_ptr(self.device))
        check(rc, "nslam_adam_step")

    @torch.no_grad()
    def step(self, grads=None, zero_grad=False):
        segs = self.segments(grads)
        self._launch([s for s, _, _ in segs], tuple(id(p) for _, p, _ in segs), zero_grad,
                     "parameter tensors per step (flatten the decoders)",
                     "parameter subset inside graph capture; run one eager step of it before capturing")

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
        self._launch(segs, key, zero_grad, "segments per step", "segment set inside graph capture; run one eager step")

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
