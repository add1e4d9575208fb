"""Seeded inputs and float64 references for the per-ray kernels at their edges (test infrastructure; plain torch
on the CPU, no device code).  Used by test_ray_edges_cpu.py (the input conditions, on the reference alone) and
test_gpu_ray_edges.py (the kernels).

The references are the restatements the suite already pins to the reference implementation:
oracle.nslam_oracle.sample_z / composite / tracker_loss / mapper_loss and imap_ref.composite_density.  Every
compositing or loss case carries the result of that code in float64 (`ref`: what float32 arithmetic
approximates) and in the reference's own float32 (`f32`); their difference (`floor`) is one float32
evaluation's error for that quantity.  No floor is measured from a kernel.

Scene of the compositing cases.  Rows cycle through four kinds (period 8: transparent, surface, saturated,
surface, transparent, surface, empty, surface):
  transparent  occupancy logits N(-0.55, 0.05^2): alpha ~ 0.004, a third of the light left after 256 samples;
  surface k0   transparent before k0, then the ramp 0.08 * min(k - k0 + 1, 40); k0 cycles over the chunk
               boundaries, so the carried transmittance and the backward's cross-chunk tail decide the answer;
  saturated    logits +3: alpha rounds to 1.0f, the factor is 1e-10 and the transmittance underflows;
  empty        logits -3.
"""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imap_ref  # noqa: E402
from oracle import nslam_oracle as orc  # noqa: E402

# the project's bars (already in tests/): compositor outputs max-abs, g_raw rel-L2, the loss relative
BAR_OUT, BAR_GRAD, BAR_LOSS = 1e-6, 1e-5, 1e-6


def bar(project, floor):
    """max(project bar, 4 x floor): two independent float32 evaluations differ by up to about twice one
    evaluation's error."""
    return max(project, 4.0 * floor)


def rel_l2(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def max_abs(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max()) if a.numel() else 0.0


def chunk_rel_l2(a, b):
    """rel-L2 of g_raw [N,S,4] per 64-sample chunk: a wrong later chunk must not hide behind chunk 0."""
    return [rel_l2(a[:, c:c + 64], b[:, c:c + 64]) for c in range(0, b.shape[1], 64)]


def chunk_norms(b):
    return [float(b[:, c:c + 64].double().norm()) for c in range(0, b.shape[1], 64)]


# ---------------------------------------------------------------------------------------------- sampler
BOUND = torch.tensor([[-2.0, 2.5], [-1.5, 3.0], [-1.0, 2.0]], dtype=torch.float64)
SAMPLE_COUNTS = [(1, 1), (2, 0), (32, 16), (48, 16), (49, 16), (64, 0), (65, 0), (128, 0), (128, 64)]
N_WAVE, N_SERIAL, N_MAX_GT = 37, 131, 8193  # 37 % 4 != 0; 131 = a workgroup of 128 and one of 3; > kLocalMaxRays
GT_MAX = 7.5  # the batch maximum a ray-sharded caller passes in (above every gt of the batch)


def sampler_n(n_strat, n_surf, with_gt):
    """Rays of a case: 37 where the wave form runs (S <= 64), 131 where the serial one does."""
    return N_WAVE if n_strat + (n_surf if with_gt else 0) <= 64 else N_SERIAL


@functools.lru_cache(maxsize=None)
def sampler_rays(n, all_zero=False):
    """(rays_o, rays_d, gt_depth) float32.  Row i is of kind i % 6:
      0, 5  origin inside the bound, any direction;
      1     origin outside (beyond +x) pointing away: far_bb < 0, far clamps to 0, the stratified list descends;
      2     one direction component exactly 0.0;   3  one exactly -0.0;   4  two zero components (0.0 and -0.0).
    gt_depth is 0 on every fifth ray (all_zero: on every ray, so the surface list descends too)."""
    g = torch.Generator().manual_seed(300 + n)
    lo, hi = BOUND[:, 0].float(), BOUND[:, 1].float()
    o = lo + (hi - lo) * (0.1 + 0.8 * torch.rand(n, 3, generator=g))
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    kind = torch.arange(n) % 6
    out = kind == 1
    o[out, 0] = hi[0] + 0.5 + torch.rand(n, generator=g)[out]
    d[out, 0] = d[out, 0].abs() + 0.2
    d[kind == 2, 1] = 0.0
    d[kind == 3, 2] = -0.0
    d[kind == 4, 0] = 0.0
    d[kind == 4, 1] = -0.0
    gt = 0.5 + 3.0 * torch.rand(n, generator=g)
    gt[::5] = 0.0
    if all_zero:
        gt = torch.zeros(n)
    return o, d, gt


@functools.lru_cache(maxsize=None)
def sampler_case(n_strat, n_surf, with_gt, lindisp, n=None, gt_max=False, all_zero=False):
    """inputs and the oracle's z [n, S] float64 (compared bit for bit: the sampler has no noise floor)."""
    n = sampler_n(n_strat, n_surf, with_gt) if n is None else n
    o, d, gt = sampler_rays(n, all_zero)
    gm = torch.tensor(GT_MAX) if gt_max else None
    z = orc.sample_z(o, d, gt if with_gt else None, BOUND, n_strat, n_surf, lindisp=lindisp, gt_max=gm)
    far = None
    if with_gt:  # the clamped far of the oracle (rows with far == 0 and lindisp hold inf * 0 at t = 0)
        gmax = torch.max(gt) if gm is None else gm
        far = torch.clamp(orc.far_bound(o, d, BOUND) + 0.01, 0, gmax * 1.2)
    return dict(rays_o=o, rays_d=d, gt=gt if with_gt else None, gt_max=gm, z=z, far=far,
                n_strat=n_strat, n_surf=n_surf, lindisp=lindisp)


def sampler_cases():
    """Every SAMPLE_COUNTS entry with and without gt_depth, lindisp off and on, as sampler_case keyword dicts.
    The counts: the smallest ones, the production 32 + 16, S = 64 / 65 (the last wave form, the first serial
    one) reached with and without surface samples, and the limits kMaxS0 = 128 and kMaxS1 = 64."""
    return [dict(n_strat=a, n_surf=b, with_gt=g, lindisp=l) for a, b in SAMPLE_COUNTS for g in (True, False)
            for l in (False, True)]


EXTRA_SAMPLER = {
    # wave form above kLocalMaxRays without gt_max: the memset + k_max_gt launch
    "max_gt_launch": dict(n_strat=32, n_surf=16, with_gt=True, lindisp=False, n=N_MAX_GT),
    # serial form with the caller's batch maximum: k_key_of
    "serial_gt_max": dict(n_strat=49, n_surf=16, with_gt=True, lindisp=False, gt_max=True),
    "wave_gt_max": dict(n_strat=32, n_surf=16, with_gt=True, lindisp=False, gt_max=True),
    # every gt_depth 0: max is 0, far is 0, the surface list 0.001 -> 0 descends
    "all_zero_wave": dict(n_strat=32, n_surf=16, with_gt=True, lindisp=False, all_zero=True),
    "all_zero_serial": dict(n_strat=128, n_surf=64, with_gt=True, lindisp=False, all_zero=True),
}


# ---------------------------------------------------------------------------------------------- compositors
COMPOSITE_S = [1, 2, 48, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256]
N_COMPOSITE = 51  # 51 % 4 != 0: the last workgroup is partly empty
# Density mode has no S = 1 reference: raw2outputs_nerf_color sizes the trailing 1e10 from a slice of the
# (empty) z differences, so it composites zero samples and returns 0 for everything (common.py:224-227).
# One opaque sample at dist 1e10, which the kernels' arithmetic would give, is not that answer, so
# nslam_composite_density_fwd / _bwd refuse S = 1 (test_compositors_refuse_unsupported_sample_counts).
DENSITY_S = COMPOSITE_S[1:]
TRANSPARENT, SURFACE, SATURATED, EMPTY = 0, 1, 2, 3
ALL_KINDS = (TRANSPARENT, SURFACE, SATURATED, SURFACE, TRANSPARENT, SURFACE, EMPTY, SURFACE)
SEMI_KINDS = (TRANSPARENT, SURFACE)  # rows with a spread-out weight distribution (var well above 0)


def surface_starts(S):
    ks = []
    for k in (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, S - 2, S - 1):
        if 0 <= k < S and k not in ks:
            ks.append(k)
    return ks


def scene(n, S, seed, kinds=ALL_KINDS):
    """(logits [n,S] f32, colours [n,S,3] f32, z [n,S] f64 ascending in [0.1, 4.1], kind [n], k0 [n])."""
    g = torch.Generator().manual_seed(seed)
    logit = -0.55 + 0.05 * torch.randn(n, S, generator=g)
    kind = torch.tensor([kinds[i % len(kinds)] for i in range(n)])
    k0 = torch.full((n,), -1)
    starts, j = surface_starts(S), 0
    k = torch.arange(S)
    for i in range(n):
        if kind[i] == SURFACE:
            k0[i] = starts[j % len(starts)]
            j += 1
            ramp = 0.08 * torch.clamp(k - k0[i] + 1, max=40).float()
            logit[i] = torch.where(k >= k0[i], ramp, logit[i])
        elif kind[i] == SATURATED:
            logit[i] = 3.0
        elif kind[i] == EMPTY:
            logit[i] = -3.0
    rgb = torch.rand(n, S, 3, generator=g)
    steps = 0.5 + torch.rand(n, S, generator=g, dtype=torch.float64)  # spacings within a factor 3 of each other
    z = 0.1 + 4.0 * torch.cumsum(steps, 1) / steps.sum(1, keepdim=True)
    return logit, rgb, z, kind, k0


def cotangents(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64),
            torch.randn(n, 3, generator=g))


def _occupancy_eval(raw, z, cots, dtype):
    """oracle.composite and its VJP with raw in `dtype` (float32: the reference's own arithmetic)."""
    r = raw.detach().to(dtype).requires_grad_(True)
    depth, var, rgb, w = orc.composite(r, z)
    gd, gv, gc = cots
    (g_raw,) = torch.autograd.grad((depth * gd).sum() + (var * gv).sum() + (rgb * gc.to(dtype)).sum(), r)
    trans = w.detach().double() / torch.sigmoid(10 * r.detach().double()[..., 3])  # exclusive transmittance
    return dict(depth=depth.detach(), var=var.detach(), rgb=rgb.detach(), g_raw=g_raw, trans=trans)


def _floors(ref, f32, outs, grads, whole=()):
    fl = {k: max_abs(f32[k], ref[k]) for k in outs}
    fl.update({k: max(chunk_rel_l2(f32[k], ref[k])) for k in grads})
    fl.update({k: rel_l2(f32[k], ref[k]) for k in whole})
    return fl


@functools.lru_cache(maxsize=None)
def composite_case(S, n=N_COMPOSITE):
    logit, rgb, z, kind, k0 = scene(n, S, 1000 + S)
    raw = torch.cat([rgb, logit[..., None]], -1)
    cots = cotangents(n, 2000 + S)
    ref = _occupancy_eval(raw, z, cots, torch.float64)
    f32 = _occupancy_eval(raw, z, cots, torch.float32)
    return dict(raw=raw, z=z, cots=cots, kind=kind, k0=k0, ref=ref, f32=f32,
                floor=_floors(ref, f32, ("depth", "var", "rgb"), ("g_raw",)))


def _density_eval(raw, z, rays_d, cots, dtype):
    r = raw.detach().to(dtype).requires_grad_(True)
    d = rays_d.detach().to(dtype).requires_grad_(True)
    depth, var, rgb, w = imap_ref.composite_density(r, z, d, dtype)
    gd, gv, gc = cots
    g_raw, g_d = torch.autograd.grad((depth * gd).sum() + (var * gv).sum() + (rgb * gc.to(dtype)).sum(), (r, d))
    return dict(depth=depth.detach(), var=var.detach(), rgb=rgb.detach(), weights=w.detach(), g_raw=g_raw,
                g_rays_d=g_d)


@functools.lru_cache(maxsize=None)
def density_case(S, n=N_COMPOSITE):
    """The occupancy scene with its alphas mapped to densities: sigma = -log(1 - alpha) / (dist |rays_d|), so
    the transmittance along every ray is the occupancy scene's (but for the last sample, whose dist is 1e10).
    Empty rows get sigma = -0.7: the relu's closed side.  |rays_d| is between 0.5 and 2."""
    logit, rgb, z, kind, k0 = scene(n, S, 3000 + S)
    g = torch.Generator().manual_seed(3500 + S)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(n, 1, generator=g))
    dist = torch.cat([(z[:, 1:] - z[:, :-1]).float().double(), torch.full((n, 1), 1e10, dtype=torch.float64)], 1)
    dist = dist * d.double().norm(dim=1, keepdim=True)
    sigma = -torch.log1p(-torch.sigmoid(10 * logit.double())) / dist
    sigma[kind == EMPTY] = -0.7
    # the last sample's dist is 1e10: a partial alpha there needs sigma ~ 1e-10, whose gradient (~ 1e10) would
    # be the whole norm of the last chunk's g_raw.  Every row but the empty ones ends in an opaque sample.
    sigma[kind != EMPTY, -1] = 0.5
    raw = torch.cat([rgb, sigma.float()[..., None]], -1)
    cots = cotangents(n, 4000 + S)
    ref = _density_eval(raw, z, d, cots, torch.float64)
    f32 = _density_eval(raw, z, d, cots, torch.float32)
    alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3].double()) * dist)
    trans = torch.cumprod(torch.cat([torch.ones(n, 1, dtype=torch.float64), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    ref["trans"] = trans
    return dict(raw=raw, z=z, rays_d=d, cots=cots, kind=kind, k0=k0, ref=ref, f32=f32,
                floor=_floors(ref, f32, ("depth", "var", "rgb", "weights"), ("g_raw",), ("g_rays_d",)))


# ---------------------------------------------------------------------------------------------- render loss
# (S, n): 5 rays: the threshold formed inside pass 2, one partial workgroup; 257: the first n above
# kInlineMedian (the median launch, rank selection); 1030 > the 1024 threads of the median workgroup: bitonic sort
LOSS_CASES = [(48, 5), (65, 257), (130, 1030)]
LOSS_MODES = {  # name: (mode, use_color, handle_dynamic, w_color)
    "mapper_color": ("mapper", True, False, 0.2),
    "mapper_depth": ("mapper", False, False, 0.2),
    "tracker_dynamic": ("tracker", True, True, 0.5),
    "tracker_static": ("tracker", True, False, 0.5),
}


def _loss_eval(raw, z, gt_depth, gt_color, keep, mode, dtype):
    """oracle.composite then oracle.mapper_loss / tracker_loss on the kept rays, under autograd, with raw (and
    what follows from it in the reference's float32) in `dtype`.  Never ops.composite."""
    kind, use_color, hd, w = LOSS_MODES[mode]
    r = raw.detach().to(dtype).requires_grad_(True)
    depth, var, rgb, _ = orc.composite(r, z)
    k = keep.bool()
    gd = gt_depth.to(dtype)[k]  # float32 in the reference (gt - depth promotes to float64)
    gc = gt_color.to(dtype)[k]
    resid = (torch.abs(gt_depth.to(dtype) - depth) / torch.sqrt(var + 1e-10)).detach()
    if not bool(k.any()):  # (median of nothing raises in torch; the loss over no ray is 0)
        loss = depth.sum() * 0.0
    elif kind == "mapper":
        loss = orc.mapper_loss(depth[k], rgb[k], gd, gc, "color" if use_color else "fine", w_color=w)
    else:
        loss = orc.tracker_loss(depth[k], var[k], rgb[k], gd, gc, handle_dynamic=hd, w_color=w, use_color=use_color)
    (g_raw,) = torch.autograd.grad(loss, r)
    return dict(depth=depth.detach(), var=var.detach(), color=rgb.detach(), loss=loss.detach().double(),
                g_raw=g_raw, resid=resid)


@functools.lru_cache(maxsize=None)
def loss_case(S, n, mode, keep_none=False):
    """Mapper cases use every row kind; tracker cases only transparent and surface rows (var >= 1e-4: with
    var ~ 0 the residual |gt - depth| / sqrt(var) has a float32 floor of 2e-3).

    Ray i is an outlier when i % 9 == 0 (gt_depth far behind the rendered depth: the dynamic mask removes it),
    has gt_depth == 0 when i % 7 == 3, and is masked out by keep when i % 5 == 2.  gt values sit at least 1e-3
    from the rendered ones (the L1 kinks) and the tracker's residuals far from 10 x their median.

    The occupancy channel is the float32 sum of two float32 parts (`occ_a`, `occ_b`): the kernel is given
    either the sum, or occ_a in raw and occ_b as occ_add; the reference always sees the sum."""
    tracker = LOSS_MODES[mode][0] == "tracker"
    logit, rgb, z, kind, k0 = scene(n, S, 5000 + S + (7 if tracker else 0), SEMI_KINDS if tracker else ALL_KINDS)
    occ_a = logit * 0.625
    occ_b = logit - occ_a
    raw = torch.cat([rgb, (occ_a + occ_b)[..., None]], -1)
    with torch.no_grad():
        d64, v64, c64, _ = orc.composite(raw.double(), z)
    g = torch.Generator().manual_seed(6000 + S)
    i = torch.arange(n)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    u = torch.rand(n, generator=g, dtype=torch.float64)
    if tracker:  # offsets in units of the ray's own uncertainty: r in [0.2, 0.8], outliers r in [40, 60]
        sd = torch.sqrt(v64 + 1e-10)
        off = sign * (0.2 + 0.6 * u) * sd
        far = (40.0 + 20.0 * u) * sd
    else:
        off = sign * (0.01 + 0.05 * u)
        far = 1.5 + u
    off = torch.where(d64 + off < 0.05, off.abs(), off)
    gt = torch.where(i % 9 == 0, d64 + far, d64 + off).float()
    gt[i % 7 == 3] = 0.0
    csign = torch.where(torch.rand(n, 3, generator=g) < 0.5, -1.0, 1.0).double()
    gt_color = (c64 + csign * (0.01 + 0.3 * torch.rand(n, 3, generator=g, dtype=torch.float64))).float()
    keep = torch.zeros(n, dtype=torch.uint8) if keep_none else (i % 5 != 2).to(torch.uint8)
    ref = _loss_eval(raw, z, gt, gt_color, keep, mode, torch.float64)
    f32 = _loss_eval(raw, z, gt, gt_color, keep, mode, torch.float32)
    floor = _floors(ref, f32, ("depth", "var", "color"), ("g_raw",))
    floor["loss"] = abs(float(f32["loss"]) - float(ref["loss"])) / max(1.0, abs(float(ref["loss"])))
    floor["resid"] = max_abs(f32["resid"], ref["resid"])
    return dict(raw=raw, raw_a=torch.cat([rgb, occ_a[..., None]], -1), occ_b=occ_b, z=z, gt_depth=gt,
                gt_color=gt_color, keep=keep, kind=kind, ref=ref, f32=f32, floor=floor, mode=mode)
