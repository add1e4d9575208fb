"""Live-point lists of the mask-only mapping backward (nslam_live_points, nslam_query_bwd_decoders_live):

  the lists     vs a torch restatement of the corner convention with a +-1e-4-cell margin (the kernel's set
                   contains the strict set and lies inside the loose one), ascending, n_live = their length;
  edge cases    a slot map that selects nothing / everything, a live count that is a multiple of 32;
  gradients     compaction on vs off: grid gradients rel_l2 < 1e-5 (the bound test_gpu_fused.py uses between
                   backward variants: only the order of the float atomics differs), the colour decoder's
                   gradient bit for bit (its kernel does not see the lists);
  row rebinding two prefetching iterations with other frustum rows bound between them.
"""
import importlib
import itertools

import pytest
import torch

from conftest import rel_l2
from test_gpu_fused import _frames, _nice

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
KEYS = ("grid_middle", "grid_fine", "grid_color")
GRID_OF = {"middle": "grid_middle", "fine": "grid_fine", "color": "grid_color"}
HW = (96, 128)


def _half_rows(c, frac=0.7):
    """Frustum-like selections: the voxels of the low-x part of every grid (a good share of the rays' samples
    then touches no selected voxel; at 0.5 only a ninth of the fine grid's points were live)."""
    rows = {}
    for k in KEYS:
        Z, Y, X = c[k].shape[2:]
        ix = torch.arange(Z * Y * X, device=DEV) % X
        rows[k] = torch.nonzero(ix < max(1, int(X * frac))).reshape(-1).to(torch.int32)
    return rows


def _rays(sc, frames, n_per, seed=4):
    pix = torch.randint(HW[0] * HW[1], (len(frames) * n_per,), device=DEV,
                        generator=torch.Generator(device=DEV).manual_seed(seed))
    ro, rd, gd, gc, keep = P.ops.gather_rays(frames, pix, n_per, HW[0], HW[1], (0, HW[0], 0, HW[1]), sc.fx, sc.fy,
                                             sc.cx, sc.cy, sc.bound)
    z = P.ops.sample_z(ro, rd, gd, sc.bound, 32, 16)
    return pix, ro, rd, z


def _live_ref(eng, name, c, ro, rd, z):
    """(strict, loose) bool [N*S]: the points with a selected in-range corner in decoder `name`'s grid for
    every / for some displacement of the cell coordinates by up to 1e-4 cells per axis."""
    key = GRID_OF[name]
    Z, Y, X = c[key].shape[2:]
    slot = eng.slot[key]
    lo, hi = (torch.tensor(v, dtype=torch.float64, device=DEV) for v in eng.dec_bounds[name])
    p = (ro.double()[:, None] + rd.double()[:, None] * z[..., None]).reshape(-1, 3)
    nc = (((p - lo) / (hi - lo)) * 2 - 1.0).float().double()  # decoder.py:168-175: normalised, then .float()
    n = torch.tensor([X, Y, Z], dtype=torch.float64, device=DEV)
    u0 = ((nc + 1) / 2) * (n - 1)
    strict = torch.ones(p.shape[0], dtype=torch.bool, device=DEV)
    loose = torch.zeros_like(strict)
    for d in itertools.product((-1e-4, 0.0, 1e-4), repeat=3):
        u = torch.minimum(torch.clamp(u0 + torch.tensor(d, dtype=torch.float64, device=DEV), min=0.0), n - 1)
        i0 = torch.floor(u).long()
        hit = torch.zeros_like(loose)
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            ix, iy, iz = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
            ok = (ix <= X - 1) & (iy <= Y - 1) & (iz <= Z - 1)  # (grid_sample's within_bounds)
            row = ((iz * Y + iy) * X + ix).clamp(max=Z * Y * X - 1)
            hit |= ok & (slot[row] >= 0)
        strict &= hit
        loose |= hit
    return strict, loose


@pytest.mark.parametrize("nf,n_per", [(1, 1), (1, 13), (3, 50)])
def test_live_lists_match_torch(tiny, nf, n_per):
    """1, 13 and 150 rays x 48 samples (no multiple of the 256-point scan block; one, three and 29 of them)."""
    sc, frames = _frames(tiny, nf=nf)
    nice, c = _nice(sc)
    eng = P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV, rows=_half_rows(c))
    _, ro, rd, z = _rays(sc, frames, n_per)
    n = z.numel()
    assert n == nf * n_per * 48
    idx, nl = eng.live_lists("color", ro, rd, z)
    torch.cuda.synchronize()
    some_dead = False
    for i, name in enumerate(("middle", "fine", "color")):
        k = int(nl[P.ops.DEC_ID[name]])
        assert 0 <= k <= n, name
        lst = idx[i, :k].long()
        assert bool((lst[1:] > lst[:-1]).all()), f"{name}: not ascending"
        assert k == 0 or (int(lst[0]) >= 0 and int(lst[-1]) < n), name
        got = torch.zeros(n, dtype=torch.bool, device=DEV)
        got[lst] = True
        assert int(got.sum()) == k, name  # n_live is the list's length: no duplicates
        strict, loose = _live_ref(eng, name, c, ro, rd, z)
        print(f"{name}: n={n} n_live={k} strict={int(strict.sum())} loose={int(loose.sum())}")
        assert bool((got | ~strict).all()), f"{name}: a strictly live point is missing"
        assert bool((loose | ~got).all()), f"{name}: a listed point touches no selected voxel"
        some_dead |= 0 < k < n
    if nf * n_per >= 150:
        assert some_dead  # the selection splits the batch: both outcomes of the test are exercised


def _bwd(eng, stage, ro, rd, z, g_raw, live, keys):
    """One mask-only backward of `stage` into zeroed gradients; returns the grids' compact gradients."""
    eng.gall.zero_()
    eng.query_fwd(stage, ro, rd, z, defer_occ=True)
    eng.query_bwd(stage, ro, rd, z, g_raw, keys, (), live=eng.live_lists(stage, ro, rd, z) if live else None)
    torch.cuda.synchronize()
    return {k: eng.ggrad[k].clone() for k in keys}


def test_live_edge_cases(tiny):
    """Nothing selected: n_live = 0 and the launch writes nothing.  Everything selected: the list is
    arange(n), here with n = 2 rays x 48 = 96 points, a live count that is an exact multiple of 32, and the
    gradients equal the uncompacted launch's."""
    sc, frames = _frames(tiny, nf=1)
    nice, c = _nice(sc)
    rows = {k: torch.arange(c[k].shape[2:].numel(), dtype=torch.int32, device=DEV) for k in KEYS}
    eng = P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV, rows=rows)
    _, ro, rd, z = _rays(sc, frames, 2)
    n = z.numel()
    assert n == 96
    g_raw = torch.randn(n, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    idx, nl = eng.live_lists("color", ro, rd, z)
    for i, name in enumerate(("middle", "fine", "color")):
        assert int(nl[P.ops.DEC_ID[name]]) == n, name
        assert torch.equal(idx[i].long(), torch.arange(n, device=DEV)), name
    off = _bwd(eng, "color", ro, rd, z, g_raw, False, KEYS)
    on = _bwd(eng, "color", ro, rd, z, g_raw, True, KEYS)
    for k in KEYS:
        assert float(off[k].abs().sum()) > 0, k
        assert rel_l2(on[k], off[k]) < 1e-5, k
    # nothing selected (the gradient buffers keep their size: any write would show)
    for k in KEYS:
        eng.slot[k].fill_(-1)
    eng.rows_gen += 1
    idx, nl = eng.live_lists("color", ro, rd, z)
    for name in ("middle", "fine", "color"):
        assert int(nl[P.ops.DEC_ID[name]]) == 0, name
    eng.gall.zero_()
    eng.query_fwd("color", ro, rd, z, defer_occ=True)
    eng.query_bwd("color", ro, rd, z, g_raw, KEYS, (), live=(idx, nl))
    torch.cuda.synchronize()
    assert float(eng.gall.abs().sum()) == 0.0


@pytest.mark.parametrize("stage", ["middle", "fine", "color"])
@pytest.mark.parametrize("nf,n_per", [(1, 13), (3, 50)])
def test_live_gradients_match_uncompacted(tiny, stage, nf, n_per):
    """One mapping iteration of the engine (13 and 150 rays) with the lists on and off: the grid gradients
    agree to rel_l2 < 1e-5 per grid and the colour decoder's gradient bit for bit."""
    sc, frames = _frames(tiny, nf=nf)
    pix = torch.randint(HW[0] * HW[1], (nf * n_per,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(21))
    out = {}
    for live in (False, True):
        nice, c = _nice(sc)
        rows = _half_rows(c)
        eng = P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV, rows=rows)
        eng.live_points = live
        opt = P.ops.FusedAdam([{"params": [eng.decs["color"].param], "lr": 0.0}] +
                              [{"params": [c[k]], "lr": 0.0, "rows": rows[k]} for k in KEYS])
        gr = {}
        keys = eng.grads_for(stage, ("color",))[0]

        def snapshot(ks, dn):
            for k in keys:
                gr[k] = eng.ggrad[k].clone()
            gr["dec"] = eng.decs["color"].grad.clone()

        eng.iteration(stage, frames, pix, n_per, HW, (sc.fx, sc.fy, sc.cx, sc.cy), opt, exchange=snapshot)
        torch.cuda.synchronize()
        out[live] = gr
    for k in keys:
        err = rel_l2(out[True][k], out[False][k])
        print(f"{stage} {nf * n_per} rays {k}: rel_l2 {err:.2e} |g| {float(out[False][k].abs().sum()):.3e}")
        if nf * n_per >= 150:  # (13 rays may leave a grid's selected rows without any gradient)
            assert float(out[False][k].abs().sum()) > 0, k
        assert err < 1e-5, k
    assert torch.equal(out[True]["dec"], out[False]["dec"])
    if stage == "color":
        assert float(out[False]["dec"].abs().sum()) > 0


def test_live_lists_follow_row_rebinding(tiny):
    """Two prefetching iterations with other frustum rows bound between them: the batch prefetched during
    the first call carries lists of the old slot maps, which the second call must not use.  The map after
    the second call equals the run without lists."""
    sc, frames = _frames(tiny)
    out = {}
    for live in (False, True):
        nice, c = _nice(sc)
        eng = P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV)
        eng.live_points = live
        masks = []
        for lo, hi in ((0.0, 0.5), (0.4, 1.0)):  # low-x half, then the high-x part
            m = {}
            for k in KEYS:
                Z, Y, X = c[k].shape[2:]
                x = torch.arange(X, device=DEV)
                m[k] = ((x >= int(X * lo)) & (x < max(1, int(X * hi))))[:, None, None].expand(X, Y, Z).contiguous()
            masks.append(m)
        eng.bind_masks(masks[0])
        groups = [{"params": [eng.decs["color"].param], "lr": 0.005}]
        for k in KEYS:
            r, nlv = eng.live_rows(k)
            groups.append({"params": [c[k]], "lr": 0.005, "rows": r, "n_live": nlv})
        opt = P.ops.FusedAdam(groups)
        args = (None, 50, HW, (sc.fx, sc.fy, sc.cx, sc.cy), opt)
        eng.iteration("color", frames, *args, seed=11, prefetch=True)
        eng.bind_masks(masks[1])
        eng.iteration("color", frames, *args, seed=11, prefetch=True)
        torch.cuda.synchronize()
        if live:  # the second call used the prefetched rays with lists of the rows bound for it
            assert eng.ring.live_gen[0] == eng.ring.live_gen[1] == (eng.layout_gen, eng.rows_gen)
        out[live] = ({k: c[k].detach().clone() for k in KEYS}, eng.decs["color"].param.detach().clone())
    for k in KEYS:
        err = rel_l2(out[True][0][k], out[False][0][k])
        print(f"{k}: rel_l2 {err:.2e}")
        assert err < 1e-5, k
    assert rel_l2(out[True][1], out[False][1]) < 1e-5


def test_live_points_knob_rejects_unknown_values(tiny, monkeypatch):
    sc, _ = _frames(tiny, nf=1)
    nice, c = _nice(sc)
    monkeypatch.setenv("NSLAM_LIVE_POINTS", "yes")
    with pytest.raises(ValueError, match="NSLAM_LIVE_POINTS"):
        P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV)
    monkeypatch.setenv("NSLAM_LIVE_POINTS", "0")
    assert P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV).live_points is False
