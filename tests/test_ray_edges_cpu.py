"""The input conditions of tests/ray_edge_cases.py, asserted on the references alone (no GPU), and the
float32 noise floors, printed (`pytest -s`).  With these holding, test_gpu_ray_edges.py can neither pass nor
fail because of badly conditioned inputs: its bars are max(project bar, 4 x floor), and a floor above ten
times its project bar fails here, where the inputs (not the bar) are to be changed.
"""
import numpy as np
import pytest
import torch

import ray_edge_cases as rc


# ---------------------------------------------------------------------------------------------- sampler
def _check_sampler(c):
    z = c["z"]
    n, S = z.shape
    s0 = c["n_strat"]
    s1 = c["n_surf"] if c["gt"] is not None else 0
    assert S == s0 + s1
    nan = torch.isnan(z)
    # Where the reference produces NaN (lindisp with gt_depth only): 1/near = inf meets (1 - t) = 0 at t = 1
    # in a row with gt_depth == 0 (the linspace holds t = 1 once s0 >= 2), and 1/far = inf meets t = 0 in a
    # row whose far clamps to 0 (origin outside the bound, pointing away).  One NaN per cause, nowhere else.
    want = torch.zeros(n, dtype=torch.long)
    if c["lindisp"] and c["gt"] is not None:
        want += ((c["gt"] == 0) & (s0 >= 2)).long() + (c["far"] == 0).long()
    assert torch.equal(nan.sum(1), want)
    if s1 > 0:  # the reference sorts only then (Renderer.py:168): ascending, the NaNs last
        for r in range(n):
            k = S - int(want[r])
            assert not bool(nan[r, :k].any()) and bool(nan[r, k:].all())
            assert bool((z[r, 1:k] >= z[r, :k - 1]).all())
    return int(want.sum())


@pytest.mark.parametrize("kw", rc.sampler_cases(), ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_sampler_reference_conditions(kw):
    c = rc.sampler_case(**kw)
    o, d, gt = rc.sampler_rays(c["z"].shape[0])
    lo, hi = rc.BOUND[:, 0].float(), rc.BOUND[:, 1].float()
    kind = torch.arange(o.shape[0]) % 6
    inside = ((o > lo) & (o < hi)).all(1)
    assert bool(inside[kind != 1].all()) and not bool(inside[kind == 1].any())
    assert bool((rc.orc.far_bound(o, d, rc.BOUND)[kind == 1] + 0.01 < 0).all())  # far_bb < 0: far clamps to 0
    assert bool((d[kind == 2, 1] == 0).all()) and not bool(torch.signbit(d[kind == 2, 1]).any())
    assert bool(torch.signbit(d[kind == 3, 2]).all()) and bool((d[kind == 3, 2] == 0).all())
    assert bool(((d[kind == 4] == 0).sum(1) == 2).all())
    assert bool((gt[::5] == 0).all()) and int((gt == 0).sum()) == (o.shape[0] + 4) // 5
    assert bool(torch.isfinite(rc.orc.far_bound(o, d, rc.BOUND)).all())
    nans = _check_sampler(c)
    if kw["lindisp"] and kw["with_gt"]:
        assert nans > 0
    # the descending stratified list really occurs
    if kw["n_strat"] >= 2 and not kw["lindisp"] and not kw["with_gt"]:
        assert bool((c["z"][kind == 1][:, -1] < c["z"][kind == 1][:, 0]).all())


@pytest.mark.parametrize("name", sorted(rc.EXTRA_SAMPLER))
def test_sampler_extra_conditions(name):
    kw = rc.EXTRA_SAMPLER[name]
    c = rc.sampler_case(**kw)
    assert _check_sampler(c) == 0
    if kw.get("all_zero"):
        assert float(c["gt"].abs().max()) == 0.0 and float(c["far"].abs().max()) == 0.0
        assert float(c["z"].max()) == 0.001 and float(c["z"].min()) == 0.0
    if kw.get("gt_max"):
        assert float(c["gt"].max()) < rc.GT_MAX
        plain = rc.sampler_case(**{**kw, "gt_max": False})
        assert not torch.equal(plain["z"], c["z"])  # the given maximum is really used
    if name == "max_gt_launch":
        assert c["z"].shape[0] > 8192


# ---------------------------------------------------------------------------------------------- compositors
def _check_scene(c, S, grads, outs, whole=()):
    ref, kind, k0 = c["ref"], c["kind"], c["k0"]
    for k in range(4):
        assert int((kind == k).sum()) >= 3
    assert 3 <= int((kind == rc.SATURATED).sum()) <= 8 and 3 <= int((kind == rc.EMPTY).sum()) <= 8
    assert sorted(set(k0[kind == rc.SURFACE].tolist())) == sorted(rc.surface_starts(S))
    # enough light reaches the end of every transparent row for the late chunks to matter
    assert float(ref["trans"][kind == rc.TRANSPARENT][:, -1].min()) >= 0.1
    a32 = torch.sigmoid(10 * c["raw"][kind == rc.SATURATED][..., 3]) if "rays_d" not in c else None
    if a32 is not None:
        assert bool((a32 == 1.0).all())  # alpha rounds to exactly 1.0f: the factor is the bare 1e-10
    z = c["z"]
    assert z.dtype == torch.float64 and bool((z[:, 1:] > z[:, :-1]).all())
    assert float(z.min()) >= 0.1 and float(z.max()) <= 4.1 + 1e-12
    for name in grads + whole:
        assert bool(torch.isfinite(ref[name]).all()) and bool(torch.isfinite(c["f32"][name]).all())
    norms = rc.chunk_norms(ref["g_raw"])
    assert all(norms[0] / 10 <= v <= norms[0] * 10 for v in norms), norms
    fl = c["floor"]
    for name in outs:
        assert fl[name] <= 10 * rc.BAR_OUT, (name, fl[name])
    for name in grads + whole:
        assert fl[name] <= 10 * rc.BAR_GRAD, (name, fl[name])
    return norms


@pytest.mark.parametrize("S", rc.COMPOSITE_S)
def test_composite_reference_conditions(S):
    c = rc.composite_case(S)
    assert c["raw"].shape == (rc.N_COMPOSITE, S, 4) and rc.N_COMPOSITE % 4 != 0
    norms = _check_scene(c, S, ("g_raw",), ("depth", "var", "rgb"))
    print(f"composite S={S}: floors " + " ".join(f"{k} {v:.2e}" for k, v in c["floor"].items())
          + f" | min T_end {float(c['ref']['trans'][c['kind'] == rc.TRANSPARENT][:, -1].min()):.2f}"
          + " | chunk norms " + " ".join(f"{v:.2f}" for v in norms))


@pytest.mark.parametrize("S", rc.DENSITY_S)
def test_density_reference_conditions(S):
    c = rc.density_case(S)
    norms = _check_scene(c, S, ("g_raw",), ("depth", "var", "rgb", "weights"), ("g_rays_d",))
    nrm = c["rays_d"].norm(dim=1)
    assert float(nrm.min()) < 0.9 and float(nrm.max()) > 1.1
    assert bool((c["raw"][c["kind"] == rc.EMPTY][..., 3] < 0).all())  # the relu's closed side
    # the documented scene: every row but the empty ones ends in an opaque sample (alpha exactly 1 at dist 1e10),
    # which takes all the light that is left; the empty rows weigh nothing anywhere
    full = c["kind"] != rc.EMPTY
    assert bool((c["raw"][full][:, -1, 3] == 0.5).all())
    w_end, t_end = c["ref"]["weights"][full][:, -1], c["ref"]["trans"][full][:, -1]
    # (`trans` rounds the z differences to float32 as the kernel does; the float64 reference does not: 1e-5.
    # Behind a surface 1 - alpha cancels and the two products agree to fewer digits still.)
    lit = t_end > 1e-6
    assert int(lit.sum()) >= int((c["kind"] == rc.TRANSPARENT).sum())
    assert torch.allclose(w_end[lit], t_end[lit], rtol=1e-5, atol=0) and bool((w_end[~lit] <= 2e-6).all())
    assert float(c["ref"]["weights"][~full].abs().max()) == 0.0
    print(f"density S={S}: floors " + " ".join(f"{k} {v:.2e}" for k, v in c["floor"].items())
          + " | chunk norms " + " ".join(f"{v:.2f}" for v in norms))


def test_density_reference_composites_nothing_at_one_sample():
    """Why density mode has no S = 1 case (and the kernels refuse it): the restated reference sizes the trailing
    1e10 from an empty slice, so a ray with one dense sample comes out with no weight at all."""
    raw = torch.tensor([[[0.2, 0.4, 0.6, 5.0]]])
    depth, var, rgb, w = rc.imap_ref.composite_density(raw, torch.tensor([[1.5]], dtype=torch.float64),
                                                       torch.tensor([[0.0, 0.0, 1.0]]))
    assert w.numel() == 0 and float(depth) == 0.0 and float(var) == 0.0 and float(rgb.abs().max()) == 0.0
    assert 1 not in rc.DENSITY_S and rc.DENSITY_S == rc.COMPOSITE_S[1:]


# ---------------------------------------------------------------------------------------------- render loss
@pytest.mark.parametrize("mode", sorted(rc.LOSS_MODES))
@pytest.mark.parametrize("S,n", rc.LOSS_CASES)
def test_loss_reference_conditions(S, n, mode):
    c = rc.loss_case(S, n, mode)
    kind_name, use_color, hd, w = rc.LOSS_MODES[mode]
    ref, f32, fl = c["ref"], c["f32"], c["floor"]
    keep = c["keep"].bool()
    gt = c["gt_depth"]
    assert 0 < int(keep.sum()) < n and int((gt[keep] == 0).sum()) > 0
    assert torch.equal(c["raw_a"][..., 3] + c["occ_b"], c["raw"][..., 3]) and float(c["occ_b"].abs().min()) > 0
    # the L1 kinks: no kept ray within 1e-3 of |x| = 0, in depth or in any colour channel
    pos = keep & (gt > 0)
    assert float((gt.double() - ref["depth"])[pos].abs().min()) >= 1e-3
    assert float((c["gt_color"].double() - ref["color"])[keep].abs().min()) >= 1e-3
    if kind_name == "tracker":
        assert float(ref["var"].min()) >= 1e-4
    removed = None
    if hd:
        r = ref["resid"]
        thr = 10 * r[keep].median()
        assert float((r - thr).abs().min()) > 10 * fl["resid"], (float((r - thr).abs().min()), fl["resid"])
        removed = float((r[pos] >= thr).sum()) / int(pos.sum())
        assert 0.05 <= removed <= 0.5, removed
        thr32 = 10 * f32["resid"][keep].median()
        assert torch.equal(r < thr, f32["resid"] < thr32)  # both precisions keep the same rays
    for name in ("g_raw",):
        assert bool(torch.isfinite(ref[name]).all())
    assert float(ref["g_raw"].abs().max()) > 0
    for name in ("depth", "var", "color"):
        assert fl[name] <= 10 * rc.BAR_OUT, (name, fl[name])
    assert fl["g_raw"] <= 10 * rc.BAR_GRAD and fl["loss"] <= 10 * rc.BAR_LOSS
    print(f"loss S={S} n={n} {mode}: floors " + " ".join(f"{k} {v:.2e}" for k, v in fl.items())
          + (f" | removed {removed:.2f}" if removed is not None else "") + f" | loss {float(ref['loss']):.4f}")


def test_loss_nothing_kept_is_zero():
    for mode in ("mapper_color", "tracker_dynamic"):
        c = rc.loss_case(48, 5, mode, keep_none=True)
        assert float(c["ref"]["loss"]) == 0.0 and float(c["ref"]["g_raw"].abs().max()) == 0.0


def test_bar_rule():
    assert rc.bar(1e-6, 1e-7) == 1e-6 and rc.bar(1e-6, 5e-7) == 2e-6
    a = torch.zeros(2, 130, 4)
    b = torch.ones(2, 130, 4)
    a[:, :64] = 1
    assert np.allclose(rc.chunk_rel_l2(a, b), [0.0, 1.0, 1.0])  # a wrong later chunk shows in its own figure
