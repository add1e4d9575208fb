"""The per-ray kernels at chunk edges, sample counts and saturation, against float64 references that share no
code with them (tests/ray_edge_cases.py; its input conditions are asserted in test_ray_edges_cpu.py).

  A  nslam_sample_rays: both kernels (one wave per ray up to 64 samples, the serial merge above), with and
     without gt_depth, lindisp off and on, every max-depth path, the limits and their refusals — bit for bit
     against oracle.sample_z, into an `out=` pre-filled with a sentinel so an unwritten slot cannot match.
  B  nslam_composite_fwd / _bwd at S = 1 .. 256: the transmittance carried across 64-sample chunks, the
     backward's cross-chunk suffix sum, surfaces on chunk boundaries, alpha == 1.0f, NULL cotangents.
  C  nslam_composite_density_fwd / _bwd on the same scene mapped to densities, with |rays_d| != 1, at S = 2 .. 256;
     S = 1 is refused (the reference composites no sample there).
  D  nslam_render_loss against oracle.composite + oracle.mapper_loss / tracker_loss under autograd in float64
     (never ops.composite), at the three median paths, with keep holes, gt_depth == 0, outliers the dynamic
     mask removes, and occ_add.

Bars: max(project bar, 4 x floor).  Project bars: 1e-6 max-abs for compositor outputs, 1e-5 rel-L2 for g_raw
(here per 64-sample chunk), 1e-6 relative for the loss.  The floor is the reference's own float32 result
against its float64 one, per case and quantity (ray_edge_cases.py), never anything measured from a kernel;
DESIGN 7e tabulates floors and what the kernels measured.  Every ray of every case is compared.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ray_edge_cases as rc

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
SENTINEL = -7.0
UNSUPPORTED = "configuration outside the supported"


def dev(t):
    return t.to(DEV) if t is not None else None


# ------------------------------------------------------------------------------------------------ A sampler
def run_sampler(c):
    n, S = c["z"].shape
    out = torch.full((n, S), SENTINEL, dtype=torch.float64, device=DEV)
    z = P.ops.sample_z(dev(c["rays_o"]), dev(c["rays_d"]), dev(c["gt"]), rc.BOUND, c["n_strat"], c["n_surf"],
                       lindisp=c["lindisp"], gt_max=dev(c["gt_max"]), out=out)
    assert z is out
    got, want = z.cpu().numpy(), c["z"].numpy()
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    print(f"sampler {c['n_strat']}+{c['n_surf']} gt={c['gt'] is not None} lindisp={c['lindisp']} n={n}: "
          f"{int(bad.sum())} of {bad.size} differ, {int((got == SENTINEL).sum())} slots unwritten, "
          f"{int(np.isnan(want).sum())} NaN in the oracle")
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("kw", rc.sampler_cases(), ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_sampler_bitexact(kw):
    run_sampler(rc.sampler_case(**kw))


@pytest.mark.parametrize("name", sorted(rc.EXTRA_SAMPLER))
def test_sampler_max_paths_and_descending_surface(name):
    run_sampler(rc.sampler_case(**rc.EXTRA_SAMPLER[name]))


@pytest.mark.parametrize("n_strat,n_surf", [(129, 16), (32, 65)])
def test_sampler_refuses_above_limits(n_strat, n_surf):
    o, d, gt = (dev(t) for t in rc.sampler_rays(rc.N_WAVE))
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        P.ops.sample_z(o, d, gt, rc.BOUND, n_strat, n_surf)


def test_sampler_no_rays():
    e3, e1 = torch.empty(0, 3, device=DEV), torch.empty(0, device=DEV)
    z = P.ops.sample_z(e3, e3, e1, rc.BOUND, 49, 16)
    assert tuple(z.shape) == (0, 65) and z.dtype == torch.float64
    assert tuple(P.ops.sample_z(e3, e3, None, rc.BOUND, 32, 16).shape) == (0, 32)


# ------------------------------------------------------------------------------------------------ B, C, E
def compare(tag, got, c, outs, chunked, whole=()):
    """Print every figure, then assert each against max(project bar, 4 x floor)."""
    ref, fl = c["ref"], c["floor"]
    fails = []
    for name in outs:
        e, b = rc.max_abs(got[name].cpu(), ref[name]), rc.bar(rc.BAR_OUT, fl[name])
        print(f"{tag} {name}: max-abs {e:.2e} (floor {fl[name]:.2e}, bar {b:.1e})")
        assert got[name].shape == ref[name].shape
        fails += [(name, e, b)] if not e <= b else []
    for name in chunked:
        es, b = rc.chunk_rel_l2(got[name].cpu(), ref[name]), rc.bar(rc.BAR_GRAD, fl[name])
        print(f"{tag} {name}: rel-L2 per chunk " + " ".join(f"{e:.2e}" for e in es)
              + f" (floor {fl[name]:.2e}, bar {b:.1e})")
        assert got[name].shape == ref[name].shape and bool(torch.isfinite(got[name]).all())
        fails += [(name, es, b)] if not all(e <= b for e in es) else []
    for name in whole:
        e, b = rc.rel_l2(got[name].cpu(), ref[name]), rc.bar(rc.BAR_GRAD, fl[name])
        print(f"{tag} {name}: rel-L2 {e:.2e} (floor {fl[name]:.2e}, bar {b:.1e})")
        fails += [(name, e, b)] if not e <= b else []
    assert not fails, (tag, fails)


@pytest.mark.parametrize("S", rc.COMPOSITE_S)
def test_composite_vs_float64(S):
    c = rc.composite_case(S)
    raw = dev(c["raw"]).requires_grad_(True)
    depth, var, rgb = P.ops.composite(raw, dev(c["z"]))
    (g_raw,) = torch.autograd.grad((depth, var, rgb), (raw,), [dev(t) for t in c["cots"]])
    assert depth.dtype == torch.float64 and var.dtype == torch.float64 and rgb.dtype == torch.float32
    compare(f"composite S={S}", dict(depth=depth, var=var, rgb=rgb, g_raw=g_raw), c, ("depth", "var", "rgb"),
            ("g_raw",))


@pytest.mark.parametrize("S", rc.DENSITY_S)
def test_composite_density_vs_float64(S):
    c = rc.density_case(S)
    raw = dev(c["raw"]).requires_grad_(True)
    rd = dev(c["rays_d"]).requires_grad_(True)
    depth, var, rgb, weights = P.ops.composite_density(raw, dev(c["z"]), rd)
    g_raw, g_rd = torch.autograd.grad((depth, var, rgb), (raw, rd), [dev(t) for t in c["cots"]])
    compare(f"density S={S}", dict(depth=depth, var=var, rgb=rgb, weights=weights, g_raw=g_raw, g_rays_d=g_rd), c,
            ("depth", "var", "rgb", "weights"), ("g_raw",), ("g_rays_d",))


def test_compositors_refuse_unsupported_sample_counts():
    """S = 257 everywhere; S = 1 in density mode, where the reference composites no sample at all
    (test_ray_edges_cpu.py) and one opaque sample at dist 1e10 would not be its answer."""
    one = torch.tensor([[[0.2, 0.4, 0.6, 5.0]]] * 3, device=DEV)
    z1 = torch.full((3, 1), 1.5, dtype=torch.float64, device=DEV)
    rd = torch.ones(3, 3, device=DEV)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        P.ops.composite_density(one, z1, rd)
    L, ptr = P._lib.lib(), P._lib.ptr
    g1 = torch.full_like(one, SENTINEL)
    for s in (1, 257):  # (refused before any pointer is read: the buffers hold one sample)
        code = L.nslam_composite_density_bwd(ptr(one), ptr(z1), ptr(rd), 3, s, None, None, None, ptr(g1), None,
                                             P._lib.stream_ptr(DEV))
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            P._lib.check(code, "nslam_composite_density_bwd")
    assert bool((g1 == SENTINEL).all())
    d1, v1, c1 = P.ops.composite(one, z1)  # occupancy mode has a one-sample answer (test_composite_vs_float64[1])
    assert d1.shape == (3,)
    raw = torch.zeros(3, 257, 4, device=DEV)
    z = torch.linspace(0.1, 4.1, 257, dtype=torch.float64, device=DEV).repeat(3, 1)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        P.ops.composite(raw, z)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        P.ops.composite_density(raw, z, torch.ones(3, 3, device=DEV))
    g = torch.empty_like(raw)
    L = P._lib.lib()
    rcode = L.nslam_composite_bwd(P._lib.ptr(raw), P._lib.ptr(z), 3, 257, None, None, None, P._lib.ptr(g),
                                  P._lib.stream_ptr(DEV))
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        P._lib.check(rcode, "nslam_composite_bwd")
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        P.ops.render_loss(raw, z, torch.ones(3, device=DEV), None, mode="mapper", use_color=False)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_composite_bwd_null_cotangents(which):
    """A NULL cotangent is a zero one: the direct call with one cotangent equals, in bits, the autograd call
    that passes zeros for the other two (S = 130: three chunks)."""
    c = rc.composite_case(130)
    raw, z = dev(c["raw"]), dev(c["z"])
    cots = [dev(t) for t in c["cots"]]
    zeros = [torch.zeros_like(t) if i != which else t for i, t in enumerate(cots)]
    r = raw.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(P.ops.composite(r, z), (r,), zeros)
    g = torch.full_like(raw, SENTINEL)
    ptrs = [P._lib.ptr(t) if i == which else None for i, t in enumerate(cots)]
    code = P._lib.lib().nslam_composite_bwd(P._lib.ptr(raw), P._lib.ptr(z), raw.shape[0], raw.shape[1], ptrs[0],
                                            ptrs[1], ptrs[2], P._lib.ptr(g), P._lib.stream_ptr(DEV))
    P._lib.check(code, "nslam_composite_bwd")
    assert float(want.abs().max()) > 0
    assert torch.equal(g, want)


# ------------------------------------------------------------------------------------------------ D
def run_loss(c, occ_add):
    _, use_color, hd, w = rc.LOSS_MODES[c["mode"]]
    kind = rc.LOSS_MODES[c["mode"]][0]
    raw = dev(c["raw_a"] if occ_add else c["raw"])
    occ = dev(c["occ_b"]).contiguous() if occ_add else None
    depth, var, color, ray_loss, g_raw = P.ops.render_loss(raw, dev(c["z"]), dev(c["gt_depth"]), dev(c["gt_color"]),
                                                           dev(c["keep"]), mode=kind, use_color=use_color,
                                                           handle_dynamic=hd, w_color=w, occ_add=occ)
    return dict(depth=depth, var=var, color=color, loss=ray_loss.sum(), g_raw=g_raw.reshape(c["raw"].shape))


@pytest.mark.parametrize("occ_add", [False, True], ids=["raw", "occ_add"])
@pytest.mark.parametrize("mode", sorted(rc.LOSS_MODES))
@pytest.mark.parametrize("S,n", rc.LOSS_CASES)
def test_render_loss_vs_float64(S, n, mode, occ_add):
    c = rc.loss_case(S, n, mode)
    got = run_loss(c, occ_add)
    tag = f"loss S={S} n={n} {mode}{' occ_add' if occ_add else ''}"
    want = float(c["ref"]["loss"])
    e, b = abs(float(got["loss"]) - want) / max(1.0, abs(want)), rc.bar(rc.BAR_LOSS, c["floor"]["loss"])
    print(f"{tag} loss: {float(got['loss']):.9g} vs {want:.9g}: relative {e:.2e} (floor {c['floor']['loss']:.2e}, "
          f"bar {b:.1e})")
    compare(tag, got, c, ("depth", "var", "color"), ("g_raw",))
    assert e <= b, (tag, e, b)


@pytest.mark.parametrize("mode", ["mapper_color", "tracker_dynamic"])
def test_render_loss_nothing_kept(mode):
    c = rc.loss_case(48, 5, mode, keep_none=True)
    got = run_loss(c, False)
    compare(f"loss nothing kept {mode}", got, c, ("depth", "var", "color"), ())
    assert float(got["loss"]) == 0.0 and float(got["g_raw"].abs().max()) == 0.0
