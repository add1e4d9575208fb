"""tests/nice_ref.py (the plain-torch restatement of the NICE point query) in float32 against the reference's own
outputs in the trained regime, tests/golden/trained_fixtures.*.npz (make_golden_trained.py) — on the CPU — and the
conditions that make tests/golden/trained_scene.py the regime it claims to be.

Tolerance, as tests/test_imap_golden.py: two float32 evaluations of one formula differ by at most about twice one
evaluation's error, which the fixture records per quantity as `floor` (reference float32 against the restatement
in float64); the bar is 4 x floor, and never below 1e-6.  d/dpts is compared on trained_scene.NOT_LATTICE (the rows
its floor was measured on): at a grid node the trilinear weights have a kink.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nice_ref as ref  # noqa: E402
import trained_scene as sc  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return load_golden("trained_fixtures")


@pytest.fixture(scope="module")
def scene():
    return (torch.from_numpy(sc.bound()), {k: torch.from_numpy(v) for k, v in sc.decoders().items()},
            {k: torch.from_numpy(v) for k, v in sc.grids().items()}, torch.from_numpy(sc.points()))


def close(fx, case, name, got, rows=None):
    want = torch.from_numpy(fx[f"{case}.{name}"])
    if rows is not None:
        got, want = got[rows], want[rows]
    bar = max(4.0 * float(fx[f"{case}.floor.{name}"]), 1e-6)
    err = ref.rel_l2(got, want)
    print(f"{case}.{name}: rel_l2 {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (case, name, err, bar)


@pytest.mark.parametrize("stage", ref.STAGES)
def test_eval_points(fx, scene, stage):
    bound, sd, grids, p = scene
    case = "eval." + stage
    cot = torch.from_numpy(sc.cotangent(stage))
    assert np.array_equal(fx[case + ".cot"], cot.numpy())
    raw, g = ref.vjp(sd, grids, p, cot, stage, bound)
    close(fx, case, "raw", raw)
    stored = sorted(k[len(case) + 6:] for k in fx if k.startswith(case + ".grad."))
    assert stored == sorted(g)
    for name in stored:
        close(fx, case, "grad." + name, g[name], rows=sc.NOT_LATTICE if name == "pts" else None)
    assert int((raw[:, 3] == 100).sum()) == int(fx[case + ".n_oob"]) == sc.OOB.size
    assert bool((raw[sc.OOB, 3] == 100).all())


@pytest.mark.parametrize("name", sc.DECODERS)
def test_sub_decoder(fx, scene, name):
    bound, sd, grids, p = scene
    out = ref.sub_decoder(sd, name, p, grids, bound)
    assert out.shape == ((sc.M, 4) if name == "color" else (sc.M,))
    close(fx, "sub." + name, "out", out)


def test_every_bias_is_nonzero(scene):
    sd = scene[1]
    assert len(sc.BIASED) == 24
    for k in sd:
        if k.endswith(".bias"):
            assert bool((sd[k] != 0).all()), k
    assert float(sd["color_decoder.output_linear.bias"][3]) != 0.0  # bo[3]: the 4th colour row of direct callers


def test_relu_layers_are_half_active(scene):
    bound, sd, grids, p = scene
    for name in sc.DECODERS:
        acts = []
        ref.sub_decoder(sd, name, p, grids, bound, torch.float64, acts)
        frac = [float((a > 0).double().mean()) for a in acts]
        assert len(frac) == 5 and all(0.3 <= f <= 0.7 for f in frac), (name, frac)


def test_point_classes(scene):
    bound, _, grids, p = scene
    lo, hi = bound[:, 0], bound[:, 1]
    ext = hi - lo
    assert p.shape == (sc.M, 3) and sc.M == 10 * 32 + 10
    assert sc.LATTICE.size == 40 and sc.NEAR_FACE.size == 20
    groups = [sc.LATTICE, sc.NEAR_FACE, sc.OOB]
    assert np.unique(np.concatenate(groups)).size == sum(g.size for g in groups)  # disjoint
    ins = ref.inside(p, bound)
    assert sorted(np.nonzero(~ins.numpy())[0]) == sorted(sc.OOB) and sc.OOB.size == 35
    assert float(p[sc.FACE_LO, 0]) == float(lo[0]) and float(p[sc.FACE_HI, 1]) == float(hi[1])
    assert bool(ins[sc.FACE_LO] | ins[sc.FACE_HI]) is False
    assert torch.equal(p[sc.CORNER_LO], lo) and torch.equal(p[sc.CORNER_HI], hi)
    assert bool(((p[sc.OUTSIDE] < lo) | (p[sc.OUTSIDE] > hi)).any(1).all())
    # LATTICE: on interior nodes of the fine grid (to the rounding of the float64 point)
    g = grids["grid_fine"]
    n = torch.tensor([g.shape[4], g.shape[3], g.shape[2]], dtype=torch.float64)
    u = (p[sc.LATTICE] - lo) / ext * (n - 1)
    k = torch.round(u)
    assert float((u - k).abs().max()) < 1e-9 and bool(((k >= 1) & (k <= n - 2)).all())
    # NEAR_FACE: inside, and on at least one axis 1e-7 .. 2e-6 of the extent below the hi face
    d = (hi - p[sc.NEAR_FACE]) / ext
    near = (d >= 1e-7 * (1 - 1e-6)) & (d <= 2e-6 * (1 + 1e-6))
    assert bool(near.any(1).all()) and bool(ins[sc.NEAR_FACE].all())
    assert bool((((n - 1) * (1 - d))[near] > n.expand_as(d)[near] - 2).all())  # the last cell
    # the ray form: 7 x 48 points, some of every ray's out of bound
    rp = torch.from_numpy(sc.ray_points())
    assert rp.shape == (336, 3) and sc.N_SAMPLES % 32 != 0
    rin = ref.inside(rp, bound).reshape(sc.N_RAYS, sc.N_SAMPLES)
    assert bool(rin.any(1).all()) and bool((~rin).any(1).all())
    z = sc.rays()[2]
    assert bool((np.diff(z, axis=1) > 0).all())


def test_live_rows_keep_a_third():
    for name in ("middle", "fine", "color"):
        n = int(np.prod(sc.grid_shape(name)[2:]))
        r = sc.live_rows(name)
        assert 0.25 * n < r.size < 0.42 * n and bool((np.diff(r) > 0).all()), (name, r.size, n)
