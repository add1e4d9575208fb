"""Golden vectors of the fused point query in the trained regime (trained_scene.py: non-zero decoder biases, grids
of the magnitude a trained map has), produced by the reference's own code (build container only; the .npz parts it
writes are what tests/test_trained_golden.py and tests/test_gpu_trained.py read).

Run:  PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trained.py

Cases, inputs from trained_scene.py, the reference on the CPU in float32 (make_golden.py's harness: the reference's
NICE with the state_dict loaded, its sub-decoders combined by StageCombiner because NICE.forward names a cuda device,
Renderer.eval_points):
  eval.<stage>   coarse, middle, fine, color: raw of the 330 points, the cotangent, and its VJP to the points, the
                 stage's grids and every parameter that receives one (the embeddings' _B included).
  sub.<decoder>  each sub-decoder called directly (MLP.forward / MLP_no_xyz.forward): its output, the colour
                 decoder's with its own 4th row.
Only outputs are stored; the inputs are rebuilt from seeds.  Nothing of the reference is copied or modified.

For every quantity q the fixture also holds `<case>.floor.<q>` = rel_l2(reference float32, tests/nice_ref.py in
float64) and `<case>.floor_max.<q>`, the same difference's largest absolute entry: the noise floor of one float32
evaluation, from which the tests derive their tolerances.  d/dpts (grad.pts) is stored for every row; its floors
are over trained_scene.NOT_LATTICE, because at a grid node the trilinear weights have a kink and the float32 and
float64 coordinates fall into different cells (`eval.<stage>.lattice_err.pts` records what that does on the LATTICE
rows).  The generator asserts the regime: biases non-zero, every ReLU layer between 0.3 and 0.7 active, the
out-of-bound rows, and no point but the LATTICE and NEAR_FACE rows within 1e-4 cells of a cell face of any grid.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import nice_ref as ref  # noqa: E402
import scenes  # noqa: E402
import trained_scene as sc  # noqa: E402
from make_golden import StageCombiner, ref_nice, ref_renderer  # noqa: E402  (imports the reference)
from oracle import nslam_oracle as orc  # noqa: E402


def put(out, case, name, got32, ref64, rows=None):
    out[f"{case}.{name}"] = got32.detach().numpy()
    a, b = got32.detach().double(), ref64.detach().double()
    if rows is not None:
        a, b = a[rows], b[rows]
    out[f"{case}.floor.{name}"] = np.float64(ref.rel_l2(a, b))
    out[f"{case}.floor_max.{name}"] = np.float64((a - b).abs().max())


def check_regime(sd, grids, p, bound):
    for k in sc.BIASED:
        assert bool((sd[k] != 0).all()), k
    for name in sc.DECODERS:
        acts = []
        ref.sub_decoder(sd, name, p, grids, bound, torch.float64, acts)
        frac = [float((a > 0).double().mean()) for a in acts]
        print(f"  relu active {name}: " + " ".join(f"{f:.3f}" for f in frac))
        assert len(frac) == 5 and all(0.3 <= f <= 0.7 for f in frac), (name, frac)
        assert min(float(a.abs().min()) for a in acts) > 1e-7, name  # (no pre-activation at zero: masks agree)
    ins = ref.inside(p, bound)
    assert int((~ins).sum()) == sc.OOB.size and not bool(ins[sc.OOB].any())


def check_cells(p, bound, grids, skip):
    """No row outside `skip` within 1e-4 cells of a cell face of a grid it reads (coarse: the doubled bound)."""
    rows = np.setdiff1d(np.arange(p.shape[0]), skip)
    for key, g in grids.items():
        b = bound * 2 if key == "grid_coarse" else bound
        n = torch.tensor([g.shape[4], g.shape[3], g.shape[2]], dtype=torch.float64)
        u = ((ref.normalize(p, b).float().double() + 1) / 2) * (n - 1)
        d = (u - torch.round(u)).abs()
        d = torch.where((u > 0) & (u < n - 1), d, torch.ones_like(d))[rows]  # (a clamped axis has no gradient)
        assert float(d.min()) > 1e-4, (key, float(d.min()))


def eval_case(out, sd, grids, bound, stage):
    p = torch.from_numpy(sc.points())
    cot = torch.from_numpy(sc.cotangent(stage))
    m = ref_nice(sd, bound)
    r = ref_renderer(bound)
    gr = {k: v.clone().requires_grad_(True) for k, v in grids.items()}
    pp = p.clone().requires_grad_(True)
    raw = r.eval_points(pp, StageCombiner(m), gr, stage, "cpu")
    params = dict(m.named_parameters())
    names = ["pts"] + list(gr) + list(params)
    tens = [pp] + list(gr.values()) + list(params.values())
    grads = torch.autograd.grad(raw, tens, cot, allow_unused=True)
    raw64, g64 = ref.vjp(sd, grids, p, cot, stage, bound, torch.float64)
    case = "eval." + stage
    put(out, case, "raw", raw, raw64)
    out[case + ".cot"] = cot.numpy()
    got = {n: g for n, g in zip(names, grads) if g is not None}
    assert sorted(got) == sorted(g64), (sorted(got), sorted(g64))
    for n, g in got.items():
        put(out, case, "grad." + n, g, g64[n], rows=sc.NOT_LATTICE if n == "pts" else None)
    d = (got["pts"].double() - g64["pts"])[sc.LATTICE].abs().max()
    out[case + ".lattice_err.pts"] = np.float64(d)
    out[case + ".n_oob"] = np.int64(int((raw[:, 3] == 100).sum()))
    assert int(out[case + ".n_oob"]) == sc.OOB.size and bool((raw[sc.OOB, 3] == 100).all())
    occ = raw.detach()[np.setdiff1d(np.arange(sc.M), sc.OOB), 3]
    print(f"  {stage}: occupancy logits {float(occ.min()):.2f} .. {float(occ.max()):.2f}, "
          f"lattice d/dpts error {float(d):.3e} on |g| <= {float(got['pts'][sc.LATTICE].abs().max()):.1f}")


def sub_case(out, sd, grids, bound):
    p = torch.from_numpy(sc.points())
    m = ref_nice(sd, bound)
    for name in sc.DECODERS:
        o = getattr(m, name + "_decoder")(p[None], grids).squeeze(0).detach()
        o64 = ref.sub_decoder(sd, name, p, grids, bound, torch.float64)
        assert o.shape == o64.shape == ((sc.M, 4) if name == "color" else (sc.M,)), (name, o.shape)
        put(out, "sub." + name, "out", o, o64)


def main():
    torch.set_num_threads(1)
    bound = torch.from_numpy(sc.bound())
    assert torch.equal(bound, orc.enlarge_bound(sc.TINY_BOUND, sc.LEN["bound_divisible"]))
    sd = {k: torch.from_numpy(v) for k, v in sc.decoders().items()}
    grids = {k: torch.from_numpy(v) for k, v in sc.grids().items()}
    for k in sc.DECODERS:
        assert sc.grid_shape(k) == orc.grid_shape(bound, sc.LEN[k], 32, 2.0 if k == "coarse" else 1.0), k
    assert sorted(sd) == sorted(orc.init_decoders(torch.Generator().manual_seed(0)))
    p = torch.from_numpy(sc.points())
    check_regime(sd, grids, p, bound)
    check_cells(p, bound, grids, np.concatenate([sc.LATTICE, sc.NEAR_FACE, sc.OOB]))
    check_cells(torch.from_numpy(sc.ray_points()), bound, grids, np.zeros(0, dtype=np.int64))
    out = {}
    for stage in ref.STAGES:
        eval_case(out, sd, grids, bound, stage)
    sub_case(out, sd, grids, bound)
    paths = scenes.save_parts(os.path.join(HERE, "trained_fixtures"), out)
    print("wrote", [(os.path.basename(q), os.path.getsize(q)) for q in paths], len(out), "arrays")
    for k in sorted(out):
        if ".floor." in k or ".floor_max." in k:
            print(f"  {k:60s} {float(out[k]):.3e}")


if __name__ == "__main__":
    main()
