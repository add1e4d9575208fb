"""The fused point query in the trained regime (tests/golden/trained_scene.py: every pts_linears / output_linear
bias non-zero, grids N(0, 0.5^2)) — the regime every real run is in and oracle.init_decoders' zero biases never
reach — against the reference's own outputs (tests/golden/trained_fixtures.*.npz) and tests/nice_ref.py in float64.

  a. parity           Renderer.eval_points / ops.query_points, four stages: raw and every gradient vs the fixture
  b. tile independence a point's raw does not depend on the tile or lane it lands in: prefixes of 1, 31, 32, 33
                      points and a permutation, bit for bit; the gradients of the 1- and 33-point prefixes
  c. forward variants nslam_query_fwd_ws UNITS / PC / PARTS, with and without defer_occ: one against the fixture,
                      the others bit-identical to it in raw, saved masks and tape
  d. backward paths   ray form (7 x 48): the recompute backward (nslam_query_bwd), the mask-only merged backward
                      with nslam_color_wgrad from the tape, and the live-point form with a third of the voxels
  f. engine           one MappingEngine.iteration per stage and one TrackingEngine.iteration vs the float32 oracle
                      step, then two Adam steps with every decoder of the stage trainable: packed == repack()
(e, the direct sub-decoder calls, is tests/test_gpu_decoders.py parametrised over this scene.)

Bars: max(the project's bar for the class, 4 x the fixture's recorded float32 floor) — forward rel-L2 1e-4 and
max-abs 2e-4 (per row), gradients per test_gpu_parity.tol_for.  d/dpts leaves out trained_scene.LATTICE (points on
grid nodes, where the trilinear weights have a kink and float32 / float64 pick different cells) by that fixed index
list; nothing else is ever left out.  No test uses more than the 336 ray-form points.
"""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_l2
from oracle import nslam_oracle as orc
from test_gpu_configs import TOL, check, compact, decoder_flat, frustum_rows, oracle_batch, oracle_step, run_engine
from test_gpu_dropins import oracle_samples
from test_gpu_parity import FWD_ABS, FWD_REL, make_renderer, tol_for

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nice_ref as ref  # noqa: E402
import scenes  # noqa: E402
import trained_scene as sc  # noqa: E402

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
GRID_KEYS = ("grid_coarse", "grid_middle", "grid_fine", "grid_color")


@pytest.fixture(scope="module")
def fx():
    return load_golden("trained_fixtures")


@pytest.fixture(scope="module")
def scene():
    return SimpleNamespace(bound=torch.from_numpy(sc.bound()),
                           sd={k: torch.from_numpy(v) for k, v in sc.decoders().items()},
                           grids={k: torch.from_numpy(v) for k, v in sc.grids().items()},
                           pts=torch.from_numpy(sc.points()))


@pytest.fixture(scope="module")
def ray_ref(scene):
    """stage -> (raw, gradients) of tests/nice_ref.py in float64 on the 336 ray-form points (computed once)."""
    cache = {}

    def get(stage):
        if stage not in cache:
            cot = torch.from_numpy(sc.cotangent(stage, (sc.N_RAYS * sc.N_SAMPLES, 4)))
            cache[stage] = ref.vjp(scene.sd, scene.grids, torch.from_numpy(sc.ray_points()), cot, stage, scene.bound,
                                   torch.float64)
        return cache[stage]

    return get


def make_nice(scene):
    nice = P.NICE(dim=3, c_dim=32, coarse_grid_len=sc.LEN["coarse"], middle_grid_len=sc.LEN["middle"],
                  fine_grid_len=sc.LEN["fine"], color_grid_len=sc.LEN["color"], hidden_size=32, coarse=True)
    nice.load_state_dict({k: v.clone() for k, v in scene.sd.items()})
    nice.set_bound(scene.bound)
    return nice.to(DEV)


def dev_grids(scene, grad=True):
    return {k: v.to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(grad)
            for k, v in scene.grids.items()}


def bar(cls, floor):
    return max(cls, 4.0 * float(floor))


def where(row):
    return f"row {row} (tile {row // 32}, lane {row % 32})"


def rows_err(got, want, rows=None):
    """(rel_l2, max_abs, worst row) of a per-point quantity [M, k] over `rows` (all when None)."""
    got, want = got.detach().cpu().double(), torch.as_tensor(want).double()
    idx = np.arange(got.shape[0]) if rows is None else np.asarray(rows)
    d = (got[idx] - want[idx]).reshape(idx.size, -1).abs().max(1).values
    return rel_l2(got[idx], want[idx]), float(d.max()), int(idx[int(d.argmax())])


def forward_errors(tag, raw, want, floor, floor_max, fails):
    """Forward values: rel-L2 over every row, the same over the in-bound rows alone (the 100s of the out-of-bound
    rows carry most of the norm) and each row's max-abs."""
    want = torch.as_tensor(want)
    r, m, row = rows_err(raw, want)
    inb = np.nonzero((want[:, 3] != 100).numpy())[0]
    ri = rows_err(raw, want, inb)[0]
    print(f"{tag}: rel_l2 {r:.3e} (in-bound rows {ri:.3e}) max_abs {m:.3e} at {where(row)}")
    if max(r, ri) > bar(FWD_REL, floor):
        fails.append(f"{tag}: rel_l2 {r:.3e} / in-bound {ri:.3e} > {bar(FWD_REL, floor):.1e}; worst {where(row)}")
    if not m <= bar(FWD_ABS, floor_max):
        fails.append(f"{tag}: max_abs {m:.3e} > {bar(FWD_ABS, floor_max):.1e} at {where(row)}")


def grad_error(tag, name, got, want, floor, fails, rows=None):
    """A gradient against its reference at max(tol_for(name), 4 x floor); per-point ones name the worst row."""
    b = bar(tol_for(name), floor)
    if got is None:
        fails.append(f"{tag}.{name}: missing")
        return
    if name == "pts":
        r, m, row = rows_err(got, want, rows)
        loc = where(row)
    else:
        got, want = got.detach().cpu().double(), torch.as_tensor(want).double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        r = rel_l2(got, want)
        d = (got - want).abs().reshape(-1)
        m, loc = float(d.max()), f"flat index {int(d.argmax())}"
    print(f"{tag}.{name}: rel_l2 {r:.3e} (bar {b:.1e}) max_abs {m:.3e}")
    if not r <= b:
        fails.append(f"{tag}.{name}: rel_l2 {r:.3e} > {b:.1e}; worst {loc}, max_abs {m:.3e}")


def query_grads(nice, grids, stage, pts, cot, bound):
    """raw and {name: gradient} of ops.query_points (NICE.forward) for pts [n,3] float64 on the device."""
    p = pts.to(DEV).requires_grad_(True)
    raw = nice(p, grids, stage=stage, oob_bound=bound)
    params = dict(nice.named_parameters())
    names = ["pts"] + list(grids) + list(params)
    tens = [p] + list(grids.values()) + list(params.values())
    grads = torch.autograd.grad(raw, tens, cot.to(DEV), allow_unused=True)
    return raw.detach(), dict(zip(names, grads))


def compare_grads(tag, got, want, floors, fails, rows=None):
    """Every gradient of `got` against `want` ({name: tensor}); one the reference does not have must be None / 0."""
    for name, g in got.items():
        if name not in want:
            if g is not None and float(g.abs().max()) != 0.0:
                fails.append(f"{tag}.{name}: a gradient where the reference has none")
            continue
        grad_error(tag, name, g, want[name], floors(name), fails, rows if name == "pts" else None)
    assert set(want) <= set(got), sorted(set(want) - set(got))


# ------------------------------------------------------------------------------------------------------------
# a. parity, four stages
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ref.STAGES)
def test_eval_points_matches_reference(fx, scene, stage):
    nice, grids = make_nice(scene), dev_grids(scene)
    r = make_renderer(P, scene.bound)
    case = "eval." + stage
    p = scene.pts.to(DEV).requires_grad_(True)
    raw = r.eval_points(p, nice, grids, stage, DEV)
    fails = []
    forward_errors(case + ".raw", raw, fx[case + ".raw"], fx[case + ".floor.raw"], fx[case + ".floor_max.raw"], fails)
    assert torch.equal(raw[:, 3].detach().cpu() == 100, torch.from_numpy(fx[case + ".raw"][:, 3] == 100))
    params = dict(nice.named_parameters())
    names = ["pts"] + list(grids) + list(params)
    grads = torch.autograd.grad(raw, [p] + list(grids.values()) + list(params.values()),
                                torch.from_numpy(fx[case + ".cot"]).to(DEV), allow_unused=True)
    want = {k[len(case) + 6:]: v for k, v in fx.items() if k.startswith(case + ".grad.")}
    compare_grads(case, dict(zip(names, grads)), want, lambda n: fx[f"{case}.floor.grad.{n}"], fails, sc.NOT_LATTICE)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------
# b. tile independence
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ref.STAGES)
def test_raw_does_not_depend_on_tile_or_lane(scene, stage):
    nice, grids = make_nice(scene), dev_grids(scene, grad=False)
    pts = scene.pts.to(DEV)
    with torch.no_grad():
        full = nice(pts, grids, stage=stage, oob_bound=scene.bound)
        for n in (1, 31, 32, 33):
            part = nice(pts[:n].contiguous(), grids, stage=stage, oob_bound=scene.bound)
            bad = torch.nonzero((part != full[:n]).any(1)).reshape(-1)
            assert bad.numel() == 0, f"prefix of {n}: differs from the {sc.M}-point call at {where(int(bad[0]))}"
        perm = torch.from_numpy(sc.permutation()).to(DEV)
        moved = nice(pts[perm].contiguous(), grids, stage=stage, oob_bound=scene.bound)
    bad = torch.nonzero((moved != full[perm]).any(1)).reshape(-1)
    if bad.numel():
        i = int(bad[0])
        pytest.fail(f"permuted call: its {where(i)} differs from {where(int(perm[i]))} of the ordered call")
    assert 0 < int((full[:, 3] == 100).sum()) == sc.OOB.size


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("stage", ref.STAGES)
def test_prefix_gradients_match_float64(fx, scene, stage, n):
    """A batch of one point (31 idle lanes) and of one full tile and one point: every gradient against the
    float64 restatement on that prefix (rows 0 .. 32 are ordinary interior points)."""
    assert n <= int(sc.LATTICE.min()) and not np.intersect1d(np.arange(n), sc.OOB).size
    nice, grids = make_nice(scene), dev_grids(scene)
    cot = torch.from_numpy(sc.cotangent(stage)[:n].copy())
    raw, got = query_grads(nice, grids, stage, scene.pts[:n].contiguous(), cot, scene.bound)
    raw64, want = ref.vjp(scene.sd, scene.grids, scene.pts[:n], cot, stage, scene.bound, torch.float64)
    case, fails = "eval." + stage, []
    forward_errors(f"{stage}[:{n}].raw", raw, raw64, fx[case + ".floor.raw"], fx[case + ".floor_max.raw"], fails)
    compare_grads(f"{stage}[:{n}]", got, want, lambda k: fx[f"{case}.floor.grad.{k}"], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------
# c. forward variants
# ------------------------------------------------------------------------------------------------------------
def fwd_ws(nice, grids, stage, pts, bound, split, defer):
    """nslam_query_fwd_ws (split) or nslam_query_fwd in pts form → (raw, deferred middle occupancy or None,
    saved masks, tape or None)."""
    ops, lib = P.ops, P._lib.lib()
    decs = ops.DEC_FOR_STAGE[stage]
    packers = {d: nice.decoder(d).packer() for d in decs}
    meta = ops.QueryMeta(stage, decs, packers, {d: ops.bound_list(nice.decoder(d).bound) for d in decs},
                         ops.bound_list(bound), None)
    packed = {d: packers[d].pack(list(nice.decoder(d).parameters())) for d in decs}
    cfg = ops.fill_cfg(meta, [(grids[k], None) for k in GRID_KEYS], packed, {}, False)
    n = pts.shape[0]
    saved = torch.zeros(lib.nslam_query_saved_size(n), dtype=torch.uint8, device=DEV)
    cfg.saved_masks = saved.data_ptr()
    tape = None
    if stage == "color":
        tape = torch.zeros(lib.nslam_query_tape_size(n) // 4, dtype=torch.float32, device=DEV)
        cfg.act_tape = tape.data_ptr()
    raw = torch.empty(n, 4, dtype=torch.float32, device=DEV)
    occ = ops.query_fwd_launch(cfg, pts, n, raw, split=split, defer_occ=defer)
    torch.cuda.synchronize()
    assert (occ is not None) == defer
    return raw, None if occ is None else occ.clone(), saved, tape


@pytest.mark.parametrize("stage", ["fine", "color"])
def test_forward_variants(fx, scene, stage):
    """The decoder-parallel forward against the fixtures, then itself with the occupancy combine deferred
    and the fused forward (one wave runs every decoder) against it: raw, masks and tape bit for bit."""
    nice, grids = make_nice(scene), dev_grids(scene, grad=False)
    pts = scene.pts.to(DEV).contiguous()
    case = "eval." + stage
    base = fwd_ws(nice, grids, stage, pts, scene.bound, True, False)
    fails = []
    forward_errors(case + ".raw[UNITS]", base[0], fx[case + ".raw"], fx[case + ".floor.raw"],
                   fx[case + ".floor_max.raw"], fails)
    assert not fails, "\n".join(fails)
    nt = (sc.M + 31) // 32
    decs = [P.ops.DEC_ID[d] for d in P.ops.DEC_FOR_STAGE[stage]]
    masks = lambda s: s.view(torch.int16).view(4, nt, 5, 64)[decs]  # noqa: E731  [decoder][tile][layer][lane]
    assert int((masks(base[2]) != 0).sum()) > 0
    for split, defer in ((True, False), (True, True), (False, False)):
        raw, occ, saved, tape = fwd_ws(nice, grids, stage, pts, scene.bound, split, defer)
        tag = f"{'units' if split else 'fused'} defer_occ {defer}"
        full = raw if not defer else torch.cat([raw[:, :3], (raw[:, 3] + occ)[:, None]], 1)
        bad = torch.nonzero((full != base[0]).any(1)).reshape(-1)
        assert bad.numel() == 0, f"{tag}: raw differs at {where(int(bad[0]))}"
        bad = torch.nonzero((masks(saved) != masks(base[2])).reshape(len(decs), nt, -1).any(2).any(0)).reshape(-1)
        assert bad.numel() == 0, f"{tag}: saved masks differ in tile {int(bad[0])}"
        if stage == "color":
            bad = torch.nonzero((tape != base[3]).view(nt, -1).any(1)).reshape(-1)
            assert bad.numel() == 0, f"{tag}: tape differs in tile {int(bad[0])}"


# ------------------------------------------------------------------------------------------------------------
# d. every backward path, ray form
# ------------------------------------------------------------------------------------------------------------
def dev_rays():
    o, d, z = sc.rays()
    return torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV).contiguous()


def decoder_errors(tag, nice, name, flat, want, floors, fails):
    """A decoder's flat gradient (named_parameters order), tensor by tensor."""
    off = 0
    for k, q in nice.decoder(name).named_parameters():
        key = f"{name}_decoder.{k}"
        grad_error(tag, key, flat[off:off + q.numel()].view(q.shape), want[key], floors(key), fails)
        off += q.numel()
    assert off == flat.numel()


def test_recompute_backward_ray_points(fx, scene, ray_ref):
    """nslam_query_bwd (the forward recomputed, parameter gradients of all three decoders) through _Query."""
    nice, grids = make_nice(scene), dev_grids(scene)
    raw64, want = ray_ref("color")
    cot = torch.from_numpy(sc.cotangent("color", (sc.N_RAYS * sc.N_SAMPLES, 4)))
    raw, got = query_grads(nice, grids, "color", torch.from_numpy(sc.ray_points()), cot, scene.bound)
    fails = []
    forward_errors("rays.raw", raw, raw64, fx["eval.color.floor.raw"], fx["eval.color.floor_max.raw"], fails)
    compare_grads("rays", got, want, lambda k: fx[f"eval.color.floor.grad.{k}"], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("stage", ["fine", "color"])
def test_mask_only_backward_and_color_wgrad(fx, scene, ray_ref, stage):
    """MappingEngine.query_fwd / query_bwd: nslam_query_bwd_decoders from the saved masks (every grid, d/dpts) and,
    in the colour stage, nslam_color_wgrad from the tape (the colour decoder's parameters)."""
    nice = make_nice(scene)
    c = dev_grids(scene, grad=False)
    eng = P.engine.MappingEngine(nice, c, scene.bound, 32, 16, device=DEV)
    ro, rd, z = dev_rays()
    raw64, want = ray_ref(stage)
    g_raw = torch.from_numpy(sc.cotangent(stage, (z.numel(), 4))).to(DEV)
    dn = ("color",) if stage == "color" else ()
    keys, _ = eng.grads_for(stage, dn)
    raw = eng.query_fwd(stage, ro, rd, z, tape=True)
    assert (eng._tape is not None) == (stage == "color")
    eng.gall.zero_()
    g_pts = eng.query_bwd(stage, ro, rd, z, g_raw, keys, dn, pts_grad=True)
    torch.cuda.synchronize()
    case, fails = "eval." + stage, []
    floors = lambda k: fx[f"{case}.floor.grad.{k}"]  # noqa: E731
    forward_errors(f"engine.{stage}.raw", raw, raw64, fx[case + ".floor.raw"], fx[case + ".floor_max.raw"], fails)
    grad_error("engine." + stage, "pts", g_pts, want["pts"], floors("pts"), fails)
    for k in keys:
        grad_error("engine." + stage, k, eng.ggrad[k], want[k], floors(k), fails)
    if stage == "color":
        decoder_errors("engine.color", nice, "color", eng.decs["color"].grad, want, floors, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("stage", ["fine", "color"])
def test_live_point_backward(fx, scene, ray_ref, stage):
    """nslam_query_bwd_decoders_live with slot maps that keep about a third of each grid's voxels: the compact
    gradients are the reference's rows, whichever points the lists drop."""
    nice = make_nice(scene)
    c = dev_grids(scene, grad=False)
    rows = {"grid_" + k: torch.from_numpy(sc.live_rows(k)).to(DEV) for k in ("middle", "fine", "color")}
    eng = P.engine.MappingEngine(nice, c, scene.bound, 32, 16, device=DEV, rows=rows)
    ro, rd, z = dev_rays()
    _, want = ray_ref(stage)
    g_raw = torch.from_numpy(sc.cotangent(stage, (z.numel(), 4))).to(DEV)
    keys, _ = eng.grads_for(stage, ())
    eng.query_fwd(stage, ro, rd, z, defer_occ=True)
    live = eng.live_lists(stage, ro, rd, z)
    eng.gall.zero_()
    eng.query_bwd(stage, ro, rd, z, g_raw, keys, (), live=live)
    torch.cuda.synchronize()
    n_live = [int(live[1][P.ops.DEC_ID[d]]) for d in P.ops.DEC_FOR_STAGE[stage]]
    print("live points per decoder:", n_live, "of", z.numel())
    assert all(0 < k <= z.numel() for k in n_live) and any(k < z.numel() for k in n_live)
    fails = []
    for k in keys:
        ref_rows = compact(want[k], rows[k].cpu())
        assert float(ref_rows.abs().max()) > 0
        grad_error("live." + stage, k, eng.ggrad[k], ref_rows, fx[f"eval.{stage}.floor.grad.{k}"], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------
# f. engine iterations and the Adam mirror
# ------------------------------------------------------------------------------------------------------------
CAM = scenes.TINY_CAM
N_PIX = 7  # x 48 samples = 336 points


def one_frame(scene, seed):
    b = scene.bound.numpy()
    # (a camera off the centre: from the centre the middle stage's rays saturate at their first samples and its
    # gradients vanish to 1e-23)
    c2w = scenes.look_pose(b.mean(1), 3.5, 0.1, (0.8, 0.5, 0.3))
    return (torch.from_numpy(scenes.box_depth(c2w, CAM, b, seed=seed, hole_frac=0.0)),
            torch.from_numpy(scenes.color_image(CAM, seed=seed + 1)), torch.from_numpy(c2w))


def step_float64(scene, ro, rd, gd, gc, stage):
    """The oracle's mapping step (test_gpu_configs.oracle_step: sampler, query, compositing, mapper loss) with the
    query, the compositing and the loss in float64 → (loss, grid gradients, decoder gradients).  What the float32
    oracle step differs from it by is that step's own noise floor."""
    pre = tuple(d + "_decoder." for d in ref.DECODERS_OF[stage])
    sdl = {k: (v.double().requires_grad_(True) if k.startswith(pre) else v) for k, v in scene.sd.items()}
    gl = {k: (v.double().requires_grad_(True) if k in ref.GRIDS_OF[stage] else v) for k, v in scene.grids.items()}
    z = orc.sample_z(ro, rd, None if stage == "coarse" else gd, scene.bound, 32, 16)
    pts = ro[:, None, :] + rd[:, None, :] * z[:, :, None]
    raw = ref.eval_points(sdl, pts.reshape(-1, 3), gl, stage, scene.bound, torch.float64)
    d, _, c, _ = orc.composite(raw.reshape(z.shape[0], z.shape[1], 4), z)
    loss = orc.mapper_loss(d, c, gd, gc, stage)
    loss.backward()
    return (float(loss.detach()), {k: gl[k].grad for k in ref.GRIDS_OF[stage]},
            {k: v.grad for k, v in sdl.items() if k.startswith(pre)})


@pytest.mark.parametrize("stage", ref.STAGES)
def test_mapping_iteration_and_adam_mirror(scene, stage):
    """One engine mapping iteration of 7 rays with every decoder of the stage trainable vs the float32 oracle step
    (tests/test_gpu_configs.py's comparison; bars: loss 1e-5, gradients max(its TOL, 4 x the oracle step's own
    float32 floor, measured here against the same step in float64 — the coarse stage's weights are ~1e-5 before an
    opaque out-of-bound sample, and float32 autograd through 1 - alpha + 1e-10 and the cumprod then carries a
    relative error of 2.7e-4 in the coarse grid's gradient, above that grid's 2e-4)), then two Adam steps: each
    trained decoder's packed copy, which Adam's mirror keeps current (its Bias and Bo sections too), equals a fresh
    repack() bit for bit."""
    frames = [one_frame(scene, 201)]
    fdev = [tuple(t.to(DEV) for t in f) for f in frames]
    pix = torch.randint(CAM["H"] * CAM["W"], (N_PIX,), generator=torch.Generator().manual_seed(202))
    trainable = P.ops.DEC_FOR_STAGE[stage]
    intr = (CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])

    def setup():
        nice, c = make_nice(scene), dev_grids(scene, grad=False)
        rows = None if stage == "coarse" else \
            frustum_rows(frames, {k: v for k, v in c.items() if k != "grid_coarse"}, scene.bound, CAM)
        return nice, c, rows

    nice, c, rows = setup()
    eng, snap, ray_loss, keep = run_engine(nice, c, scene.bound, fdev, pix, N_PIX, CAM, stage, rows, 32, 16, trainable)
    ro, rd, gd, gc, k_ref = oracle_batch(frames, pix, N_PIX, CAM, scene.bound)
    assert torch.equal(keep.bool().cpu(), k_ref) and ro.shape[0] >= 5
    loss, g, dec, _ = oracle_step(scene.sd, scene.grids, ro, rd, gd, gc, stage, scene.bound, 32, 16, trainable,
                                  coarse_bound=scene.bound * 2)
    _, g64, dec64 = step_float64(scene, ro, rd, gd, gc, stage)
    report = {"loss_rel": abs(float(ray_loss.sum()) - loss) / loss, "rays": int(ro.shape[0])}
    ok = report["loss_rel"] < 1e-5
    for k in g:
        want, w64 = (g[k], g64[k]) if rows is None else (compact(g[k], rows[k]), compact(g64[k], rows[k]))
        assert float(want.abs().max()) > 1e-4, (k, "the reference gradient is degenerate")
        report[k + ".floor"], report[k + ".vs_float64"] = rel_l2(want, w64), rel_l2(snap[k], w64)
        ok &= check(report, k, snap[k], want, bar(TOL[k], report[k + ".floor"]))
    for n in trainable:
        want, w64 = decoder_flat(nice, n, dec), decoder_flat(nice, n, dec64)
        assert float(want.abs().max()) > 1e-4, (n, "the reference gradient is degenerate")
        key = n + "_decoder"
        report[key + ".floor"], report[key + ".vs_float64"] = rel_l2(want, w64), rel_l2(snap["dec." + n], w64)
        ok &= check(report, key, snap["dec." + n], want, bar(TOL["decoder"], report[key + ".floor"]))
    print(report)
    assert ok, report

    nice, c, rows = setup()
    eng = P.engine.MappingEngine(nice, c, scene.bound, 32, 16, device=DEV, rows=rows)
    keys, dn = eng.grads_for(stage, trainable)
    assert dn == tuple(trainable)
    opt = P.ops.FusedAdam([{"params": [eng.decs[n].param], "lr": 0.005} for n in dn] +
                          [{"params": [c[k]], "lr": 0.005, **({"rows": rows[k]} if rows else {})} for k in keys])
    before = {n: eng.decs[n].packed.clone() for n in dn}
    for _ in range(2):
        eng.iteration(stage, fdev, pix.to(DEV), N_PIX, (CAM["H"], CAM["W"]), intr, opt, trainable_decoders=trainable,
                      use_gt_in_sampler=stage != "coarse")
    torch.cuda.synchronize()
    for n in dn:
        d = eng.decs[n]
        assert d.param in opt.mirrors, n
        got = d.packed.clone()
        d.repack()
        bad = torch.nonzero(got != d.packed).reshape(-1)
        L = d.packer.layout
        assert bad.numel() == 0, f"{n}: packed[{int(bad[0])}] is stale (Bias at {L['Bias']}, Bo at {L['Bo']})"
        for sec, size in (("Bias", 160), ("Bo", 4 if n == "color" else 1)):
            assert bool((got[L[sec]:L[sec] + size] != before[n][L[sec]:L[sec] + size]).any()), (n, sec, "not stepped")


def test_tracking_iteration(scene):
    """One TrackingEngine.iteration of 7 pixels vs the oracle's autograd replica on the same draws: the loss at
    1e-5 and the camera gradient at the project's bar for ray / point gradients (it is d/dpts pulled back through
    pts = o + d z and the pose), 5e-3."""
    depth, color, c2w = one_frame(scene, 211)
    nice = make_nice(scene)
    c = {k: v for k, v in dev_grids(scene, grad=False).items() if k != "grid_coarse"}
    H, W = CAM["H"], CAM["W"]
    intr = SimpleNamespace(fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"])
    eng = P.engine.TrackingEngine(nice, c, scene.bound, 32, 16, (H, W), (intr.fx, intr.fy, intr.cx, intr.cy),
                                  ignore_edge=(20, 20), w_color=0.5, handle_dynamic=True, use_color=True, device=DEV)
    cam0 = P.common.get_tensor_from_camera(c2w).float()
    cam = cam0.to(DEV).clone().requires_grad_(True)
    opt = P.ops.FusedAdam([{"params": [cam], "lr": 0.001}])
    pix = torch.randint(eng.n_window(), (N_PIX,), generator=torch.Generator().manual_seed(212))
    loss = float(eng.iteration(cam, depth.to(DEV), color.to(DEV), pix.to(DEV), opt))
    grad = cam.grad.detach().cpu().clone()
    camo = cam0.clone().requires_grad_(True)
    ro, rd, gd, gc = oracle_samples(intr, pix, 20, H - 20, 20, W - 20, orc.camera_from_tensor(camo), depth, color)
    keep = orc.inside_mask(ro, rd, gd, scene.bound)
    assert int(keep.sum()) >= 5
    ro, rd, gd, gc = ro[keep], rd[keep], gd[keep], gc[keep]
    grids = {k: v for k, v in scene.grids.items() if k != "grid_coarse"}
    d, v, col = orc.render_batch_ray(scene.sd, grids, rd, ro, "color", scene.bound, gd)
    ref_loss = orc.tracker_loss(d, v, col, gd, gc)
    ref_loss.backward()
    rel = abs(loss - float(ref_loss)) / abs(float(ref_loss))
    err = rel_l2(grad, camo.grad)
    print({"loss_rel": rel, "cam_grad": err, "rays": int(keep.sum())})
    assert float(camo.grad.abs().max()) > 0
    assert rel < 1e-5 and err <= 5e-3, (rel, err)
