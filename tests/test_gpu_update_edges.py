"""The update chain at its launch edges, against float64 references that share no code with it
(tests/update_ref.py; the references' own checks, the floors and the input conditions: test_update_ref_cpu.py).

  A  nslam_cam_grad_parts over 1 .. 32 workgroups and the stride pass beyond 32 * 1024 points, with 1 .. 4 d/dpts
     buffers; repeated calls and launches of different widths on one ws / ticket.
  B  nslam_cam_grad_batch: 1, 4 and 32 cameras, slices out of order with a gap of NaN rays, c2w rows of 12 and 16
     floats, per-camera ws rows and tickets; each row against the reference and, in bits, nslam_cam_grad_parts.
  C  nslam_cam_grad_step / _lr2 over 6 synthetic iterations: the gradient against cam_grad_ref, the tail
     (camera, moments, step, loss, best loss, best pose) against cam_tail_ref fed the gradient the kernel published.
  D  nslam_adam_step: workgroup edges of dense and row-masked segments, 16 segments, live counts around the 512
     workgroups of an n_live segment, gradients far below eps, zero_grad, the launch without a ticket, the mirror.

ws and every buffer tail the contract says is never read hold NaN.  Bars: update_ref's docstring; DESIGN 7e-2
tabulates floors and what the kernels measured.
"""
import importlib

import pytest
import torch

import update_ref as ur

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
NAN = float("nan")


def dev(t):
    return t.to(DEV) if t is not None else None


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ A one camera
class CamRun:
    """One camera's inputs on the device: the pose is the kernel's own (ops.cam_pose), rays_d the float32
    R . dir of the restated pose; the reference sees exactly what the kernel sees."""

    def __init__(self, c):
        self.cam = dev(c["cam"])
        self.c2w = P.ops.cam_pose(self.cam, torch.empty(3, 4, dtype=torch.float32, device=DEV))
        rd = ur.rays_of(ur.camera_pose(c["cam"]), c["dirs"]).contiguous()
        self.rd, self.z = dev(rd), dev(c["z"])
        self.g_pts = [dev(g) for g in c["g_pts"]]
        self.ref = ur.cam_grad_ref(c["cam"], self.c2w.cpu(), c["g_pts"], c["z"], rd)

    def parts(self, ws, ticket):
        out = torch.full((7,), NAN, device=DEV)
        return P.ops.cam_grad_parts(self.cam, self.c2w, self.g_pts, self.z, self.rd, out, ws, ticket)


def check_cam_grad(got, ref, what):
    """|got - ref| <= 4 * 2^-24 * max|ref_part|, the quaternion and the translation elements separately."""
    got, worst = got.detach().cpu().double(), 0.0
    assert bool(torch.isfinite(got).all()), (what, got)
    for name, sl in (("quaternion", slice(0, 4)), ("translation", slice(4, 7))):
        err, scale = float((got[sl] - ref[sl]).abs().max()), float(ref[sl].abs().max())
        print(f"cam_grad {what} {name}: err {err:.3e} = {err / (ur.CAM_BAR * scale):.3f} of the bar")
        assert err <= ur.CAM_BAR * scale, (what, name, err, ur.CAM_BAR * scale)
        worst = max(worst, err / (ur.CAM_BAR * scale))
    return worst


def fresh_ws(n=1):
    return (torch.full((n * P.ops.CAM_GRAD_WS_DOUBLES,), NAN, dtype=torch.float64, device=DEV),
            torch.zeros(n, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("n,S", ur.CAM_SHAPES)
def test_cam_grad_parts_vs_float64(n, S):
    for nbuf in ur.cam_buffers(n, S):
        run = CamRun(ur.cam_case(n, S, nbuf, ur.cam_quat_of(n, S)))
        ws, ticket = fresh_ws()
        outs = []
        for rep in range(3):  # the same ws and ticket: the call re-arms them
            if rep == 2:
                ws.fill_(NAN)
            outs.append(run.parts(ws, ticket))
            assert int(ticket) == 0, (nbuf, rep)
        check_cam_grad(outs[0], run.ref, f"({n},{S}) x{nbuf}")
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])


def test_cam_grad_parts_widths_share_workspace():
    """32, 2, 1 and 32 workgroups in turn on one ws and ticket: no launch sees another's partials."""
    ws, ticket = fresh_ws()
    for n, S in ur.CAM_SEQUENCE:
        run = CamRun(ur.cam_case(n, S, 2, "big", seed=3))
        check_cam_grad(run.parts(ws, ticket), run.ref, f"sequence ({n},{S})")
        assert int(ticket) == 0


# ------------------------------------------------------------------------------------------------ B batch
@pytest.mark.parametrize("n_cams,n_per,S,nbuf,rows4", ur.BATCH_CASES)
def test_cam_grad_batch_vs_float64_and_parts(n_cams, n_per, S, nbuf, rows4):
    c = ur.batch_case(n_cams, n_per, S, nbuf)
    cams = dev(c["cams"])
    c2w = P.ops.cam_pose_batch(cams, torch.full((n_cams, rows4, 4), NAN, dtype=torch.float32, device=DEV))
    rd = torch.full_like(c["dirs"], NAN)
    for k in range(n_cams):
        rays, _ = ur.batch_slice(c, k)
        rd[rays] = ur.rays_of(ur.camera_pose(c["cams"][k]), c["dirs"][rays])
    z_d, rd_d, gp_d = dev(c["z"]), dev(rd), [dev(g) for g in c["g_pts"]]
    ws, tickets = fresh_ws(n_cams)
    outs = []
    for rep in range(2):
        out = torch.full((n_cams, 7), NAN, device=DEV)
        outs.append(P.ops.cam_grad_batch(cams, c2w, c["ray_begin"], n_per, gp_d, z_d, rd_d, out, ws, tickets))
        assert int(tickets.abs().sum()) == 0
    assert same_bits(outs[0], outs[1])
    if rows4 == 4:
        assert bool(torch.isnan(c2w[:, 3]).all())
    c2w_h = c2w.cpu()
    ws1, ticket1 = fresh_ws()
    for k in range(n_cams):
        rays, pts = ur.batch_slice(c, k)
        ref = ur.cam_grad_ref(c["cams"][k], c2w_h[k, :3], [g[pts] for g in c["g_pts"]], c["z"][rays], rd[rays])
        check_cam_grad(outs[0][k], ref, f"batch {n_cams}x({n_per},{S}) camera {k}")
        one = P.ops.cam_grad_parts(cams[k], c2w[k, :3], [g[pts] for g in gp_d], z_d[rays], rd_d[rays],
                                   torch.full((7,), NAN, device=DEV), ws1, ticket1)
        assert same_bits(outs[0][k], one), k


# ------------------------------------------------------------------------------------------------ C fused tail
def check_adam(got, ref, floor, what):
    """Elementwise max-abs against the float64 reference: 4 x the case's floor."""
    err = float((got.detach().cpu().double().reshape(-1) - ref.reshape(-1)).abs().max())
    assert err <= 4 * floor, (what, err, 4 * floor)
    return err


@pytest.mark.parametrize("n_loss", ur.TAIL_LOSS_LENGTHS)
@pytest.mark.parametrize("mode", sorted(ur.TAIL_MODES))
@pytest.mark.parametrize("n,S", ur.TAIL_SHAPES)
def test_cam_grad_step_vs_references(n, S, mode, n_loss):
    two_rates, before = ur.TAIL_MODES[mode]
    lr, lr_quat = ur.TAIL_LR, (4 * ur.TAIL_LR if two_rates else ur.TAIL_LR)
    c = ur.tail_case(n, S, n_loss)
    cam = dev(c["cam"]).clone()
    z = dev(c["z"])
    ex, ex2, stp = (torch.zeros(k, dtype=torch.float32, device=DEV) for k in (7, 7, 1))
    loss_out = torch.full((), NAN, dtype=torch.float64, device=DEV)
    best_loss = torch.full((), ur.TAIL_BEST0, dtype=torch.float64, device=DEV)
    best = torch.full((7,), NAN, device=DEV)
    ws, ticket = fresh_ws()
    g_cams, trace, worst_g = [], [], 0.0
    for it in range(ur.K_STEPS):
        cam_h = cam.cpu()
        c2w = P.ops.cam_pose(cam, torch.empty(3, 4, dtype=torch.float32, device=DEV))
        rd = ur.rays_of(ur.camera_pose(cam_h), c["dirs"]).contiguous()
        g_cam = torch.full((7,), NAN, device=DEV)
        ws.fill_(NAN)
        P.ops.cam_grad_step(cam, c2w, [dev(g) for g in c["g_pts"][it]], z, dev(rd), g_cam, ws, ticket,
                            (ex, ex2, stp, lr, *ur.BETAS, ur.EPS), dev(c["ray_loss"][it]), loss_out, best_loss, best,
                            lr_quat=lr_quat if two_rates else None, best_before_step=before)
        # (a) the gradient, at the camera the kernel read
        ref_g = ur.cam_grad_ref(cam_h, c2w.cpu(), c["g_pts"][it], c["z"], rd)
        worst_g = max(worst_g, check_cam_grad(g_cam, ref_g, f"tail ({n},{S}) it {it}"))
        assert int(ticket) == 0
        g_cams.append(g_cam.cpu())
        trace.append({"before": cam_h, "cam": cam.cpu(), "exp_avg": ex.cpu(), "exp_avg_sq": ex2.cpu(), "step": float(stp),
                      "loss": float(loss_out), "best_loss": float(best_loss), "best": best.cpu()})
    # (b) the tail, against the reference loop fed the published gradients
    p64, r64, floors = ur.tail_expect(c["cam"], g_cams, c["ray_loss"], lr, lr_quat, before)
    errs = {"cam": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    set_at = []
    for it, t in enumerate(trace):
        assert t["step"] == it + 1
        errs["cam"] = max(errs["cam"], check_adam(t["cam"], p64["cam"][it], floors["cam"], ("cam", it)))
        for k in ("exp_avg", "exp_avg_sq"):
            errs[k] = max(errs[k], check_adam(t[k], r64[k][it], floors[k], (k, it)))
        want = p64["loss"][it]
        if want != want:
            assert t["loss"] != t["loss"], it
        else:
            assert abs(t["loss"] - want) <= 1e-12 * abs(want), (it, t["loss"], want)
        prev = trace[it - 1]["best_loss"] if it else ur.TAIL_BEST0
        if t["best_loss"] != prev:
            set_at.append(it)
            assert t["best_loss"] == t["loss"]  # the kernel's own sum, in bits
            assert same_bits(t["best"], t["before"] if before else t["cam"]), it
        elif it:
            assert same_bits(t["best"], trace[it - 1]["best"]), it
    assert set_at == p64["set_at"] == ([0, 2] if n_loss else [0])
    want_best = p64["best_loss"][-1]
    assert abs(trace[-1]["best_loss"] - want_best) <= 1e-12 * abs(want_best)
    check_adam(trace[-1]["best"], p64["best"][-1], floors["cam"], "best pose")
    # the two rates, directly: the first Adam step moves an element by its rate
    moved = (trace[0]["cam"].double() - c["cam"].double()).abs()
    rates = torch.tensor([lr_quat] * 4 + [lr] * 3, dtype=torch.float64)
    assert float(((moved - rates).abs() / rates).max()) < 1e-3, moved
    print(f"tail ({n},{S}) {mode} n_loss={n_loss}: g_cam {worst_g:.3f} of bar; " +
          "; ".join(f"{k} err {errs[k]:.2e} floor {floors[k]:.2e}" for k in errs))


# ------------------------------------------------------------------------------------------------ D Adam
class AdamRun:
    """The segments of an update_ref Adam case on the device behind one FusedAdam."""

    def __init__(self, segs, n_live=None):
        self.segs, self.params, self.rows, groups = segs, [], [], []
        for s in segs:
            p = dev(s["p0"]).clone(memory_format=torch.preserve_format)
            grp = {"params": [p], "lr": s["lr"]}
            rows = dev(s["rows"])
            if rows is not None:
                grp["rows"] = rows
                if n_live is not None:
                    grp["n_live"] = n_live
            self.params.append(p)
            self.rows.append(rows)
            groups.append(grp)
        self.opt = P.ops.FusedAdam(groups, betas=ur.BETAS, eps=ur.EPS)
        self.opt.init_state()

    def grads(self, it, keep=None):
        """{param: device gradient} of step `it` (a copy: zero_grad may clear it); keep: also store them here."""
        out = {}
        for s, p in zip(self.segs, self.params):
            g = s["grads"][it]
            if g is not None:
                out[p] = dev(g).clone(memory_format=torch.preserve_format)
        if keep is not None:
            keep.append(out)
        return out

    def run(self, **kw):
        for it in range(ur.K_STEPS):
            self.opt.step(grads=self.grads(it), **kw)
        return self

    def vector(self, i):
        p = self.params[i]
        return ur.rows_view(p)[self.rows[i].long()] if self.rows[i] is not None else p

    def state(self, i):
        return self.opt.state_of(self.params[i])

    def check(self, name, what=None):
        """Every segment against the case's references and bars; rows outside a row list bit-unchanged."""
        refs, floors = ur.adam_expect(name)
        errs = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
        for i, (s, r) in enumerate(zip(self.segs, refs)):
            m, v, step = self.state(i)
            assert float(step) == r["steps"], (s["name"], float(step))
            for k, got in (("p", self.vector(i)), ("exp_avg", m), ("exp_avg_sq", v)):
                errs[k] = max(errs[k], check_adam(got, r[k], floors[k], (name, s["name"], k)))
            if self.rows[i] is not None:
                other = torch.ones(ur.rows_view(s["p0"]).shape[0], dtype=torch.bool)
                other[s["rows"].long()] = False
                assert same_bits(ur.rows_view(self.params[i]).cpu()[other], ur.rows_view(s["p0"])[other]), s["name"]
        print(f"adam {what or name}: " + "; ".join(f"{k} err {errs[k]:.2e} floor {floors[k]:.2e}" for k in errs))
        return errs


@pytest.mark.parametrize("name", ["dense", "rows_dense", "rows_compact"])
def test_adam_workgroup_edges(name):
    """Dense segments of 1 .. 4099 elements (a workgroup covers 1024), one skipping odd steps; row-masked
    segments of 1 .. 257 rows (a workgroup covers 128) with a dense and with a compact gradient."""
    AdamRun(ur.adam_case(name)).run().check(name)


def test_adam_segment_limit():
    AdamRun(ur.adam_case("seg_limit")).run().check("seg_limit")
    over = AdamRun(ur._case_seg_limit(17))
    with pytest.raises(ValueError):
        over.opt.step(grads=over.grads(0))


def test_adam_gradient_scale():
    """Gradients of 1e-12 (eps dominates the denominator); an element whose gradient and moments are zero keeps
    its bits, one whose gradient stops at step 2 goes on moving on its momentum, as the reference's does."""
    run = AdamRun(ur.adam_case("grad_scale")).run()
    run.check("grad_scale")
    s = run.segs[0]
    never = torch.arange(s["p0"].numel()) % 7 == 0
    assert same_bits(run.params[0].cpu()[never], s["p0"][never])
    m, v, _ = run.state(0)
    assert float(m.cpu()[never].abs().max()) == 0.0 and float(v.cpu()[never].abs().max()) == 0.0


def test_adam_zero_grad():
    """zero_grad: exactly the gradient elements the update read are 0 afterwards (a dense, a row-masked dense
    and a compact gradient); the dense gradient outside the rows keeps its bits (NaN)."""
    run, kept = AdamRun(ur.adam_case("zero_grad")), []
    for it in range(ur.K_STEPS):
        run.opt.step(grads=run.grads(it, keep=kept), zero_grad=True)
    run.check("zero_grad")
    for it, gd in enumerate(kept):
        for s, p, rows in zip(run.segs, run.params, run.rows):
            g = gd[p].cpu()
            if rows is None or s["compact"]:
                assert float(g.abs().max()) == 0.0, (it, s["name"])
            else:
                mask = torch.zeros(ur.rows_view(g).shape[0], dtype=torch.bool)
                mask[s["rows"].long()] = True
                assert float(ur.rows_view(g)[mask].abs().max()) == 0.0, (it, s["name"])
                assert same_bits(ur.rows_view(g)[~mask], ur.rows_view(s["grads"][it])[~mask]), (it, s["name"])
    # a live count: the compact gradient past the live rows is not cleared
    segs = [ur.adam_case("zero_grad")[2]]
    live = 130
    run = AdamRun(segs, n_live=torch.tensor([live], dtype=torch.int64, device=DEV))
    g = run.grads(0)
    run.opt.step(grads=g, zero_grad=True)
    g = g[run.params[0]].cpu()
    assert float(g[:live].abs().max()) == 0.0 and same_bits(g[live:], segs[0]["grads"][0][live:])


def test_adam_without_ticket():
    """nslam_adam_step with a NULL ticket (k_adam + k_adam_steps) on FusedAdam.segments()' structs: the bits and
    step counts of the ticket path, and the reference's values."""
    with_ticket = AdamRun(ur.adam_case("no_ticket")).run()
    raw = AdamRun(ur.adam_case("no_ticket"))
    L = P._lib.lib()
    for it in range(ur.K_STEPS):
        structs = raw.opt.segments(raw.grads(it))  # (the gradients stay alive in the tuples)
        arr = (P._lib.NslamAdamSeg * len(structs))(*[s for s, _, _ in structs])
        rc = L.nslam_adam_step(arr, len(structs), *ur.BETAS, ur.EPS, 0, None, P._lib.stream_ptr(DEV))
        assert rc == 0
        torch.cuda.synchronize()
    raw.check("no_ticket", "no_ticket (NULL ticket)")
    for i in range(len(raw.segs)):
        assert same_bits(raw.params[i], with_ticket.params[i])
        for a, b in zip(raw.state(i), with_ticket.state(i)):
            assert same_bits(a, b)


def test_adam_mirror():
    """A dense segment of 1025 elements with mirror slots (both, one, none): the mirror holds the parameter at
    the mapped places and keeps its bits everywhere else."""
    run = AdamRun(ur.adam_case("mirror"))
    idx = ur.mirror_index(1025, 3000)
    mirror = torch.full((3000,), -7.0, device=DEV)
    run.opt.set_mirror(run.params[0], dev(idx), mirror)
    run.run().check("mirror")
    got, p = mirror.cpu(), run.params[0].cpu()
    touched = torch.zeros(3000, dtype=torch.bool)
    for slot in (0, 1):
        has = idx[:, slot] >= 0
        touched[idx[has, slot].long()] = True
        assert same_bits(got[idx[has, slot].long()], p[has])
    assert int(touched.sum()) == int((idx >= 0).sum()) and bool((got[~touched] == -7.0).all())


@pytest.fixture(scope="module")
def n_live_inputs():
    """The capacity case on the device, once: the grid, the row list and the K_STEPS compact gradients."""
    s = ur.adam_case("n_live")[0]
    return s, [dev(g) for g in s["grads"]]


@pytest.mark.parametrize("count", ur.N_LIVE_COUNTS)
def test_adam_live_count_vs_float64(n_live_inputs, count):
    """A segment sized for 70000 rows (547 workgroups' worth, capped at 512 that stride the live rows) at live
    counts around the workgroup (128 rows) and the cap (65536 rows; 65537: a second pass of one row); a count
    above the capacity is clamped.  Live rows against float64 Adam; the gradient past them is NaN; the state
    past them and the grid rows of the list's tail keep their bits."""
    s, grads = n_live_inputs
    live = min(count, ur.N_LIVE_CAP)
    run = AdamRun([s], n_live=torch.tensor([count], dtype=torch.int64, device=DEV))
    m, v, step = run.state(0)
    m[live * ur.ROW_LEN:] = -7.0
    v[live * ur.ROW_LEN:] = -7.0
    for it in range(ur.K_STEPS):
        g = grads[it].clone()
        g[live:] = NAN
        run.opt.step(grads={run.params[0]: g})
    assert float(step) == ur.K_STEPS
    refs, floors = ur.adam_expect("n_live")
    got = {"p": run.vector(0), "exp_avg": m.view(-1, ur.ROW_LEN), "exp_avg_sq": v.view(-1, ur.ROW_LEN)}
    errs = {k: (check_adam(got[k][:live], refs[0][k][:live], floors[k], (count, k)) if live else 0.0) for k in got}
    print(f"adam n_live={count}: " + "; ".join(f"{k} err {errs[k]:.2e} floor {floors[k]:.2e}" for k in errs))
    assert bool((m[live * ur.ROW_LEN:] == -7.0).all()) and bool((v[live * ur.ROW_LEN:] == -7.0).all())
    tail = s["rows"][live:].long()
    assert same_bits(ur.rows_view(run.params[0]).cpu()[tail], ur.rows_view(s["p0"])[tail])
