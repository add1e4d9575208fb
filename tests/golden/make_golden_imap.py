"""Golden vectors for the iMAP* path, produced by the reference's own code (build container only; the .npz parts
it writes are what tests/test_imap_golden.py and tests/test_gpu_imap.py read).

Run:  PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imap.py

Cases (reference file:line they execute), inputs from imap_scene.py, the reference on the CPU in float32:
  mlp         config.get_model(cfg, nice=False) (conv_onet/config.py:28-32) with imap_scene.weights() loaded, through
              Renderer.eval_points (Renderer.py:23-61): raw of 333 points (out-of-bound ones, one on a face) and the
              VJP of a fixed cotangent to every parameter and to the points.
  composite   raw2outputs_nerf_color(occupancy=False) (common.py:204-245) at S = 32, 44, 70 with non-unit rays_d:
              depth, var, rgb, weights and the VJP to raw and rays_d.
  pdf         sample_pdf(z_mid, weights[..., 1:-1], 12, det=True) (common.py:19-63) and the sort of Renderer.py:186.
  render      Renderer.render_batch_ray (Renderer.py:63-198), 32 + 12 samples, with gt_depth and without: outputs and
              the VJP to every parameter, rays_o and rays_d.
  regulation  Renderer.regulation (Renderer.py:258-296) with its torch.rand draws recorded (t_rand).
  map         Mapper.optimize_map with nice=False (Mapper.py:230-540), 3 iterations on two 24x32 frames (one keyframe
              and the current frame), 64 pixels, without and with BA: the per-iteration losses, the parameters'
              update (final - initial; imap_scene.probe's part of it) and with BA the returned pose.  The pixel
              draws (select_uv) and the regulation's torch.rand draws are recorded.
  track       3 iterations of Tracker.optimize_cam_in_batch with nice=False (Tracker.py:71-128): losses and the
              camera tensor.
  The two loop cases use make_golden_loop.py's harness (FixedDraws for select_uv, CPU get_device, quat_from_c2w for
  get_tensor_from_camera: mathutils is absent).  Their floors come from the same loops replayed by imap_ref in
  float64 with the recorded draws.  They use imap_scene.loop_weights() (opaque rays), and the generator asserts the
  condition that makes them well-posed: in every render of every iteration no ray has a weight above 1e-6 in its
  last four samples.  There sample_pdf decides by `cdf <= 1` with a cdf whose last entry is 1 up to rounding, so the
  bin of the last new sample depends on the order in which the weights were summed (torch's vectorised CPU sum,
  a GPU reduction and a sequential loop differ); replaying the float32 loop with another order moved the third
  loss of a semi-transparent scene by 5e-4, ten times the floor, although no kernel output differed by more than
  2e-6.  With no weight at the far end the decision has no effect.
Nothing of the reference is copied or modified; it is imported and called (torch.rand is wrapped for the one
call that records it).

For every compared quantity q the fixture also holds `<case>.floor.<q>` = rel_l2(reference float32, imap_ref
float64), and `<case>.floor_max.<q>`, the same difference's largest absolute entry: the noise floor of one float32
evaluation, from which the tests derive their tolerances.  (The two differ most in `pdf`: where u = 1 meets a cdf
whose last entries round to just above or just below 1, the search lands one bin apart, so one sample of one ray
moves by 7.5e-4 between float32 and float64 while the rel-L2 stays at 2e-5.)  The
generator asserts the conditions under which that is meaningful: no pre-activation within 1e-6 of zero (ReLU masks
cannot differ), no sample_pdf denominator within 1e-7 of its 1e-5 switch, no point but the deliberate one within
1e-5 of a bound face.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import imap_ref as ref  # noqa: E402
import imap_scene as sc  # noqa: E402
import scenes  # noqa: E402

from src import config as ref_config  # noqa: E402  (reference)
from src.common import raw2outputs_nerf_color, sample_pdf  # noqa: E402  (reference)
from src.utils.Renderer import Renderer  # noqa: E402  (reference)

CFG = {"data": {"dim": 3}, "grid_len": {"coarse": 2, "middle": 0.32, "fine": 0.16, "color": 0.16},
       "model": {"c_dim": 32, "pos_embedding_method": "fourier"}, "coarse": False}


def ref_model(sd):
    m = ref_config.get_model(CFG, nice=False)
    assert sorted(m.state_dict()) == sorted(sd), sorted(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def ref_renderer(bound, n_importance=sc.N_IMPORTANCE):
    cfg = {"rendering": {"N_samples": sc.N_SAMPLES, "N_surface": 0, "N_importance": n_importance, "lindisp": False,
                         "perturb": 0.0}, "scale": 1, "occupancy": False}
    slam = SimpleNamespace(nice=False, bound=bound, **sc.CAM)
    return Renderer(cfg, None, slam)


def tsd(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def put(out, case, name, got32, ref64):
    out[f"{case}.{name}"] = got32.detach().numpy()
    out[f"{case}.floor.{name}"] = np.float64(ref.rel_l2(got32.detach(), ref64.detach()))
    out[f"{case}.floor_max.{name}"] = np.float64((got32.detach().double() - ref64.detach().double()).abs().max())


def check_points(p, bound, allow=()):
    d = torch.minimum((p - bound[:, 0]).abs(), (p - bound[:, 1]).abs()).min(1)[0]
    near = [int(i) for i in torch.nonzero(d < 1e-5).reshape(-1)]
    assert near == list(allow), near


def check_preact(sd, p):
    t = tsd(sd)
    h = torch.sin(p.float().double() @ t["embedder._B"].double())
    for i in range(4):
        a = torch.nn.functional.linear(h, t[f"pts_linears.{i}.weight"].double(), t[f"pts_linears.{i}.bias"].double())
        assert float(a.abs().min()) > 1e-6, (i, float(a.abs().min()))
        h = torch.relu(a)


def mlp_case(out, sd, bound):
    p = torch.from_numpy(sc.mlp_points())
    check_points(p, bound, allow=(sc.ON_FACE,))
    check_preact(sd, p)
    g = torch.from_numpy(sc.cotangent((p.shape[0], 4), 12))
    m, r = ref_model(sd), ref_renderer(bound)
    pr = p.clone().requires_grad_(True)
    raw = r.eval_points(pr, m, None, "color", "cpu")
    raw.backward(g)
    t64 = {k: v.clone().requires_grad_(True) for k, v in tsd(sd).items()}
    p64 = p.clone().requires_grad_(True)
    raw64 = ref.eval_points(t64, p64, bound, torch.float64)
    raw64.backward(g.double())
    put(out, "mlp", "raw", raw, raw64)
    put(out, "mlp", "g_p", pr.grad, p64.grad)
    for k, prm in m.state_dict(keep_vars=True).items():
        put(out, "mlp", "g." + k, prm.grad, t64[k].grad)
    out["mlp.n_outside"] = np.int64(int((raw[:, 3] == 100).sum()))
    assert 20 < out["mlp.n_outside"] < 200 and float(raw[sc.ON_FACE, 3].detach()) == 100.0


def composite_case(out):
    for S in (32, 44, 70):
        raw_np, z_np, d_np = sc.composite_inputs(S)
        n = raw_np.shape[0]
        gd, gv = torch.from_numpy(sc.cotangent(n, 50 + S, np.float64)), torch.from_numpy(sc.cotangent(n, 51 + S, np.float64))
        gc = torch.from_numpy(sc.cotangent((n, 3), 52 + S))
        res = []
        for dt in (torch.float32, torch.float64):
            raw = torch.from_numpy(raw_np).to(dt).requires_grad_(True)
            d = torch.from_numpy(d_np).to(dt).requires_grad_(True)
            z = torch.from_numpy(z_np)
            if dt == torch.float32:
                o = raw2outputs_nerf_color(raw * 1.0, z, d, occupancy=False, device="cpu")
            else:
                o = ref.composite_density(raw, z, d, dt)
            ((o[0] * gd).sum() + (o[1] * gv).sum() + (o[2] * gc.to(dt)).sum()).backward()
            res.append((o[0], o[1], o[2], o[3], raw.grad, d.grad))
        for name, a, b in zip(("depth", "var", "rgb", "weights", "g_raw", "g_rays_d"), *res):
            put(out, f"composite{S}", name, a, b)
        assert float(res[0][3][0].abs().max()) == 0.0 and float(res[0][3][1, 0]) == 1.0  # the two special rays


def pdf_case(out):
    z_np, w_np = sc.pdf_inputs()
    z, w = torch.from_numpy(z_np), torch.from_numpy(w_np)
    mid = .5 * (z[..., 1:] + z[..., :-1])
    zs = sample_pdf(mid, w[..., 1:-1], sc.N_IMPORTANCE, det=True, device="cpu")
    merged = torch.sort(torch.cat([z, zs], -1), -1)[0]
    _, denom = ref.sample_pdf_parts(mid, w[..., 1:-1], sc.N_IMPORTANCE, torch.float32)
    assert float((denom - 1e-5).abs().min()) > 1e-7, float((denom - 1e-5).abs().min())
    zs64 = ref.sample_pdf(mid, w[..., 1:-1], sc.N_IMPORTANCE, torch.float64)
    put(out, "pdf", "z_samples", zs, zs64)
    put(out, "pdf", "z_out", merged, torch.sort(torch.cat([z, zs64], -1), -1)[0])


def render_case(out, sd, bound):
    ro_np, rd_np, gt_np = sc.rays(50, 61)
    n = ro_np.shape[0]
    gd, gv = torch.from_numpy(sc.cotangent(n, 62, np.float64)), torch.from_numpy(sc.cotangent(n, 63, np.float64))
    gc = torch.from_numpy(sc.cotangent((n, 3), 64))
    for tag, gt_np_ in (("render_gt", gt_np), ("render_nogt", None)):
        gt = torch.from_numpy(gt_np_) if gt_np_ is not None else None
        m, r = ref_model(sd), ref_renderer(bound)
        ro, rd = torch.from_numpy(ro_np).requires_grad_(True), torch.from_numpy(rd_np).requires_grad_(True)
        depth, var, color = r.render_batch_ray(None, m, rd, ro, "cpu", "color", gt_depth=gt)
        ((depth * gd).sum() + (var * gv).sum() + (color * gc).sum()).backward()
        t64 = {k: v.clone().requires_grad_(True) for k, v in tsd(sd).items()}
        ro64, rd64 = torch.from_numpy(ro_np).requires_grad_(True), torch.from_numpy(rd_np).requires_grad_(True)
        d64, v64, c64, z64 = ref.render_batch_ray(t64, rd64, ro64, bound, gt, sc.N_SAMPLES, sc.N_IMPORTANCE,
                                                  torch.float64, want_z=True)
        ((d64 * gd).sum() + (v64 * gv).sum() + (c64 * gc.double()).sum()).backward()
        # conditions: the sampler's switch and the bound faces, on the float32 path's own samples
        d32, v32, c32, z32 = ref.render_batch_ray(tsd(sd), torch.from_numpy(rd_np), torch.from_numpy(ro_np), bound, gt,
                                                  sc.N_SAMPLES, sc.N_IMPORTANCE, torch.float32, want_z=True)
        pts = torch.from_numpy(ro_np)[:, None, :] + torch.from_numpy(rd_np)[:, None, :] * z32[..., None]
        check_points(pts.reshape(-1, 3), bound)
        zc = ref.coarse_z(torch.from_numpy(ro_np), torch.from_numpy(rd_np), bound, gt, sc.N_SAMPLES)
        pc = torch.from_numpy(ro_np)[:, None, :] + torch.from_numpy(rd_np)[:, None, :] * zc[..., None]
        rawc = ref.eval_points(tsd(sd), pc.reshape(-1, 3), bound).reshape(n, sc.N_SAMPLES, 4)
        wc = ref.composite_density(rawc, zc, torch.from_numpy(rd_np))[3]
        _, denom = ref.sample_pdf_parts(.5 * (zc[..., 1:] + zc[..., :-1]), wc[..., 1:-1], sc.N_IMPORTANCE)
        assert float((denom - 1e-5).abs().min()) > 1e-7
        put(out, tag, "depth", depth, d64)
        put(out, tag, "var", var, v64)
        put(out, tag, "color", color, c64)
        put(out, tag, "g_rays_o", ro.grad, ro64.grad)
        put(out, tag, "g_rays_d", rd.grad, rd64.grad)
        for k, prm in m.state_dict(keep_vars=True).items():
            put(out, tag, "g." + k, prm.grad, t64[k].grad)


def regulation_case(out, sd, bound):
    ro_np, rd_np, gt_np = sc.rays(40, 71, zero_frac=0.0)
    m, r = ref_model(sd), ref_renderer(bound)
    rec = {}
    real_rand = torch.rand

    def rand(*a, **k):
        rec["t"] = real_rand(*a, **k)
        return rec["t"]

    torch.manual_seed(72)
    torch.rand = rand
    try:
        sigma = r.regulation(None, m, torch.from_numpy(rd_np), torch.from_numpy(ro_np), torch.from_numpy(gt_np), "cpu")
    finally:
        torch.rand = real_rand
    (sigma.abs().sum()).backward()
    t64 = {k: v.clone().requires_grad_(True) for k, v in tsd(sd).items()}
    s64 = ref.regulation(t64, torch.from_numpy(rd_np), torch.from_numpy(ro_np), torch.from_numpy(gt_np), bound,
                         sc.N_SAMPLES, rec["t"], torch.float64)
    s64.abs().sum().backward()
    out["regulation.t_rand"] = rec["t"].numpy()
    put(out, "regulation", "sigma", sigma, s64)
    for k in ("embedder._B", "output_linear.weight"):  # (every parameter's VJP is pinned by the mlp and render cases)
        put(out, "regulation", "g." + k, m.state_dict(keep_vars=True)[k].grad, t64[k].grad)


class RecordRand:
    """torch.rand, with every draw kept."""

    def __enter__(self):
        self.log, self.real = [], torch.rand

        def rand(*a, **k):
            self.log.append(self.real(*a, **k))
            return self.log[-1]

        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand = self.real


def frame_tensors():
    c2w, depth, color = sc.frames()
    return [(torch.from_numpy(c2w[k]), torch.from_numpy(depth[k]), torch.from_numpy(color[k])) for k in range(2)]


def tail_is_empty(fn):
    """Run fn (an imap_ref float32 replay) and assert the loops' condition on every render it makes."""
    ref.TAIL_MASS = []
    try:
        fn()
        assert ref.TAIL_MASS and max(ref.TAIL_MASS) < 1e-6, ref.TAIL_MASS
    finally:
        ref.TAIL_MASS = None


def map_case(out, bound):
    import make_golden_loop as L  # (registers its stand-ins, imports the reference's Mapper and Tracker)
    sd = sc.loop_weights()
    cam = SimpleNamespace(**sc.CAM)
    fr = frame_tensors()
    for tag, ba in (("map", False), ("map_ba", True)):
        m, r = ref_model(sd), ref_renderer(bound)
        kf = [{"gt_c2w": fr[0][0], "idx": 0, "est_c2w": fr[0][0].clone(), "depth": fr[0][1], "color": fr[0][2]}]
        mp = object.__new__(L.ref_mapper_mod.Mapper)
        mp.__dict__.update(L._mapper_attrs(cam, bound, r, m, {}, pixels=sc.MAP_PIXELS, frustum=False, window=5))
        mp.__dict__.update(nice=False, occupancy=False, keyframe_selection_method="global", keyframe_dict=kf, BA=ba,
                           BA_cam_lr=sc.BA_CAM_LR, w_color_loss=sc.MAP_W_COLOR, stage="color",
                           cfg={"mapping": {"imap_decoders_lr": sc.MAP_LR}})
        orig_q = L.ref_mapper_mod.get_tensor_from_camera
        L.ref_mapper_mod.get_tensor_from_camera = L.quat_from_c2w
        losses = []
        np.random.seed(5)
        torch.manual_seed(81)
        try:
            with L.cpu_get_device(), L.fixed_draws(82) as fd, L.record_losses(losses), RecordRand() as rr:
                out_c2w = mp.optimize_map(sc.MAP_ITERS, 1.0, 5, fr[1][2], fr[1][1], fr[1][0], kf, [0], fr[1][0].clone())
        finally:
            L.ref_mapper_mod.get_tensor_from_camera = orig_q
        assert len(losses) == sc.MAP_ITERS and len(fd.log) == 2 * sc.MAP_ITERS and len(rr.log) == sc.MAP_ITERS
        draws = [(fd.log[2 * i], fd.log[2 * i + 1]) for i in range(sc.MAP_ITERS)]
        t64 = {k: v.double().clone().requires_grad_(True) for k, v in tsd(sd).items()}
        l64, cam64 = ref.map_loop(t64, bound, sc.CAM, fr, fr[1], draws, rr.log, sc.MAP_ITERS, sc.MAP_LR, sc.MAP_W_COLOR,
                                  sc.N_SAMPLES, sc.N_IMPORTANCE, ba_cam=L.quat_from_c2w(fr[1][0]) if ba else None,
                                  ba_lr=sc.BA_CAM_LR, dtype=torch.float64)
        t32 = {k: v.clone().requires_grad_(True) for k, v in tsd(sd).items()}
        tail_is_empty(lambda: ref.map_loop(t32, bound, sc.CAM, fr, fr[1], draws, rr.log, sc.MAP_ITERS, sc.MAP_LR,
                                           sc.MAP_W_COLOR, sc.N_SAMPLES, sc.N_IMPORTANCE,
                                           ba_cam=L.quat_from_c2w(fr[1][0]) if ba else None, ba_lr=sc.BA_CAM_LR))
        out[f"{tag}.draws"] = torch.stack(fd.log).numpy()
        out[f"{tag}.t_rand"] = torch.stack(rr.log).numpy()
        put(out, tag, "losses", torch.tensor(losses, dtype=torch.float64), torch.tensor(l64, dtype=torch.float64))
        for k, v in m.state_dict().items():
            init = torch.from_numpy(sd[k])
            put(out, tag, "update." + k, torch.from_numpy(sc.probe(k, (v.detach() - init).numpy())),
                torch.from_numpy(sc.probe(k, (t64[k].detach() - init.double()).numpy())))
        if ba:
            assert float((kf[0]["est_c2w"] - fr[0][0]).abs().max()) == 0.0  # the oldest frame is fixed
            put(out, tag, "c2w_update", out_c2w[:3].detach() - fr[1][0][:3],
                ref.camera_matrix(cam64).double() - fr[1][0][:3].double())
        else:
            assert out_c2w is None


def track_case(out, bound):
    import make_golden_loop as L
    sd = sc.loop_weights()
    cam = SimpleNamespace(**sc.CAM)
    fr = frame_tensors()
    m, r = ref_model(sd), ref_renderer(bound)
    tr = object.__new__(L.ref_tracker_mod.Tracker)
    tr.__dict__.update(device="cpu", H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy,
                       ignore_edge_W=sc.TRACK_EDGE, ignore_edge_H=sc.TRACK_EDGE, nice=False, bound=bound, renderer=r,
                       c={}, decoders=m, handle_dynamic=False, use_color_in_tracking=True, w_color_loss=sc.TRACK_W_COLOR)
    cam0 = L.quat_from_c2w(torch.from_numpy(sc.track_start(fr[1][0].numpy())))
    camt = cam0.clone().requires_grad_(True)
    opt = torch.optim.Adam([camt], lr=sc.TRACK_LR)
    losses = []
    with L.cpu_get_device(), L.fixed_draws(91) as fd:
        for _ in range(sc.TRACK_ITERS):
            losses.append(tr.optimize_cam_in_batch(camt, fr[1][2], fr[1][1], sc.TRACK_PIXELS, opt))
    l64, cam64 = ref.track_loop({k: v.double() for k, v in tsd(sd).items()}, bound, sc.CAM, fr[1], cam0, fd.log,
                                sc.TRACK_ITERS, sc.TRACK_LR, sc.TRACK_W_COLOR, sc.TRACK_EDGE, sc.N_SAMPLES,
                                sc.N_IMPORTANCE, torch.float64)
    tail_is_empty(lambda: ref.track_loop(tsd(sd), bound, sc.CAM, fr[1], cam0, fd.log, sc.TRACK_ITERS, sc.TRACK_LR,
                                         sc.TRACK_W_COLOR, sc.TRACK_EDGE, sc.N_SAMPLES, sc.N_IMPORTANCE))
    out["track.draws"] = torch.stack(fd.log).numpy()
    out["track.cam0"] = cam0.numpy()
    put(out, "track", "losses", torch.tensor(losses, dtype=torch.float64), torch.tensor(l64, dtype=torch.float64))
    put(out, "track", "cam_update", camt.detach() - cam0, cam64 - cam0)


def main():
    torch.set_num_threads(1)
    sd = sc.weights()
    bound = torch.from_numpy(np.asarray(sc.BOUND, dtype=np.float64))
    out = {}
    mlp_case(out, sd, bound)
    composite_case(out)
    pdf_case(out)
    render_case(out, sd, bound)
    regulation_case(out, sd, bound)
    map_case(out, bound)
    track_case(out, bound)
    paths = scenes.save_parts(os.path.join(HERE, "imap_fixtures"), out)
    print("wrote", [(os.path.basename(p), os.path.getsize(p)) for p in paths], len(out), "arrays")
    for k in sorted(out):
        if ".floor." in k or ".floor_max." in k:
            print(f"  {k:55s} {float(out[k]):.3e}")


if __name__ == "__main__":
    main()
