#!/usr/bin/env python3
"""The iMAP* mapping iteration at the configs/imap.yaml shape (room0 bound, 5000 rays, 32 coarse + 12 importance
samples, 32 regulation samples: 540k MLP points forward and backward).

    python tools/imap_bench.py [--repeat 5] [--rays 5000] [--out profiles/imap_iter.json]

Two stages, each in a child process of its own under its own time limit (this process never opens the device):
  launches    ms per launch at the iteration's largest call (the fine pass, rays x 44 points): MLP forward (with
              the tape), the cotangent chain (nslam_imap_bwd without parameter gradients), the weight gradients
              and their reduction (the full backward minus the chain), the weight packing, the importance sampler,
              density compositing forward and backward.  The MLP's TFLOP/s count 2 (3·93 + 93·256 + 3·256² + 256·4)
              FLOP per point forward and twice that backward, against the 157.3 TF fp32 matrix peak.
  iteration   the whole iteration (coarse pass, sampler, fine pass, regulation, the loss, backward; no optimiser
              step) through Renderer on the HIP kernels, and the same iteration written with torch operators
              (hipBLASLt GEMMs and autograd) on the same device, alternated in one process.
Medians of `--repeat` windows timed with device events after a warm-up.  Synthetic scene: DenseLayer-initialised
weights, rays from the middle of the room0 bound.  A run without a HIP device fails.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM0_BOUND = [[-2.9, 8.9], [-3.2, 5.5], [-3.5, 3.3]]  # configs/Replica/room0_imap.yaml
N_SAMPLES, N_IMPORTANCE = 32, 12
FLOP_FWD = 2 * (3 * 93 + 93 * 256 + 3 * 256 * 256 + 256 * 4)
PEAK_TF = 157.3


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def median_ms(torch, fn, repeat):
    fn()
    torch.cuda.synchronize()
    return statistics.median(event_ms(torch, fn)[0] for _ in range(repeat))


def scene(torch, P, rays):
    from types import SimpleNamespace
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    bound = torch.tensor(ROOM0_BOUND, dtype=torch.float64)
    torch.manual_seed(0)
    dec = P.MLP(name="", dim=3, c_dim=0, color=True, hidden_size=256, skips=[], n_blocks=4,
                pos_embedding_method="fourier").to(dev)
    o = bound.mean(1).float() + 0.3 * (torch.rand(3, generator=g) - 0.5)
    d = torch.randn(rays, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    t = (bound[None] - o[None, :, None].double()) / d[:, :, None].double()
    far = t.max(2)[0].min(1)[0].float()
    gt = far * (0.4 + 0.5 * torch.rand(rays, generator=g))
    cfg = {"rendering": {"N_samples": N_SAMPLES, "N_surface": 0, "N_importance": N_IMPORTANCE, "lindisp": False,
                         "perturb": 0.0}, "scale": 1, "occupancy": False}
    r = P.Renderer(cfg, None, SimpleNamespace(nice=False, bound=bound, H=680, W=1200, fx=600.0, fy=600.0, cx=599.5,
                                              cy=339.5))
    return dev, bound, dec, r, o.expand(rays, 3).contiguous().to(dev), d.to(dev), gt.to(dev), \
        torch.rand(rays, 3, generator=g).to(dev)


def stage_launches(args):
    import ctypes

    import torch
    P = importlib.import_module("nice-slam_amd")
    dev, bound, dec, r, ro, rd, gt, gc = scene(torch, P, args.rays)
    L, ops, lib = P._lib.lib(), P.ops, P._lib
    S = N_SAMPLES + N_IMPORTANCE
    n = args.rays * S
    z = torch.sort(torch.rand(args.rays, S, dtype=torch.float64, device=dev) * gt[:, None].double() * 1.2, -1)[0] + 0.01
    pts = (ro[:, None, :] + rd[:, None, :] * z[..., None]).reshape(-1, 3).contiguous()
    ps = [p.detach().contiguous() for p in ops.imap_params(dec)]
    st = ops.imap_struct(ps[0], ps[1:9:2], ps[2:9:2], ps[9], ps[10])
    grads = [torch.zeros_like(p) for p in ps]
    gs = ops.imap_struct(grads[0], grads[1:9:2], grads[2:9:2], grads[9], grads[10])
    q = ops.imap_query_struct(pts, None, ops.bound_list(bound))
    packed = torch.empty(L.nslam_imap_packed_size() // 4, dtype=torch.float32, device=dev)
    raw = torch.empty(n, 4, dtype=torch.float32, device=dev)
    tape = torch.empty(L.nslam_imap_tape_size(n) // 4, dtype=torch.float32, device=dev)
    wsb = L.nslam_imap_bwd_workspace_size(n)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    g_raw = torch.randn(n, 4, device=dev)
    g_pts = torch.empty(n, 3, dtype=torch.float64, device=dev)
    sp = lib.stream_ptr(dev)

    def call(rc, what):
        lib.check(rc, what)

    fns = {
        "imap_pack": lambda: call(L.nslam_imap_pack(ctypes.byref(st), packed.data_ptr(), sp), "pack"),
        "imap_fwd": lambda: call(L.nslam_imap_fwd(ctypes.byref(st), packed.data_ptr(), ctypes.byref(q), n,
                                                  raw.data_ptr(), tape.data_ptr(), sp), "fwd"),
        "imap_chain": lambda: call(L.nslam_imap_bwd(ctypes.byref(st), packed.data_ptr(), ctypes.byref(q), n,
                                                    g_raw.data_ptr(), tape.data_ptr(), None, g_pts.data_ptr(),
                                                    ws.data_ptr(), wsb, sp), "chain"),
        "imap_bwd_full": lambda: call(L.nslam_imap_bwd(ctypes.byref(st), packed.data_ptr(), ctypes.byref(q), n,
                                                       g_raw.data_ptr(), tape.data_ptr(), ctypes.byref(gs),
                                                       g_pts.data_ptr(), ws.data_ptr(), wsb, sp), "bwd"),
    }
    out = {"points": n, "rays": args.rays, "samples": S, "ms": {}}
    for k, fn in fns.items():
        out["ms"][k] = median_ms(torch, fn, args.repeat)
    out["ms"]["imap_wgrad_and_reduce"] = out["ms"]["imap_bwd_full"] - out["ms"]["imap_chain"]
    rawr = raw.reshape(args.rays, S, 4).clone().requires_grad_(True)
    zc = z[:, :N_SAMPLES].contiguous()
    with torch.no_grad():
        w = ops.composite_density(raw.reshape(args.rays, S, 4)[:, :N_SAMPLES].contiguous(), zc, rd)[3]
    out["ms"]["sample_importance"] = median_ms(torch, lambda: ops.sample_importance(zc, w, N_IMPORTANCE), args.repeat)
    with torch.no_grad():
        out["ms"]["composite_density_fwd"] = median_ms(torch, lambda: ops.composite_density(rawr.detach(), z, rd),
                                                       args.repeat)
    res = ops.composite_density(rawr, z, rd)
    loss = res[0].sum() + res[2].sum()
    out["ms"]["composite_density_bwd"] = median_ms(
        torch, lambda: torch.autograd.grad(loss, rawr, retain_graph=True), args.repeat)
    tf = lambda flop, ms: flop / (ms * 1e-3) / 1e12  # noqa: E731
    out["mlp_tflops"] = {"fwd": tf(n * FLOP_FWD, out["ms"]["imap_fwd"]),
                         "bwd": tf(2 * n * FLOP_FWD, out["ms"]["imap_bwd_full"]),
                         "fwd_bwd": tf(3 * n * FLOP_FWD, out["ms"]["imap_fwd"] + out["ms"]["imap_bwd_full"])}
    out["mlp_fraction_of_peak"] = {k: v / PEAK_TF for k, v in out["mlp_tflops"].items()}
    out["tape_bytes"] = int(L.nslam_imap_tape_size(n))
    out["workspace_bytes"] = int(wsb)
    return out


def torch_iteration(torch, dec, bound, ro, rd, gt, gc, t_rand):
    """The iteration in torch operators (the reference's formulas, device tensors)."""
    import torch.nn.functional as F
    dev = ro.device
    b = bound.to(dev)

    def mlp(p):
        h = torch.sin(p.float() @ dec.embedder._B)
        for lin in dec.pts_linears:
            h = F.relu(F.linear(h, lin.weight, lin.bias))
        raw = F.linear(h, dec.output_linear.weight, dec.output_linear.bias)
        inside = ((p < b[:, 1]) & (p > b[:, 0])).all(1)
        return torch.cat([raw[:, :3], torch.where(inside, raw[:, 3], torch.full_like(raw[:, 3], 100.0))[:, None]], -1)

    def composite(raw, z):
        dists = (z[..., 1:] - z[..., :-1]).float()
        dists = torch.cat([dists, torch.full_like(dists[..., :1], 1e10)], -1) * torch.norm(rd[..., None, :], dim=-1)
        alpha = 1. - torch.exp(-F.relu(raw[..., -1]) * dists)
        w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
        depth = torch.sum(w * z, -1)
        return depth, torch.sum(w[..., None] * raw[..., :3], -2), w

    def render(z):
        pts = ro[..., None, :] + rd[..., None, :] * z[..., :, None]
        return composite(mlp(pts.reshape(-1, 3)).reshape(z.shape[0], z.shape[1], 4), z)

    with torch.no_grad():
        t = (b.unsqueeze(0) - ro.unsqueeze(-1)) / rd.unsqueeze(-1)
        far_bb = torch.min(torch.max(t, dim=2)[0], dim=1)[0].unsqueeze(-1) + 0.01
    tv = torch.linspace(0., 1., steps=N_SAMPLES, device=dev)
    near = gt.reshape(-1, 1).repeat(1, N_SAMPLES) * 0.01
    z = near * (1. - tv) + torch.clamp(far_bb, 0, torch.max(gt * 1.2)) * tv
    _, _, w = render(z)
    with torch.no_grad():
        mid = .5 * (z[..., 1:] + z[..., :-1])
        ww = w[..., 1:-1] + 1e-5
        cdf = torch.cumsum(ww / torch.sum(ww, -1, keepdim=True), -1)
        cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
        u = torch.linspace(0., 1., steps=N_IMPORTANCE, device=dev).expand(cdf.shape[0], N_IMPORTANCE).contiguous()
        inds = torch.searchsorted(cdf, u, right=True)
        below, above = (inds - 1).clamp_min(0), inds.clamp_max(cdf.shape[-1] - 1)
        c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
        b0, b1 = torch.gather(mid, 1, below), torch.gather(mid, 1, above)
        den = c1 - c0
        den = torch.where(den < 1e-5, torch.ones_like(den), den)
        z = torch.sort(torch.cat([z, b0 + (u - c0) / den * (b1 - b0)], -1), -1)[0]
    depth, color, _ = render(z)
    zr = gt.reshape(-1, 1).repeat(1, N_SAMPLES) * 0.85 * tv
    mids = .5 * (zr[..., 1:] + zr[..., :-1])
    upper, lower = torch.cat([mids, zr[..., -1:]], -1), torch.cat([zr[..., :1], mids], -1)
    zr = lower + (upper - lower) * t_rand
    sigma = mlp((ro[..., None, :] + rd[..., None, :] * zr[..., :, None]).reshape(-1, 3))[:, -1]
    m = gt > 0
    return torch.abs(gt[m] - depth[m]).sum() + 0.2 * torch.abs(gc - color).sum() + 0.0005 * sigma.abs().sum()


def stage_iteration(args):
    import torch
    P = importlib.import_module("nice-slam_amd")
    dev, bound, dec, r, ro, rd, gt, gc = scene(torch, P, args.rays)
    t_rand = torch.rand(args.rays, N_SAMPLES, device=dev)

    def hip():
        depth, _, color = r.render_batch_ray({}, dec, rd, ro, dev, "color", gt_depth=gt)
        sigma = r.regulation({}, dec, rd, ro, gt, dev, t_rand=t_rand)
        m = gt > 0
        loss = torch.abs(gt[m] - depth[m]).sum() + 0.2 * torch.abs(gc - color).sum() + 0.0005 * sigma.abs().sum()
        dec.zero_grad(set_to_none=True)
        loss.backward()
        return loss

    def eager():
        loss = torch_iteration(torch, dec, bound, ro, rd, gt, gc, t_rand)
        dec.zero_grad(set_to_none=True)
        loss.backward()
        return loss

    la, lb = float(hip()), float(eager())
    torch.cuda.synchronize()
    ms = {"hip": [], "torch": []}
    for _ in range(args.repeat):  # alternated windows
        ms["hip"].append(event_ms(torch, hip)[0])
        ms["torch"].append(event_ms(torch, eager)[0])
    points = args.rays * (2 * N_SAMPLES + N_SAMPLES + N_IMPORTANCE)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"rays": args.rays, "mlp_points": points, "loss_hip": la, "loss_torch": lb, "ms_per_iteration": med,
            "ms_windows": ms, "hip_over_torch": med["hip"] / med["torch"],
            "mlp_tflops_of_iteration_time": {k: 3 * points * FLOP_FWD / (v * 1e-3) / 1e12 for k, v in med.items()}}


STAGES = {"launches": (stage_launches, 240), "iteration": (stage_iteration, 300)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--rays", type=int, default=5000)
    ap.add_argument("--stage", choices=sorted(STAGES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "imap_iter.json"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    if args.stage:  # a child: one stage, its result as the last line
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/imap_bench.py needs a HIP device")
        res = STAGES[args.stage][0](args)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        return
    out = {"repeat": args.repeat, "method": "device events, one warm-up, medians; each stage in its own process "
                                            "under its own time limit"}
    for name, (_, limit) in STAGES.items():
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", name, "--repeat", str(args.repeat),
                            "--rays", str(args.rays)], capture_output=True, text=True, timeout=limit)
        if p.returncode != 0:  # nothing more is started on the device after a failed stage
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"stage {name} failed with status {p.returncode}")
        out[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
