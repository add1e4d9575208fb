"""Plain-torch CPU restatement of the iMAP* path (test infrastructure, beside the suite because oracle/ is frozen).

What it restates (reference file:line): the iMAP* decoder (conv_onet/models/decoder.py:91-203 with c_dim=0),
Renderer.eval_points' out-of-bound rule (Renderer.py:43-57), volume-density compositing (common.py:222-245),
sample_pdf with det=True and the sort that merges its samples (common.py:19-63, Renderer.py:182-186),
render_batch_ray with N_surface=0 (Renderer.py:82-198), regulation (Renderer.py:258-296) and the mapper's and
tracker's losses (Mapper.py:487-503, Tracker.py:110-125).

dtype is the type of everything the reference computes in float32 (torch.float32 reproduces it; torch.float64
gives the value that float32 arithmetic approximates, which is how the fixtures' noise floors are measured).
What the reference computes in float64 (z, the points, depth, uncertainty) is float64 either way.  The points
are rounded to float32 before the embedding in both (decoder.py:189 is part of the model).
"""
import torch
import torch.nn.functional as F

KEYS = ("embedder._B",) + tuple(f"pts_linears.{i}.{k}" for i in range(4) for k in ("weight", "bias")) + \
    ("output_linear.weight", "output_linear.bias")


def decoder(sd, p, dtype=torch.float32):
    """raw [P,4] for p [P,3]: sin(p.float() @ B), four Linear+ReLU, a linear output."""
    h = torch.sin(p.float().to(dtype) @ sd["embedder._B"].to(dtype))
    for i in range(4):
        h = F.relu(F.linear(h, sd[f"pts_linears.{i}.weight"].to(dtype), sd[f"pts_linears.{i}.bias"].to(dtype)))
    return F.linear(h, sd["output_linear.weight"].to(dtype), sd["output_linear.bias"].to(dtype))


def eval_points(sd, p, bound, dtype=torch.float32):
    """Renderer.eval_points with nice=False: points not strictly inside the bound get sigma = 100."""
    mask = ((p[:, 0] < bound[0][1]) & (p[:, 0] > bound[0][0]) & (p[:, 1] < bound[1][1]) & (p[:, 1] > bound[1][0])
            & (p[:, 2] < bound[2][1]) & (p[:, 2] > bound[2][0]))
    raw = decoder(sd, p, dtype)
    sigma = torch.where(mask, raw[:, 3], torch.full_like(raw[:, 3], 100.0))  # (no gradient where overwritten)
    return torch.cat([raw[:, :3], sigma[:, None]], -1)


def composite_density(raw, z_vals, rays_d, dtype=torch.float32):
    """raw2outputs_nerf_color(occupancy=False) → (depth f64, var f64, rgb, weights)."""
    dists = (z_vals[..., 1:] - z_vals[..., :-1]).to(dtype)
    dists = torch.cat([dists, torch.full_like(dists[..., :1], 1e10)], -1)
    dists = dists * torch.norm(rays_d.to(dtype)[..., None, :], dim=-1)
    raw = raw.to(dtype)
    rgb = raw[..., :-1]
    alpha = 1. - torch.exp(-F.relu(raw[..., -1]) * dists)
    weights = alpha * torch.cumprod(torch.cat([torch.ones((alpha.shape[0], 1), dtype=dtype),
                                               (1. - alpha + 1e-10)], -1), -1)[:, :-1]
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z_vals, -1)
    tmp = z_vals - depth_map.unsqueeze(-1)
    depth_var = torch.sum(weights * tmp * tmp, dim=1)
    return depth_map.double(), depth_var.double(), rgb_map, weights


def sample_pdf_parts(bins, weights, n, dtype=torch.float32):
    """sample_pdf(det=True) → (samples, denom before its 1e-5 switch)."""
    weights = weights.to(dtype) + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = torch.linspace(0., 1., steps=n).to(dtype)  # (the float32 linspace's values, then widened)
    u = u.expand(list(cdf.shape[:-1]) + [n]).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    inds_g = torch.stack([below, above], -1)
    shape = [inds_g.shape[0], inds_g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, inds_g)
    denom0 = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom0 < 1e-5, torch.ones_like(denom0), denom0)
    t = (u - cdf_g[..., 0]) / denom
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0]), denom0


def sample_pdf(bins, weights, n, dtype=torch.float32):
    return sample_pdf_parts(bins, weights, n, dtype)[0]


def importance_z(z_vals, weights, n, dtype=torch.float32):
    """Renderer.py:182-186: the coarse samples merged with sample_pdf's, [N, S + n] float64."""
    mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    zs = sample_pdf(mid, weights[..., 1:-1], n, dtype).detach()
    return torch.sort(torch.cat([z_vals, zs.double()], -1), -1)[0]


def coarse_z(rays_o, rays_d, bound, gt_depth, n_samples):
    """Renderer.py:88-157 with N_surface=0, lindisp=False, perturb=0: float64 [N, n_samples]."""
    with torch.no_grad():
        t = (bound.unsqueeze(0) - rays_o.detach().unsqueeze(-1)) / rays_d.detach().unsqueeze(-1)
        far_bb = torch.min(torch.max(t, dim=2)[0], dim=1)[0].unsqueeze(-1) + 0.01
    t_vals = torch.linspace(0., 1., steps=n_samples)
    if gt_depth is None:
        near, far = 0.01, far_bb
    else:
        gt = gt_depth.reshape(-1, 1)
        near = gt.repeat(1, n_samples) * 0.01
        far = torch.clamp(far_bb, 0, torch.max(gt * 1.2))
    return (near * (1. - t_vals) + far * t_vals).double()


TAIL_MASS = None  # set to a list to record, per render_batch_ray, the largest weight of a ray's last four samples


def render_batch_ray(sd, rays_d, rays_o, bound, gt_depth, n_samples, n_importance, dtype=torch.float32,
                     want_z=False):
    """Renderer.render_batch_ray for iMAP* → (depth, uncertainty, color)."""
    n = rays_o.shape[0]
    z = coarse_z(rays_o, rays_d, bound, gt_depth, n_samples)
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
    raw = eval_points(sd, pts.reshape(-1, 3), bound, dtype).reshape(n, z.shape[1], 4)
    depth, var, color, weights = composite_density(raw, z, rays_d, dtype)
    if n_importance > 0:
        z = importance_z(z, weights.detach(), n_importance, dtype)
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
        raw = eval_points(sd, pts.reshape(-1, 3), bound, dtype).reshape(n, z.shape[1], 4)
        depth, var, color, weights = composite_density(raw, z, rays_d, dtype)
    if TAIL_MASS is not None:
        TAIL_MASS.append(float(weights[:, -4:].detach().max()))
    return (depth, var, color, z) if want_z else (depth, var, color)


def regulation(sd, rays_d, rays_o, gt_depth, bound, n_samples, t_rand, dtype=torch.float32):
    """Renderer.regulation with the recorded draws t_rand [N, n_samples] → sigma [N * n_samples]."""
    gt = gt_depth.reshape(-1, 1).repeat(1, n_samples)
    t_vals = torch.linspace(0., 1., steps=n_samples)
    z_vals = 0.0 * (1. - t_vals) + (gt * 0.85) * t_vals
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper = torch.cat([mids, z_vals[..., -1:]], -1)
    lower = torch.cat([z_vals[..., :1], mids], -1)
    z_vals = lower + (upper - lower) * t_rand
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
    return eval_points(sd, pts.reshape(-1, 3), bound, dtype)[:, -1]


def mapper_loss(depth, color, sigma, gt_depth, gt_color, w_color):
    """Mapper.py:487-503 for iMAP*: depth L1 on valid pixels + w * colour L1 + 0.0005 * |sigma|."""
    m = gt_depth > 0
    loss = torch.abs(gt_depth[m] - depth[m]).sum()
    loss = loss + w_color * torch.abs(gt_color - color).sum()
    return loss + 0.0005 * torch.abs(sigma).sum()


def tracker_loss(depth, uncertainty, color, gt_depth, gt_color, w_color, use_color=True, handle_dynamic=False):
    """Tracker.py:110-125."""
    uncertainty = uncertainty.detach()
    r = torch.abs(gt_depth - depth) / torch.sqrt(uncertainty + 1e-10)
    mask = gt_depth > 0
    if handle_dynamic:
        mask = (r < 10 * r.median()) & mask
    loss = r[mask].sum()
    if use_color:
        loss = loss + w_color * torch.abs(gt_color - color)[mask].sum()
    return loss


def rel_l2(a, b):
    """|a - b| / |b| (0 when both vanish)."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    den = float(b.norm())
    num = float((a - b).norm())
    return num / den if den > 0 else num


# ------------------------------------------------------------------------------------------------
# the mapper's and the tracker's loops for iMAP* (Mapper.py:230-540 with nice=False, Tracker.py:71-128), replayed
# with recorded pixel draws (flat indices per get_samples call) and recorded regulation jitter
# ------------------------------------------------------------------------------------------------
def camera_matrix(cam):
    """get_camera_from_tensor (common.py:137-176): (w, x, y, z, tx, ty, tz) → [3,4]."""
    qr, qi, qj, qk = cam[0], cam[1], cam[2], cam[3]
    two_s = 2.0 / (cam[:4] * cam[:4]).sum()
    R = torch.stack([1 - two_s * (qj ** 2 + qk ** 2), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                     two_s * (qi * qj + qk * qr), 1 - two_s * (qi ** 2 + qk ** 2), two_s * (qj * qk - qi * qr),
                     two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi ** 2 + qj ** 2)])
    return torch.cat([R.reshape(3, 3), cam[4:, None]], 1)


def samples(idx, H0, H1, W0, W1, cam, c2w, depth, color):
    """get_samples (common.py:92-134) for the flat pixel indices idx of the [H0:H1, W0:W1] window."""
    depth, color = depth[H0:H1, W0:W1], color[H0:H1, W0:W1]
    i, j = torch.meshgrid(torch.linspace(W0, W1 - 1, W1 - W0), torch.linspace(H0, H1 - 1, H1 - H0), indexing="ij")
    i, j = i.t().reshape(-1)[idx], j.t().reshape(-1)[idx]
    dirs = torch.stack([(i - cam["cx"]) / cam["fx"], -(j - cam["cy"]) / cam["fy"], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[:, None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, -1].expand(rays_d.shape)
    return rays_o, rays_d, depth.reshape(-1)[idx], color.reshape(-1, 3)[idx]


def map_loop(sd, bound, cam, frames, cur, draws, t_rands, n_iters, lr, w_color, n_samples, n_importance,
             ba_cam=None, ba_lr=0.0, dtype=torch.float32):
    """optimize_map for iMAP* with one keyframe (`frames[0]`, the oldest, fixed) and the current frame `cur`
    (each (c2w [4,4], depth, color)); ba_cam: the current frame's start camera tensor when BA is on.
    draws: per iteration the pixel indices of (keyframe, current); t_rands: per iteration the regulation jitter.
    sd is updated in place (leaf tensors of `dtype`).  → (losses, final camera tensor or None)."""
    params = [sd[k] for k in KEYS]
    groups = [{"params": params, "lr": lr}]
    camt = None
    if ba_cam is not None:
        camt = ba_cam.clone().requires_grad_(True)
        groups.append({"params": [camt], "lr": ba_lr})
    opt = torch.optim.Adam(groups)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=200, gamma=0.8)
    losses = []
    for it in range(n_iters):
        ro, rd, gd, gc = [], [], [], []
        for f, (c2w, depth, color) in enumerate((frames[0], cur)):
            if f == 1 and camt is not None:
                c2w = camera_matrix(camt)
            o, d, a, b = samples(draws[it][f], 0, cam["H"], 0, cam["W"], cam, c2w, depth, color)
            ro.append(o.float()), rd.append(d.float()), gd.append(a.float()), gc.append(b.float())
        ro, rd, gd, gc = torch.cat(ro), torch.cat(rd), torch.cat(gd), torch.cat(gc)
        depth, var, color = render_batch_ray(sd, rd, ro, bound, gd, n_samples, n_importance, dtype)
        sigma = regulation(sd, rd, ro, gd, bound, n_samples, t_rands[it], dtype)
        loss = mapper_loss(depth, color, sigma, gd, gc, w_color)
        opt.zero_grad()
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
        sched.step()
    return losses, (camt.detach() if camt is not None else None)


def track_loop(sd, bound, cam, frame, cam0, draws, n_iters, lr, w_color, edge, n_samples, n_importance,
               dtype=torch.float32):
    """n_iters of Tracker.optimize_cam_in_batch for iMAP* (no inside mask, handle_dynamic off) from camera
    tensor cam0 → (losses, camera tensor after the last step)."""
    camt = cam0.clone().requires_grad_(True)
    opt = torch.optim.Adam([camt], lr=lr)
    _, depth_img, color_img = frame
    losses = []
    for it in range(n_iters):
        opt.zero_grad()
        c2w = camera_matrix(camt)
        ro, rd, gd, gc = samples(draws[it], edge, cam["H"] - edge, edge, cam["W"] - edge, cam, c2w, depth_img,
                                 color_img)
        depth, var, color = render_batch_ray(sd, rd, ro, bound, gd, n_samples, n_importance, dtype)
        loss = tracker_loss(depth, var, color, gd, gc, w_color)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    return losses, camt.detach()
