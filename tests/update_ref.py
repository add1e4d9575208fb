"""Float64 restatements of the update chain, and the seeded cases of test_update_ref_cpu.py / test_gpu_update_edges.py.

The update chain turns d loss / d pts and parameter gradients into camera and map updates: the camera gradient
(nslam_cam_grad_parts / _batch), its fused tail (nslam_cam_grad_step / _lr2: Adam on the 7-vector, the loss sum,
the best pose) and Adam (nslam_adam_step).  Nothing here imports the package: quad2rotation is restated from the
reference's formula (src/common.py:137-160), Adam is torch.optim.Adam(foreach=False) itself on CPU tensors, the
camera loop's bookkeeping is the reference's (src/Tracker.py:202-247).  Everything runs without a GPU.

Bars.  Camera gradient: |got - ref| <= 4 * 2^-24 * max|ref_part| per part (quaternion, translation): the kernel
sums in float64 and rounds once.  Adam: elementwise max-abs, 4 x the floor of the case; the floor is torch's
float32 CPU Adam against float64 Adam on the same inputs, over every segment of the case (one step call = one
case; the n_live case is the capacity's 70000 rows whatever the live count, the tail case the whole 6-iteration
trajectory).  Parameters are compared with float64 Adam at betas (0.9, 0.999); the kernel takes the betas as
float and forms 1 - beta in float32, so it is exact Adam at the float32-rounded betas, and the two moments are
compared with float64 Adam at float(np.float32(beta)), their floor being torch's float32 Adam at those same
rounded betas (in float32 1 - float32(beta) is exact, so that is the kernel's recurrence) against it.
"""
import functools

import numpy as np
import torch

K_STEPS = 6
BETAS = (0.9, 0.999)
BETAS_F32 = tuple(float(np.float32(b)) for b in BETAS)  # what the kernel's float arguments hold
EPS = 1e-8
ROW_LEN = 32
CAM_BAR = 4.0 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ camera
def quad2rotation(q):
    """src/common.py:137-160 for one quaternion (w, x, y, z), unnormalised: R = I + (2 / |q|^2) P(q)."""
    qr, qi, qj, qk = q[0], q[1], q[2], q[3]
    two_s = 2.0 / (q * q).sum()
    rows = [1 - two_s * (qj ** 2 + qk ** 2), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
            two_s * (qi * qj + qk * qr), 1 - two_s * (qi ** 2 + qk ** 2), two_s * (qj * qk - qi * qr),
            two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi ** 2 + qj ** 2)]
    return torch.stack(rows).reshape(3, 3)


def camera_pose(cam):
    """get_camera_from_tensor (src/common.py:163-176) for one 7-vector: [3, 4] in cam's dtype."""
    return torch.cat([quad2rotation(cam[:4]), cam[4:, None]], 1)


def rays_of(c2w, dirs):
    """rays_d = R . dir as get_rays_from_uv forms it (src/common.py:80-89), in c2w's dtype."""
    return (dirs.to(c2w.dtype)[:, None, :] * c2w[:3, :3]).sum(-1)


def camera_chain_autograd(cam, dirs, z, g_pts, dtype):
    """d (sum g_pts . pts) / d cam by autograd through the whole chain from the 7-vector, as
    test_cam_grad_kernel_matches_autograd writes it: pose and rays_d in `dtype`, pts = t + rays_d * z in float64.
    Returns (gradient as float64 [7], c2w [3,4] and rays_d [n,3] in dtype)."""
    camg = cam.to(dtype).clone().requires_grad_(True)
    c2w = camera_pose(camg)
    rd = rays_of(c2w, dirs)
    pts = c2w[:3, 3][None, None, :].double() + rd[:, None, :].double() * z.double()[..., None]
    (g,) = torch.autograd.grad(pts.reshape(-1, 3), camg, g_pts.double())
    return g.double(), c2w.detach(), rd.detach()


def cam_grad_ref(cam, c2w, g_pts_list, z, rays_d):
    """The camera-gradient kernels' contract on the same float32 inputs, raised to float64:
    g = sum_b g_pts[b];  g_t = sum_p g_p;  A = sum_p z_p g_p (x) rd_ray(p);  g_R = A . c2w[:3,:3];
    g_q = the VJP of quad2rotation at q = cam[:4] (float64 autograd).  Returns float64 [7]."""
    n, S = z.shape
    g = g_pts_list[0].double()
    for b in g_pts_list[1:]:
        g = g + b.double()
    g_t = g.sum(0)
    rd_p = rays_d.double().repeat_interleave(S, 0)
    A = (z.double().reshape(-1, 1) * g).T @ rd_p
    g_R = A @ c2w[:3, :3].double()
    q = cam[:4].double().clone().requires_grad_(True)
    (g_q,) = torch.autograd.grad(quad2rotation(q), q, g_R)
    return torch.cat([g_q, g_t])


def _unit(seed):
    v = torch.randn(4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return v / v.norm()


def _neg_w(q):
    return q if q[0] < 0 else -q


QUATS = {
    "tiny": 0.01 * _unit(101),                                           # |q|^2 ~ 1e-4
    "unit": torch.tensor([0.5, -0.5, 0.5, 0.5], dtype=torch.float64),    # |q|^2 == 1 exactly
    "big": 8.0 ** 0.5 * _unit(102),                                      # |q|^2 ~ 8
    "negw": 1.3 * _neg_w(_unit(103)),                                    # w < 0
}

# (n, S) of the one-camera launches: workgroups of 1024 points, at most 32, which stride beyond 32 * 1024
CAM_SHAPES = [(1, 1), (1023, 1), (1024, 1), (1025, 1), (683, 3), (64, 48), (1024, 32), (1025, 32), (700, 48)]
CAM_SEQUENCE = [(1024, 32), (1025, 1), (1023, 1), (1025, 32)]  # 32, 2, 1, 32 workgroups on one ws / ticket


def cam_buffers(n, S):
    return (1, 2, 3, 4) if (n, S) == (1025, 32) else (1, 4)


def cam_quat_of(n, S):
    return sorted(QUATS)[CAM_SHAPES.index((n, S)) % len(QUATS)]


def cam_case(n, S, nbuf, quat, seed=0):
    """One camera's inputs: cam f32 [7], dirs f32 [n,3], z f64 [n,S], g_pts nbuf x f64 [n*S,3]."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + S + 31 * nbuf)
    cam = torch.cat([QUATS[quat], torch.rand(3, generator=g, dtype=torch.float64) - 0.5]).float()
    return {"cam": cam, "dirs": torch.randn(n, 3, generator=g),
            "z": torch.rand(n, S, generator=g, dtype=torch.float64) * 3 + 0.1,
            "g_pts": [torch.randn(n * S, 3, generator=g, dtype=torch.float64) for _ in range(nbuf)]}


# (n_cams, n_per, S, nbuf, rows of a c2w entry): n_per * S = 1023, 1025, 2049 and 4 cameras at (1025, 32)
BATCH_CASES = [(1, 341, 3, 1, 3), (4, 205, 5, 2, 4), (32, 683, 3, 4, 3), (32, 341, 3, 1, 4), (4, 1025, 32, 3, 4)]
BATCH_GAP = 7


def batch_case(n_cams, n_per, S, nbuf, seed=0):
    """A bundle-adjustment batch: the cameras' slices in a permuted order with a gap of BATCH_GAP unused rays
    (NaN in g_pts, z and dirs there), a quaternion of its own norm and sign per camera."""
    g = torch.Generator().manual_seed(5000 + 100 * seed + n_cams + n_per)
    perm = torch.randperm(n_cams, generator=g).tolist()
    if n_cams > 1 and perm == sorted(perm):
        perm.reverse()
    order = perm[:1] + [-1] + perm[1:] if n_cams > 1 else [-1] + perm  # -1: the gap
    begin, r = [0] * n_cams, 0
    for k in order:
        if k < 0:
            gap0, r = r, r + BATCH_GAP
        else:
            begin[k], r = r, r + n_per
    N = r
    q = torch.randn(n_cams, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True) * torch.linspace(0.3, 2.5, n_cams, dtype=torch.float64)[:, None]
    q[1::3] = torch.where(q[1::3, :1] > 0, -q[1::3], q[1::3])  # every third camera: w < 0
    cams = torch.cat([q, torch.rand(n_cams, 3, generator=g, dtype=torch.float64) - 0.5], 1).float()
    dirs = torch.randn(N, 3, generator=g)
    z = torch.rand(N, S, generator=g, dtype=torch.float64) * 3 + 0.1
    g_pts = [torch.randn(N * S, 3, generator=g, dtype=torch.float64) for _ in range(nbuf)]
    dirs[gap0:gap0 + BATCH_GAP] = float("nan")
    z[gap0:gap0 + BATCH_GAP] = float("nan")
    for b in g_pts:
        b[gap0 * S:(gap0 + BATCH_GAP) * S] = float("nan")
    return {"cams": cams, "dirs": dirs, "z": z, "g_pts": g_pts, "ray_begin": begin, "n_per": n_per, "gap": gap0}


def batch_slice(c, k):
    """Camera k's slice of a batch (or of tensors laid out like it): (rays, points) index ranges."""
    r0, S = c["ray_begin"][k], c["z"].shape[1]
    return slice(r0, r0 + c["n_per"]), slice(r0 * S, (r0 + c["n_per"]) * S)


# ------------------------------------------------------------------------------------------------ camera tail
TAIL_SHAPES = [(21, 48), (1025, 32)]
TAIL_LOSS_LENGTHS = [0, 1, 255, 256, 257, 5000]
TAIL_MODES = {"step": (False, False), "lr_quat": (True, False), "best_before": (False, True), "lr2": (True, True)}
TAIL_LR = 0.001
TAIL_BEST0 = 1e10  # current_min_loss of Tracker.py:224
TAIL_SCALES = [1.0, 1.5, 0.5, 0.5, float("nan"), 0.75]  # improves at 0 and 2, ties at 3, NaN at 4


def tail_case(n, S, n_loss, seed=0):
    """K_STEPS iterations of synthetic inputs for the fused tail: a start camera, per-iteration d/dpts buffers
    (two) and per-ray losses scaled by TAIL_SCALES (iteration 3 repeats iteration 2's array: an exact tie;
    iteration 4 carries one NaN, in the last element)."""
    g = torch.Generator().manual_seed(9000 + 10 * seed + n)  # (the camera inputs do not depend on n_loss)
    c = cam_case(n, S, 2, "negw", seed=seed + 50)
    c["g_pts"] = [[torch.randn(n * S, 3, generator=g, dtype=torch.float64) for _ in range(2)] for _ in range(K_STEPS)]
    base = torch.rand(n_loss, generator=torch.Generator().manual_seed(9500 + n_loss), dtype=torch.float64) + 0.5
    losses = []
    for s in TAIL_SCALES:
        if s != s:
            rl = base.clone()
            rl[-1:] = float("nan")
        else:
            rl = base * s
        losses.append(rl)
    c["ray_loss"] = losses
    return c


def cam_tail_ref(cam0, g_cams, ray_losses, lr, lr_quat, best_before_step, betas=BETAS, eps=EPS, best_loss0=TAIL_BEST0,
                 dtype=torch.float64):
    """The reference's camera loop bookkeeping (Tracker.py:202-247) over len(g_cams) iterations.  Adam on the
    7-vector as two groups (elements 4..6 at lr, 0..3 at lr_quat), loss = the float64 sum of the iteration's ray
    losses, best updated when loss < best_loss, the best pose being the camera after the step, or before it for
    best_before_step.  Returns per-iteration lists: cam, exp_avg, exp_avg_sq (each [7] in dtype, after the
    step), loss, best_loss, best (None until set), and `set_at`, the iterations that set best."""
    quad = cam0[:4].to(dtype).clone().requires_grad_(True)
    T = cam0[4:].to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [T], "lr": lr}, {"params": [quad], "lr": lr_quat}], betas=betas, eps=eps,
                           foreach=False)
    out = {k: [] for k in ("cam", "exp_avg", "exp_avg_sq", "loss", "best_loss", "best")}
    out["set_at"] = []
    best_loss, best = float(best_loss0), None
    for it, (gc, rl) in enumerate(zip(g_cams, ray_losses)):
        before = torch.cat([quad, T]).detach().clone()
        loss = float(rl.double().sum())
        quad.grad, T.grad = gc[:4].to(dtype).clone(), gc[4:].to(dtype).clone()
        opt.step()
        after = torch.cat([quad, T]).detach().clone()
        if loss < best_loss:  # (NaN: not better)
            best_loss, best = loss, (before if best_before_step else after)
            out["set_at"].append(it)
        out["cam"].append(after)
        for k in ("exp_avg", "exp_avg_sq"):
            out[k].append(torch.cat([opt.state[quad][k], opt.state[T][k]]).clone())
        out["loss"].append(loss)
        out["best_loss"].append(best_loss)
        out["best"].append(best)
    return out


def tail_expect(cam0, g_cams, ray_losses, lr, lr_quat, best_before_step):
    """The tail's references and floors on the published gradients: parameters against float64 Adam at BETAS,
    moments against float64 Adam at BETAS_F32; floors = the float32 run against each, over the trajectory."""
    run = functools.partial(cam_tail_ref, cam0, g_cams, ray_losses, lr, lr_quat, best_before_step)
    p64, r64 = run(betas=BETAS), run(betas=BETAS_F32)
    p32, r32 = run(betas=BETAS, dtype=torch.float32), run(betas=BETAS_F32, dtype=torch.float32)

    def gap(a, b, key):
        return max(float((x.double() - y).abs().max()) for x, y in zip(a[key], b[key]))

    floors = {"cam": gap(p32, p64, "cam"), "exp_avg": gap(r32, r64, "exp_avg"), "exp_avg_sq": gap(r32, r64, "exp_avg_sq")}
    return p64, r64, floors


# ------------------------------------------------------------------------------------------------ Adam
def rows_view(grid):
    """[voxels, C] view of a channels-last [1, C, Z, Y, X] grid in row (voxel) order (iz*ny + iy)*nx + ix."""
    return grid.permute(0, 2, 3, 4, 1).reshape(-1, grid.shape[1])


def adam_ref(p0, grads, lr, betas=BETAS, eps=EPS, dtype=torch.float64, rows=None):
    """torch.optim.Adam(foreach=False) itself on CPU tensors in `dtype`, one step per entry of grads that is
    not None (torch skips a parameter without a gradient).  rows: the parameter is the row-masked vector of the
    channels-last grid p0 (Mapper.py:314-333: grid rows[rows], [n_rows, C]); a gradient is then grid-shaped
    (its rows are gathered) or compact [n_rows, C].  Returns (parameter, exp_avg, exp_avg_sq, steps taken)."""
    idx = rows.long() if rows is not None else None
    vec = rows_view(p0)[idx] if rows is not None else p0
    p = vec.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    steps = 0
    for g in grads:
        if g is None:
            continue
        if rows is not None and g.dim() == 5:
            g = rows_view(g)[idx]
        p.grad = g.to(dtype).reshape(p.shape).clone()
        opt.step()
        steps += 1
    st = opt.state[p] if steps else {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], steps


def _signed(shape, g, scale=1.0):
    """K_STEPS gradients whose sign is fixed per element and whose size is in scale * [0.5, 1.5): every step
    moves an element the same way, by about lr."""
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return [sign * (0.5 + torch.rand(shape, generator=g)) * scale for _ in range(K_STEPS)]


def dense_seg(name, n, lr, g, skip_odd=False, scale=1.0, p_scale=1.0):
    p0 = (torch.rand(n, generator=g) * 2 - 1) * p_scale
    grads = _signed((n,), g, scale)
    if skip_odd:
        grads = [x if i % 2 == 0 else None for i, x in enumerate(grads)]
    return {"name": name, "kind": "dense", "p0": p0, "lr": lr, "grads": grads, "rows": None}


GRID_ZYX = (7, 6, 7)  # 294 voxels


def rows_seg(name, n_rows, lr, g, compact, zyx=GRID_ZYX, all_rows=False):
    """A row-masked segment on a channels-last grid: an unsorted random subset of its voxels; the gradient
    grid-shaped (NaN outside the rows: never read) or compact [n_rows, 32]."""
    nv = zyx[0] * zyx[1] * zyx[2]
    p0 = (torch.rand(1, ROW_LEN, *zyx, generator=g) * 2 - 1).contiguous(memory_format=torch.channels_last_3d)
    rows = torch.randperm(nv, generator=g)[:nv if all_rows else n_rows].to(torch.int32)
    comp = _signed((rows.numel(), ROW_LEN), g)
    if compact:
        grads = comp
    else:
        grads = []
        for c in comp:
            d = torch.full((1, ROW_LEN, *zyx), float("nan")).contiguous(memory_format=torch.channels_last_3d)
            rows_view(d)[rows.long()] = c
            grads.append(d)
    return {"name": name, "kind": "rows", "p0": p0, "lr": lr, "grads": grads, "rows": rows, "compact": compact}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case_dense():
    g = _gen(21)
    return [dense_seg(f"n{n}", n, lr, g, skip_odd=(n == 1025))
            for n, lr in zip((1, 1023, 1024, 1025, 2049, 4099), (0.1, 0.001, 0.1, 0.001, 0.1, 0.001))]


def _case_rows(compact):
    g = _gen(22 + compact)
    return [rows_seg(f"r{n}", n, lr, g, compact) for n, lr in zip((1, 127, 128, 129, 257), (0.1, 0.001, 0.1, 0.001, 0.1))]


def _case_seg_limit(n_segs=16):
    g = _gen(24)
    segs = []
    for i in range(n_segs):
        lr = 0.1 if i % 2 == 0 else 0.001
        if i % 2 == 0:
            segs.append(dense_seg(f"d{i}", (1, 5, 1023, 1024, 1025, 2049, 33, 4099, 2)[i // 2], lr, g))
        else:
            segs.append(rows_seg(f"r{i}", (1, 127, 128, 129, 257, 3, 64, 200, 2)[i // 2], lr, g, compact=(i % 4 == 1)))
    return segs


def _case_grad_scale():
    """Gradients of 1e-12: eps dominates the denominator.  Element e: e % 7 == 0 has a zero gradient at every
    step (moments zero: it must not move), e % 7 == 3 from step 2 on (it moves on its momentum)."""
    g = _gen(25)
    s = dense_seg("tiny_grad", 2049, 0.1, g, scale=1e-12, p_scale=1e-3)
    e = torch.arange(2049)
    for i, x in enumerate(s["grads"]):
        x[e % 7 == 0] = 0.0
        if i >= 2:
            x[e % 7 == 3] = 0.0
    return [s]


def _case_zero_grad():
    g = _gen(26)
    return [dense_seg("d1025", 1025, 0.1, g), rows_seg("r129_dense", 129, 0.001, g, compact=False),
            rows_seg("r257_compact", 257, 0.1, g, compact=True)]


def _case_no_ticket():
    g = _gen(27)
    return [dense_seg("d1025", 1025, 0.1, g), dense_seg("d4099", 4099, 0.001, g, skip_odd=True),
            rows_seg("r129_compact", 129, 0.1, g, compact=True)]


def _case_mirror():
    return [dense_seg("d1025", 1025, 0.1, _gen(28))]


N_LIVE_ZYX = (40, 50, 35)
N_LIVE_CAP = 70000
# 65536 rows = exactly the 512 workgroups an n_live segment gets; 65537: workgroup 0 takes a second pass of one row
N_LIVE_COUNTS = [0, 1, 128, 129, 65536, 65537, 70000, 80000]


def _case_n_live():
    """The capacity's rows (every voxel, unsorted) with compact gradients; a live count takes a prefix."""
    return [rows_seg("cap70000", N_LIVE_CAP, 0.1, _gen(29), compact=True, zyx=N_LIVE_ZYX, all_rows=True)]


ADAM_CASES = {
    "dense": _case_dense, "rows_dense": lambda: _case_rows(False), "rows_compact": lambda: _case_rows(True),
    "seg_limit": _case_seg_limit, "grad_scale": _case_grad_scale, "zero_grad": _case_zero_grad,
    "no_ticket": _case_no_ticket, "mirror": _case_mirror, "n_live": _case_n_live,
}


@functools.lru_cache(maxsize=None)
def adam_case(name):
    return ADAM_CASES[name]()


@functools.lru_cache(maxsize=None)
def adam_expect(name):
    """Per segment of the case: the float64 references (`p` at BETAS; `exp_avg`, `exp_avg_sq` at BETAS_F32;
    `steps`), and for the case the floors {p, exp_avg, exp_avg_sq}: torch's float32 Adam against each."""
    refs, floors = [], {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for s in adam_case(name):
        run = functools.partial(adam_ref, s["p0"], s["grads"], s["lr"], eps=EPS, rows=s["rows"])
        p64, _, _, steps = run(betas=BETAS)
        _, m64, v64, _ = run(betas=BETAS_F32)
        p32, _, _, _ = run(betas=BETAS, dtype=torch.float32)
        _, m32, v32, _ = run(betas=BETAS_F32, dtype=torch.float32)
        refs.append({"p": p64, "exp_avg": m64, "exp_avg_sq": v64, "steps": steps})
        for k, a, b in (("p", p32, p64), ("exp_avg", m32, m64), ("exp_avg_sq", v32, v64)):
            floors[k] = max(floors[k], float((a.double() - b).abs().max()))
    return refs, floors


def adam_live_mask(s):
    """Elements of the segment's vector that receive a non-zero gradient at some step."""
    live = None
    for g in s["grads"]:
        if g is None:
            continue
        if s["rows"] is not None and g.dim() == 5:
            g = rows_view(g)[s["rows"].long()]
        nz = g.reshape(-1) != 0
        live = nz if live is None else live | nz
    return live


def mirror_index(n, size, seed=30):
    """[n, 2] int32 slots into a mirror of `size` floats: element e has both slots (e % 4 == 0), the first only
    (1), the second only (2) or none (3); every slot is a place of its own."""
    place = torch.randperm(size, generator=_gen(seed))[:2 * n].reshape(n, 2).to(torch.int32)
    e = torch.arange(n)
    place[(e % 4 == 1) | (e % 4 == 3), 1] = -1
    place[(e % 4 == 2) | (e % 4 == 3), 0] = -1
    return place
