"""Plain-torch CPU restatement of the NICE point query with a dtype argument (test infrastructure, beside the suite
because oracle/ is frozen; the float32 oracle there restates the same formulas without one).

What it restates (reference file:line): normalize_3d_coordinate (common.py:269-284), sample_grid_feature
(conv_onet/models/decoder.py:168-175), the Fourier embedding and MLP.forward (decoder.py:177-203), MLP_no_xyz.forward
(decoder.py:262-274), NICE.forward's stage combiner (decoder.py:312-342) and Renderer.eval_points' out-of-bound
logit (Renderer.py:43-57).

dtype is the type of everything the reference computes in float32: torch.float32 reproduces it, torch.float64 gives
the value that float32 arithmetic approximates (how the fixtures' noise floors are measured).  What is part of the
model stays: the points are float64, the normalised coordinates are formed in float64 and rounded to float32
(decoder.py:171), and the points are rounded to float32 before the embedding (decoder.py:189).
"""
import torch
import torch.nn.functional as F

STAGES = ("coarse", "middle", "fine", "color")
DECODERS_OF = {"coarse": ("coarse",), "middle": ("middle",), "fine": ("middle", "fine"),
               "color": ("middle", "fine", "color")}
GRIDS_OF = {"coarse": ("grid_coarse",), "middle": ("grid_middle",), "fine": ("grid_middle", "grid_fine"),
            "color": ("grid_middle", "grid_fine", "grid_color")}


def rel_l2(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def normalize(p64, bound):
    """[P,3] float64 in [-1,1] over the bound, per axis ((p-lo)/(hi-lo))*2-1."""
    return ((p64 - bound[:, 0]) / (bound[:, 1] - bound[:, 0])) * 2 - 1.0


def grid_features(p64, grid, bound, dtype=torch.float32):
    """[P,C]: trilinear, border padding, align_corners, at the float32-rounded normalised coordinates."""
    g = normalize(p64, bound).float().to(dtype).reshape(1, -1, 1, 1, 3)
    f = F.grid_sample(grid.to(dtype), g, mode="bilinear", padding_mode="border", align_corners=True)
    return f.reshape(grid.shape[1], -1).t()


def embed(sd, pre, p64, dtype=torch.float32):
    return torch.sin(p64.float().to(dtype) @ sd[pre + "embedder._B"].to(dtype))


def _lin(sd, name, x, dtype):
    return F.linear(x, sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype))


def mlp_xyz(sd, pre, p64, feat, dtype=torch.float32, acts=None):
    """MLP.forward → [P, nout].  acts: a list that receives each layer's pre-activation."""
    emb = embed(sd, pre, p64, dtype)
    h = emb
    for i in range(5):
        a = _lin(sd, f"{pre}pts_linears.{i}", h, dtype)
        if acts is not None:
            acts.append(a.detach())
        h = F.relu(a) + _lin(sd, f"{pre}fc_c.{i}", feat, dtype)
        if i == 2:
            h = torch.cat([emb, h], -1)
    return _lin(sd, pre + "output_linear", h, dtype)


def mlp_no_xyz(sd, pre, feat, dtype=torch.float32, acts=None):
    """MLP_no_xyz.forward → [P, 1]."""
    h = feat
    for i in range(5):
        a = _lin(sd, f"{pre}pts_linears.{i}", h, dtype)
        if acts is not None:
            acts.append(a.detach())
        h = F.relu(a)
        if i == 2:
            h = torch.cat([feat, h], -1)
    return _lin(sd, pre + "output_linear", h, dtype)


def sub_decoder(sd, name, p64, grids, bound, dtype=torch.float32, acts=None):
    """One sub-decoder called directly, as NICE.forward calls them: coarse / middle / fine → [P] (the coarse one
    over the doubled bound), colour → [P,4] with its own 4th row h4 @ Wo[3] + bo[3]."""
    pre = name + "_decoder."
    if name == "coarse":
        return mlp_no_xyz(sd, pre, grid_features(p64, grids["grid_coarse"], bound * 2, dtype), dtype, acts)[:, 0]
    f = grid_features(p64, grids["grid_" + name], bound, dtype)
    if name == "fine":
        f = torch.cat([f, grid_features(p64, grids["grid_middle"], bound, dtype).detach()], 1)
    out = mlp_xyz(sd, pre, p64, f, dtype, acts)
    return out if name == "color" else out[:, 0]


def nice_raw(sd, p64, grids, stage, bound, dtype=torch.float32):
    """The stage combiner → raw [P,4]: zeros | occupancy, or rgb | fine + middle occupancy."""
    zeros = torch.zeros(p64.shape[0], 3, dtype=dtype)
    if stage == "coarse":
        return torch.cat([zeros, sub_decoder(sd, "coarse", p64, grids, bound, dtype)[:, None]], 1)
    occ = sub_decoder(sd, "middle", p64, grids, bound, dtype)
    if stage == "middle":
        return torch.cat([zeros, occ[:, None]], 1)
    occ = sub_decoder(sd, "fine", p64, grids, bound, dtype) + occ
    if stage == "fine":
        return torch.cat([zeros, occ[:, None]], 1)
    rgb = sub_decoder(sd, "color", p64, grids, bound, dtype)[:, :3]
    return torch.cat([rgb, occ[:, None]], 1)


def inside(p64, bound):
    return ((p64 > bound[:, 0]) & (p64 < bound[:, 1])).all(1)


def eval_points(sd, p64, grids, stage, bound, dtype=torch.float32):
    """Renderer.eval_points: a point not strictly inside the bound gets the occupancy logit 100 (no gradient)."""
    raw = nice_raw(sd, p64, grids, stage, bound, dtype)
    occ = torch.where(inside(p64, bound), raw[:, 3], torch.full_like(raw[:, 3], 100.0))
    return torch.cat([raw[:, :3], occ[:, None]], 1)


def vjp(sd, grids, p, cot, stage, bound, dtype=torch.float32, want_pts=True):
    """raw = eval_points(...) and the VJP of `cot` to the points, the stage's grids and the stage's decoders'
    parameters: (raw, {"pts": ..., "grid_*": ..., "<decoder>_decoder.<param>": ...}), all detached."""
    pre = tuple(d + "_decoder." for d in DECODERS_OF[stage])
    sdl = {k: (v.detach().to(dtype).clone().requires_grad_(True) if k.startswith(pre) else v) for k, v in sd.items()}
    gl = {k: (v.detach().to(dtype).clone().requires_grad_(True) if k in GRIDS_OF[stage] else v)
          for k, v in grids.items()}
    pl = p.detach().double().clone().requires_grad_(want_pts)
    raw = eval_points(sdl, pl, gl, stage, bound, dtype)
    names = (["pts"] if want_pts else []) + list(GRIDS_OF[stage]) + [k for k in sdl if k.startswith(pre)]
    tens = ([pl] if want_pts else []) + [gl[k] for k in GRIDS_OF[stage]] + [sdl[k] for k in sdl if k.startswith(pre)]
    grads = torch.autograd.grad(raw, tens, cot.to(dtype), allow_unused=True)
    out = {n: (g.detach() if g is not None else torch.zeros_like(t)) for n, t, g in zip(names, tens, grads)}
    return raw.detach(), out
