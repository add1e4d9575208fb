"""Deterministic inputs of the "trained-regime" fixtures (tests/golden/make_golden_trained.py writes them,
tests/test_trained_golden.py and tests/test_gpu_trained.py rebuild them): numpy PCG64 and float64 / integer
arithmetic only, so both sides get the same arrays from a seed and the fixture stores outputs, not inputs.

The regime is a pretrained decoder stack's, not the initialisation law's (oracle.init_decoders, which every other
NICE fixture uses): every pts_linears bias and every output_linear bias is non-zero (N(0, 0.3^2); the law has
them exactly zero) and the grids are N(0, 0.5^2) (the law: N(0, 0.01^2)), so each ReLU layer is about half
active and the occupancy logits span a few units.  Bound and grid lengths are the tiny scene's.
"""
from __future__ import annotations

import numpy as np

TINY_BOUND = [[0.0, 3.0], [-0.5, 2.2], [0.2, 2.5]]   # tests/golden/make_golden.py
LEN = {"coarse": 2.0, "middle": 0.64, "fine": 0.32, "color": 0.32, "bound_divisible": 0.32}
BIAS_STD, GRID_STD = 0.3, 0.5
EMB, HIDDEN, C_DIM = 93, 32, 32
DECODERS = ("coarse", "middle", "fine", "color")

M = 330                                   # 10 full 32-point tiles and one of 10
LATTICE = np.arange(40, 80)               # exactly on interior nodes of the fine grid (d/dpts has a kink there)
NEAR_FACE = np.arange(100, 120)           # in the last cell, 1e-7 .. 2e-6 of the extent below a `hi` face
OUTSIDE = np.concatenate([np.arange(280, 310), [325]])  # outside the bound on at least one axis
FACE_LO, FACE_HI, CORNER_LO, CORNER_HI = 310, 311, 312, 313  # on a face / a corner: out of bound (strict test)
OOB = np.concatenate([OUTSIDE, [FACE_LO, FACE_HI, CORNER_LO, CORNER_HI]])
NOT_LATTICE = np.setdiff1d(np.arange(M), LATTICE)  # the rows of every d/dpts comparison

N_RAYS, N_SAMPLES = 7, 48                 # 336 points: 48 does not divide 32, the rays straddle tiles


def _gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def bound():
    """[3,2] float64: NICE_SLAM.py:145-150 on the tiny bound (the upper end goes through float32)."""
    b = np.asarray(TINY_BOUND, dtype=np.float64)
    cells = ((b[:, 1] - b[:, 0]) / LEN["bound_divisible"]).astype(np.int32) + 1
    b[:, 1] = (cells.astype(np.float32) * np.float32(LEN["bound_divisible"])).astype(np.float64) + b[:, 0]
    return b


def grid_shape(name):
    """[1, C, Z, Y, X] (NICE_SLAM.py:211-248; the coarse grid covers the doubled bound)."""
    b = bound()
    ext = (b[:, 1] - b[:, 0]) * (2.0 if name == "coarse" else 1.0)
    xyz = [int(v) for v in (ext / LEN[name]).tolist()]
    return [1, C_DIM, xyz[2], xyz[1], xyz[0]]


def grids(seed=101):
    g = _gen(seed)
    return {"grid_" + k: (GRID_STD * g.standard_normal(grid_shape(k))).astype(np.float32) for k in DECODERS}


BIASED = tuple(f"{d}_decoder.{l}.bias" for d in DECODERS for l in
               [f"pts_linears.{i}" for i in range(5)] + ["output_linear"])


def decoders(seed=102):
    """The NICE state_dict (reference keys) as float32 arrays: weights by the initialisation law (xavier-uniform
    with the ReLU gain for pts_linears, gain 1 for output_linear, nn.Linear's default for fc_c, B = 25 N(0,1)),
    every pts_linears / output_linear bias N(0, BIAS_STD^2)."""
    g = _gen(seed)
    sd = {}

    def dense(name, fan_in, fan_out, gain):
        a = gain * np.sqrt(6.0 / (fan_in + fan_out))
        sd[name + ".weight"] = g.uniform(-a, a, (fan_out, fan_in)).astype(np.float32)
        sd[name + ".bias"] = (BIAS_STD * g.standard_normal(fan_out)).astype(np.float32)

    def linear(name, fan_in, fan_out):
        k = 1.0 / np.sqrt(fan_in)
        sd[name + ".weight"] = g.uniform(-k, k, (fan_out, fan_in)).astype(np.float32)
        sd[name + ".bias"] = g.uniform(-k, k, fan_out).astype(np.float32)

    for i, fin in enumerate([C_DIM, HIDDEN, HIDDEN, HIDDEN + C_DIM, HIDDEN]):
        dense(f"coarse_decoder.pts_linears.{i}", fin, HIDDEN, np.sqrt(2.0))
    dense("coarse_decoder.output_linear", HIDDEN, 1, 1.0)
    for dec, cin, nout in (("middle", C_DIM, 1), ("fine", 2 * C_DIM, 1), ("color", C_DIM, 4)):
        pre = f"{dec}_decoder."
        for i in range(5):
            linear(f"{pre}fc_c.{i}", cin, HIDDEN)
        sd[pre + "embedder._B"] = (25.0 * g.standard_normal((3, EMB))).astype(np.float32)
        for i, fin in enumerate([EMB, HIDDEN, HIDDEN, HIDDEN + EMB, HIDDEN]):
            dense(f"{pre}pts_linears.{i}", fin, HIDDEN, np.sqrt(2.0))
        dense(pre + "output_linear", HIDDEN, nout, 1.0)
    for k in BIASED:
        assert np.all(sd[k] != 0.0), k
    return sd


def points(seed=103):
    """[M,3] float64.  Uniform interior points, except the named rows."""
    g = _gen(seed)
    b = bound()
    lo, hi = b[:, 0], b[:, 1]
    ext = hi - lo
    p = lo + ext * g.uniform(0.02, 0.98, (M, 3))
    n = np.asarray(grid_shape("fine")[:1:-1], dtype=np.float64)  # nodes per axis (x, y, z)
    k = np.stack([g.integers(1, int(n[a]) - 1, LATTICE.size) for a in range(3)], 1)  # interior nodes 1 .. n-2
    p[LATTICE] = lo + ext * (k / (n - 1))
    near = g.uniform(size=(NEAR_FACE.size, 3)) < 0.5
    near[np.arange(NEAR_FACE.size), g.integers(0, 3, NEAR_FACE.size)] = True  # at least one axis each
    d = ext * g.uniform(1e-7, 2e-6, (NEAR_FACE.size, 3))
    p[NEAR_FACE] = np.where(near, hi - d, p[NEAR_FACE])
    out = lo + ext * g.uniform(-0.1, 1.1, (OUTSIDE.size, 3))
    ax, side = g.integers(0, 3, OUTSIDE.size), g.integers(0, 2, OUTSIDE.size)
    far = np.where(side == 0, lo[ax] - ext[ax] * g.uniform(0.001, 0.1, OUTSIDE.size),
                   hi[ax] + ext[ax] * g.uniform(0.001, 0.1, OUTSIDE.size))
    out[np.arange(OUTSIDE.size), ax] = far
    p[OUTSIDE] = out
    p[FACE_LO, 0] = lo[0]
    p[FACE_HI, 1] = hi[1]
    p[CORNER_LO] = lo
    p[CORNER_HI] = hi
    return p


def cotangent(stage, shape=(M, 4), seed=104):
    g = _gen(seed + 10 * DECODERS.index(stage) + shape[0])
    return g.standard_normal(shape).astype(np.float32)


def rays(seed=105):
    """rays_o, rays_d [N_RAYS,3] float32 and ascending z [N_RAYS,N_SAMPLES] float64, from near the bound's centre to
    10 % past the bound (the last samples of every ray are out of bound)."""
    g = _gen(seed)
    b = bound()
    o = (b.mean(1) + 0.2 * g.uniform(-1, 1, 3)).astype(np.float32)
    d = g.standard_normal((N_RAYS, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.8, 1.3, (N_RAYS, 1))).astype(np.float32)
    with np.errstate(divide="ignore"):
        t = (b[None, :, :] - o[None, :, None].astype(np.float64)) / d[:, :, None].astype(np.float64)
    far = t.max(2).min(1)
    z = np.sort(far[:, None] * g.uniform(0.02, 1.1, (N_RAYS, N_SAMPLES)), axis=1)
    return np.broadcast_to(o, (N_RAYS, 3)).copy(), d, z


def ray_points():
    """[N_RAYS * N_SAMPLES, 3] float64: o + d z, as the ray form of the query forms them."""
    o, d, z = rays()
    return (o.astype(np.float64)[:, None, :] + d.astype(np.float64)[:, None, :] * z[:, :, None]).reshape(-1, 3)


def permutation(seed=106):
    return _gen(seed).permutation(M)


def live_rows(name, seed=107):
    """About a third of a grid's voxels (ascending int32 rows z*Y*X + y*X + x): the live-point form's slot map."""
    n = int(np.prod(grid_shape(name)[2:]))
    return np.nonzero(_gen(seed + DECODERS.index(name)).uniform(size=n) < 1.0 / 3.0)[0].astype(np.int32)
