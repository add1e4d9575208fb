"""Deterministic inputs of the iMAP* fixtures (tests/golden/make_golden_imap.py writes them, tests/test_imap_golden.py
and tests/test_gpu_imap.py rebuild them): numpy PCG64 and float64 / integer arithmetic only, so both sides get
the same arrays from a seed and the fixture stores inputs' outputs, not 0.9 MB of weights.

The scene is at room scale (a bound of a few metres), so the Fourier embedding's arguments p @ B with
B ~ 25 N(0,1) reach hundreds of radians, as in a real run.
"""
from __future__ import annotations

import numpy as np

BOUND = [[-2.5, 2.5], [-2.0, 2.0], [-1.5, 1.5]]  # every face is exactly representable in float32
N_SAMPLES, N_IMPORTANCE = 32, 12                 # configs/imap.yaml:107-109
CAM = dict(H=24, W=32, fx=20.0, fy=20.0, cx=15.5, cy=11.5)


def weights(seed=7):
    """The iMAP* module's state_dict (reference keys) as float32 arrays: DenseLayer-like uniform weights
    (xavier bound, ReLU gain), small non-zero biases, and an output layer scaled up so that sigma has both signs
    at a magnitude where alpha is neither 0 nor 1."""
    g = np.random.Generator(np.random.PCG64(seed))
    sd = {"embedder._B": (25.0 * g.standard_normal((3, 93))).astype(np.float32)}
    dims = [(256, 93), (256, 256), (256, 256), (256, 256)]
    for i, (o, k) in enumerate(dims):
        b = np.sqrt(2.0) * np.sqrt(6.0 / (o + k))
        sd[f"pts_linears.{i}.weight"] = g.uniform(-b, b, (o, k)).astype(np.float32)
        sd[f"pts_linears.{i}.bias"] = (0.05 * g.standard_normal(o)).astype(np.float32)
    b = 6.0 * np.sqrt(6.0 / (256 + 4))
    sd["output_linear.weight"] = g.uniform(-b, b, (4, 256)).astype(np.float32)
    sd["output_linear.bias"] = np.array([0.2, 0.3, 0.4, 0.5], dtype=np.float32)
    return sd


def loop_weights(seed=7):
    """weights() with sigma's bias raised to 40: every ray of the map / track cases is opaque well before its far
    end.  sample_pdf's u = 1 meets a cdf whose last entry is 1 up to rounding, so which bin the last new sample
    lands in is decided by the summation order (make_golden_imap.py); with no transmittance left there, that sample
    carries no weight and the loops do not depend on the decision."""
    sd = weights(seed)
    sd["output_linear.bias"] = np.array([0.2, 0.3, 0.4, 40.0], dtype=np.float32)
    return sd


ON_FACE = 7  # index of the point that lies exactly on the face x = 2.5


def mlp_points(n=333, seed=11):
    """[n,3] float64: uniform over the bound enlarged by 10 % (about a quarter falls outside), with one point
    exactly on a face."""
    g = np.random.Generator(np.random.PCG64(seed))
    b = np.asarray(BOUND)
    ctr, half = b.mean(1), 0.55 * (b[:, 1] - b[:, 0])
    p = ctr + half * g.uniform(-1, 1, (n, 3))
    p[ON_FACE] = [2.5, 0.3, -0.2]
    return p


def cotangent(shape, seed, dtype=np.float32):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.standard_normal(shape).astype(dtype)


def rays(n, seed, zero_frac=0.1):
    """rays_o, rays_d [n,3] float32 (directions of length 0.8 .. 1.3) from near the bound's centre, gt depth
    [n] float32 = a fraction of the distance to the bound (zero for a few)."""
    g = np.random.Generator(np.random.PCG64(seed))
    b = np.asarray(BOUND)
    o = (b.mean(1) + 0.2 * g.uniform(-1, 1, 3)).astype(np.float32)
    d = g.standard_normal((n, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.8, 1.3, (n, 1))
    d = d.astype(np.float32)
    t = (b[None, :, :] - o[None, :, None].astype(np.float64)) / d[:, :, None].astype(np.float64)
    far = t.max(2).min(1)
    gt = (far * g.uniform(0.4, 0.9, n)).astype(np.float32)
    gt[g.uniform(size=n) < zero_frac] = 0.0
    gt[0] = max(gt[0], np.float32(0.5))
    return np.broadcast_to(o, (n, 3)).copy(), d, gt


def composite_inputs(S, n=37, seed=23):
    """raw [n,S,4] float32 (sigma of both signs), ascending z [n,S] float64, rays_d [n,3] float32 (non-unit).
    Ray 0 has every sigma <= 0 (nothing composited), ray 1 a saturated first sample."""
    g = np.random.Generator(np.random.PCG64(seed + S))
    raw = g.standard_normal((n, S, 4)).astype(np.float32)
    raw[..., 3] *= 3.0
    raw[0, :, 3] = -np.abs(raw[0, :, 3])
    raw[0, 3, 3] = 0.0
    raw[1, 0, 3] = 1e4
    z = np.sort(g.uniform(0.1, 4.0, (n, S)), axis=1)
    d = g.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.8, 1.3, (n, 1))).astype(np.float32)
    return raw, z, d


def pdf_inputs(S=N_SAMPLES, n=21, seed=31):
    """Ascending coarse z [n,S] float64 and weights [n,S] float32: ordinary rays (a bump over a small floor),
    ray 0 all zero, rays 1 and 2 one-hot (0.5 and 3.0)."""
    g = np.random.Generator(np.random.PCG64(seed))
    z = np.sort(g.uniform(0.05, 3.5, (n, S)), axis=1)
    k = np.arange(S)[None, :]
    c = g.uniform(3, S - 4, (n, 1))
    w = (g.uniform(0.2, 0.9, (n, 1)) * np.exp(-0.5 * ((k - c) / g.uniform(0.7, 3.0, (n, 1))) ** 2)
         + 0.01 * g.uniform(size=(n, S))).astype(np.float32)
    w[0] = 0.0
    w[1] = 0.0
    w[1, 9] = 0.5
    w[2] = 0.0
    w[2, 20] = 3.0
    return z, w


def frames(seed=41):
    """Two 24x32 frames for the map / track cases: c2w [2,4,4] float32, depth [2,24,32] float32 (a few holes),
    colour [2,24,32,3] float32."""
    g = np.random.Generator(np.random.PCG64(seed))
    H, W = CAM["H"], CAM["W"]
    c2w = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    c2w[0, :3, 3] = [0.1, -0.1, 0.2]
    a = 0.1
    c2w[1, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=np.float32)
    c2w[1, :3, 3] = [0.15, -0.05, 0.25]
    depth = (1.0 + 0.4 * g.uniform(size=(2, H, W))).astype(np.float32)
    depth[g.uniform(size=(2, H, W)) < 0.03] = 0.0
    color = g.uniform(size=(2, H, W, 3)).astype(np.float32)
    return c2w, depth, color


MAP_ITERS, MAP_PIXELS, MAP_LR, MAP_W_COLOR, BA_CAM_LR = 3, 64, 0.0002, 0.2, 0.0002
TRACK_ITERS, TRACK_PIXELS, TRACK_LR, TRACK_W_COLOR, TRACK_EDGE = 3, 64, 0.001, 0.5, 4


def probe(name, a):
    """The part of a parameter the map case stores: everything, except every 8th row of the 256x256 matrices
    (the fixture files stay small; an update's rows are as good as each other)."""
    return a[::8] if name in ("pts_linears.1.weight", "pts_linears.2.weight", "pts_linears.3.weight") else a


def track_start(c2w):
    """The tracker's start pose: the frame's pose moved by a few centimetres."""
    s = np.array(c2w, dtype=np.float32)
    s[:3, 3] += np.array([0.03, -0.02, 0.015], dtype=np.float32)
    return s
