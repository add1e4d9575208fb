"""Inputs and plain-numpy twins of csrc/nslam_metrics.hip: ssim_ref and errors_ref.

The twins run in float64 (the definition: the unrounded window, every step in float64) and, with dtype=np.float32,
in the kernel's stated order: the float32 window, the products x², y², xy first, per moment the horizontal pass
Σ_i g[i]·v[c+i] with i ascending from a zero sum, then the vertical pass in the same way, then the point formulas as
the kernel writes them; the means of the float32 maps are taken in float64, as the kernel's are.  Nothing here
imports the package."""
import math

import numpy as np

WIN, SIGMA = 11, 1.5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(dtype=np.float64):
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2) / (2.0 * SIGMA ** 2))
    return (g / g.sum()).astype(dtype)


def correlate_valid(a, g, axis):
    """Σ_i g[i]·a[.. + i] along axis, "valid", taps ascending from a zero sum, in a's dtype."""
    n = a.shape[axis] - (len(g) - 1)
    acc = np.zeros([n if k == axis else s for k, s in enumerate(a.shape)], dtype=a.dtype)
    for i in range(len(g)):
        idx = [slice(None)] * a.ndim
        idx[axis] = slice(i, i + n)
        acc = acc + g[i] * a[tuple(idx)]
    return acc


def filter2(a, g):
    """[h,w] → [h-10,w-10]: along x (the last axis) first, then along y."""
    return correlate_valid(correlate_valid(a, g, 1), g, 0)


def ssim_maps(x, y, L, dtype):
    """The SSIM and CS maps of two [h,w] images, every operation in dtype."""
    x, y, g = x.astype(dtype), y.astype(dtype), window(dtype)
    C1, C2 = dtype((0.01 * L) * (0.01 * L)), dtype((0.03 * L) * (0.03 * L))
    two = dtype(2)
    mx, my = filter2(x, g), filter2(y, g)
    exx, eyy, exy = filter2(x * x, g), filter2(y * y, g), filter2(x * y, g)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = exx - mxx, eyy - myy, exy - mxy
    cs = (two * sxy + C2) / ((sx + sy) + C2)
    ssim = ((two * mxy + C1) / ((mxx + myy) + C1)) * cs
    assert ssim.dtype == dtype and cs.dtype == dtype
    return ssim, cs


def pool2(a):
    """2x2 mean, stride 2, of [h,w]; an odd side is padded with one zero row / column on each side first."""
    a = np.pad(a, ((a.shape[0] % 2,) * 2, (a.shape[1] % 2,) * 2))
    h2, w2 = a.shape[0] // 2, a.shape[1] // 2
    v00, v01 = a[0:2 * h2:2, 0:2 * w2:2], a[0:2 * h2:2, 1:2 * w2:2]
    v10, v11 = a[1:2 * h2:2, 0:2 * w2:2], a[1:2 * h2:2, 1:2 * w2:2]
    return (((v00 + v01) + v10) + v11) * a.dtype.type(0.25)


def pyramid_sides(s, levels=5):
    out = [s]
    for _ in range(levels - 1):
        s = (s + 2 * (s % 2) - 2) // 2 + 1
        out.append(s)
    return out


def ssim_ref(x, y, L=1.0, levels=1, dtype=np.float64):
    """x, y [B,H,W,C] → float64 [B,levels,C,2]: the means of the SSIM and CS maps per image, level and channel."""
    x, y = np.asarray(x), np.asarray(y)
    B, H, W, C = x.shape
    out = np.zeros((B, levels, C, 2))
    for b in range(B):
        for c in range(C):
            px, py = x[b, :, :, c].astype(dtype), y[b, :, :, c].astype(dtype)
            for l in range(levels):
                if l:
                    px, py = pool2(px), pool2(py)
                s, cs = ssim_maps(px, py, L, dtype)
                out[b, l, c] = s.astype(np.float64).mean(), cs.astype(np.float64).mean()
    return out


def ms_ssim_from(means):
    """[levels=5,C,2] means → the mean over channels of Π cs_l^w_l (l < 5) · ssim_5^w_5, negatives clamped to 0."""
    v = np.concatenate([np.maximum(means[:-1, :, 1], 0.0), np.maximum(means[-1:, :, 0], 0.0)])
    return float(np.prod(v ** np.asarray(MS_WEIGHTS)[:, None], axis=0).mean())


def _sum(a):
    """The sum of a float64 array: exact (math.fsum) up to 65 536 terms; above, numpy's pairwise sum, whose error
    log2(n)·2^-53·Σ|a| is far inside the n·2^-52 the device sums are held to."""
    return math.fsum(a.ravel().tolist()) if a.size <= 1 << 16 else float(np.sum(a, dtype=np.float64))


def errors_ref(color=None, gt_color=None, depth=None, gt_depth=None, mask_mode=0, clamp=True):
    """→ float64 [B,4]: Σ(color - gt_color)², counted colour values, Σ|depth - gt_depth| over gt_depth > 0, count."""
    first = color if color is not None else gt_depth
    B = first.shape[0]
    out = np.zeros((B, 4))
    for b in range(B):
        valid = gt_depth[b] > 0 if gt_depth is not None else None
        if color is not None:
            c = np.clip(color[b], 0.0, 1.0) if clamp else color[b]
            d = c.astype(np.float64) - gt_color[b].astype(np.float64)
            if mask_mode == 1:
                d = d[valid]
            out[b, 0], out[b, 1] = _sum(d * d), d.size
        if depth is not None:
            d = np.abs(depth[b].astype(np.float64) - gt_depth[b].astype(np.float64))[valid]
            out[b, 2], out[b, 3] = _sum(d), d.size
    return out


def psnr_from(sq_sum, count):
    if count == 0:
        return float("nan")
    mse = sq_sum / count
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


# ------------------------------------------------------------------------------------------------
# images
# ------------------------------------------------------------------------------------------------
KINDS = ("noise", "ramp", "same", "negative", "const")


def _blur(a):
    """A 5-tap box blur along both image axes with edge replication (only to make a plausible second image)."""
    for axis in (0, 1):
        p = np.concatenate([np.take(a, [0, 0], axis), a, np.take(a, [-1, -1], axis)], axis)
        n = a.shape[axis]
        a = sum(np.take(p, range(i, i + n), axis) for i in range(5)) / 5.0
    return a


def image_pair(kind, H, W, C, seed=0):
    """float32 [H,W,C] x and y in [0,1] of one of KINDS."""
    rng = np.random.default_rng([seed, H, W, C, KINDS.index(kind)])
    if kind == "noise":
        x, y = rng.random((H, W, C)), rng.random((H, W, C))
    elif kind == "ramp":  # the typical regime: a smooth image with 5 % noise against a blurred copy
        yy, xx = np.mgrid[0:H, 0:W]
        base = 0.15 + 0.7 * (0.6 * xx / max(W - 1, 1) + 0.4 * yy / max(H - 1, 1))
        x = np.clip(base[:, :, None] * np.linspace(1.0, 0.8, C) + 0.05 * rng.standard_normal((H, W, C)), 0, 1)
        y = _blur(x)
    elif kind == "same":
        x = rng.random((H, W, C))
        y = x
    elif kind == "negative":
        x = rng.random((H, W, C))
        y = 1.0 - x.astype(np.float32).astype(np.float64)
    else:
        x = np.full((H, W, C), 0.25) * np.linspace(1.0, 1.5, C)
        y = np.full((H, W, C), 0.625) * np.linspace(1.0, 0.5, C)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


def image_batch(H, W, C, kinds=KINDS, seed=0):
    """float32 [len(kinds),H,W,C] x and y: one pair of every kind."""
    pairs = [image_pair(k, H, W, C, seed) for k in kinds]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def floors(x, y, L=1.0, levels=1):
    """(float64 twin [B,levels,C,2], float32 twin, the float32 floor [B,levels,2]): per image (a case: one image
    kind at one shape), level and output (SSIM mean, CS mean) the float32 twin's largest deviation from the float64
    twin over the channels."""
    r64 = ssim_ref(x, y, L, levels, np.float64)
    r32 = ssim_ref(x, y, L, levels, np.float32)
    return r64, r32, np.abs(r32 - r64).max(axis=2)


def error_case(B, H, W, C, seed=0, invalid_image=None):
    """Rendered / ground-truth colours (some outside [0,1]) and depths (about a third of the pixels invalid; image
    `invalid_image` has no valid pixel) as float32 arrays."""
    rng = np.random.default_rng([seed, B, H, W, C])
    gt_color = rng.random((B, H, W, C)).astype(np.float32)
    color = (gt_color + 0.3 * rng.standard_normal((B, H, W, C))).astype(np.float32)  # leaves [0,1] often
    gt_depth = (rng.random((B, H, W)) * 4.0 + 0.5).astype(np.float32)
    gt_depth[rng.random((B, H, W)) < 0.33] = 0.0
    if invalid_image is not None:
        gt_depth[invalid_image] = 0.0
    depth = (gt_depth + 0.05 * rng.standard_normal((B, H, W))).astype(np.float32)
    return color, gt_color, depth, gt_depth


# the shapes of the device tests: sides 11 (one output), 12, and T+9, T+10, T+11 for the kernel's tile side T (one
# tile, its edge, one output into the next tile), two non-square ones; five levels: 161 x 176 (every level of the
# odd side is padded, the last level has one output row) and 162 x 161
TILE = 32
SSIM_SHAPES = ((11, 11), (12, 12), (TILE + 9, TILE + 9), (TILE + 10, TILE + 10), (TILE + 11, TILE + 11), (11, 75),
               (75, 11))
MS_SSIM_SHAPES = ((161, 176), (162, 161))
