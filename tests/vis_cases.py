"""Inputs shared by tests/test_vis_cpu.py and tests/test_gpu_vis.py: images that hit every branch of the
visualiser's panel contract (include/nslam.h nslam_vis_panels).  Plain numpy."""
import numpy as np


def edge_case(H, W, seed=0):
    """gt_depth f32 [H,W], gt_color f32 [H,W,3], depth f64 [H,W], color f32 [H,W,3] with, at fixed pixels: gt
    depth 0 (residuals forced to zero, also under a rendered NaN), rendered depth equal to vmax, above vmax,
    NaN, negative, ±inf, -0.0; colours at 0, 1, k/255, just around the rounding half-steps, out of range and
    NaN; the rest random."""
    rng = np.random.default_rng(seed)
    gd = (0.5 + 3.0 * rng.random((H, W))).astype(np.float32)
    d = gd.astype(np.float64) + rng.normal(0.0, 0.4, (H, W))
    gc = rng.random((H, W, 3)).astype(np.float32)
    c = (gc + rng.normal(0.0, 0.3, (H, W, 3))).astype(np.float32)
    gd[0, 0] = 0.0
    gd[1, 2] = 0.0
    d[1, 2] = np.nan            # NaN under gt depth 0: residual panels read 0
    c[1, 2] = np.nan
    vmax = float(gd.max())
    flat = d.reshape(-1)
    flat[3] = vmax              # exactly vmax: the last colour
    flat[4] = np.nextafter(vmax, 0.0)
    flat[5] = vmax * 1.5        # above
    flat[6] = np.nan
    flat[7] = -0.25             # under
    flat[8] = np.inf
    flat[9] = -np.inf
    flat[10] = -0.0
    flat[11] = 0.0
    flat[12] = vmax / 256.0     # a table-row edge
    flat[13] = np.nextafter(vmax / 256.0, 0.0)
    cf = c.reshape(-1)
    ks = np.array([0, 1, 2, 127, 128, 254, 255], dtype=np.float32)
    vals = np.concatenate([ks / np.float32(255), (ks + np.float32(0.5)) / np.float32(255),
                           np.nextafter((ks + np.float32(0.5)) / np.float32(255), np.float32(0)),
                           np.array([0.0, 1.0, -0.0, -0.3, 1.7, np.nan, np.inf, -np.inf, 1e-9], dtype=np.float32)])
    n = min(vals.size, cf.size - 40)
    cf[40:40 + n] = vals[:n]
    gcf = gc.reshape(-1)
    gcf[40:40 + n] = vals[:n][::-1]
    return gd, gc, d, c


def zero_case(H, W, seed=1):
    """gt depth zero everywhere (vmax == 0): every depth panel is the first colour, NaN included."""
    gd, gc, d, c = edge_case(H, W, seed)
    return np.zeros_like(gd), gc, d, c


def rgb_rule(v):
    """floor(255 * clip(v, 0, 1) + 0.5) in float32, NaN as 0 — the stated rule, written independently of
    visualizer._rgb_np (scalar by scalar)."""
    out = np.empty(v.shape, dtype=np.uint8)
    for i, x in enumerate(v.reshape(-1)):
        x = np.float32(x)
        if np.isnan(x) or x <= 0:
            cl = np.float32(0)
        elif x >= 1:
            cl = np.float32(1)
        else:
            cl = x
        out.reshape(-1)[i] = int(np.floor(np.float32(np.float32(255) * cl) + np.float32(0.5)))
    return out
