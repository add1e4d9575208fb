"""The mask scene shared by tests/golden/make_golden_mesh.py (which records the reference's answers) and
tests/test_gpu_mesh.py (which replays them): inputs rebuilt from seeds, and the float64 distance of every
point to every decision threshold of Mesher.point_masks, so that points a float32 rounding could flip are
left out of the comparison.  Plain numpy.
"""
from __future__ import annotations

import numpy as np

import scenes

CAM = dict(H=24, W=32, fx=15.0, fy=15.0, cx=15.5, cy=11.5)  # the tiny camera at a quarter of its size
N_POINTS = 4096
BATCH = 1024          # the reference's chunking in the fixture: four chunks
SEED = 5
MARGIN = 1e-4         # points closer than this to any threshold are not compared
MAX_LEFT_OUT = 0.02   # at most this share of the points may be left out
MC_BOUND = [[0.1, 2.9], [-0.4, 2.1], [0.3, 2.4]]  # marching_cubes_bound of the tiny scene (inside its bound)
GRID_RES = 7


def mask_scene():
    """points float32 [4096,3] (sorted by x, so the four chunks see different parts of the images), three
    keyframe poses (float32 c2w) and their 24x32 depth images."""
    b, poses, _ = scenes.tiny_window(3)
    rng = np.random.default_rng(SEED)
    ext = b[:, 1] - b[:, 0]
    pts = ((b[:, 0] - 0.3 * ext) + rng.random((N_POINTS + 256, 3)) * (1.6 * ext)).astype(np.float32)
    # no point within 2 mm of a camera plane: uv = ./z there is the reference's NaN / inf path (unpinned)
    ok = np.ones(pts.shape[0], dtype=bool)
    for c2w in poses:
        w2c = np.linalg.inv(np.asarray(c2w, dtype=np.float64))
        ok &= np.abs(pts.astype(np.float64) @ w2c[2, :3] + w2c[2, 3]) > 2e-3
    pts = pts[ok][:N_POINTS]
    assert pts.shape[0] == N_POINTS
    pts = pts[np.argsort(pts[:, 0], kind="stable")]
    depths = [scenes.box_depth(p, CAM, b, seed=20 + k) for k, p in enumerate(poses)]
    return pts, [np.asarray(p, dtype=np.float32) for p in poses], depths


def _bilinear_zero(img, u, v):
    """grid_sample(bilinear, zeros, align_corners=True) at pixel coordinates, float64."""
    H, W = img.shape
    x0, y0 = np.floor(u), np.floor(v)
    out = np.zeros_like(u)
    for dx in (0, 1):
        for dy in (0, 1):
            x, y = x0 + dx, y0 + dy
            w = (1 - np.abs(u - x)) * (1 - np.abs(v - y))
            ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            xi = np.clip(x, 0, W - 1).astype(np.int64)
            yi = np.clip(y, 0, H - 1).astype(np.int64)
            out += np.where(ok, img[yi, xi].astype(np.float64) * w, 0.0)
    return out


def mask_margins(pts, poses, depths, depth_test, use_all, batch):
    """min over keyframes and thresholds of |value - threshold| per point (float64), and the smallest
    |z| per point.  Thresholds: the image edges (edge 0 and edge -1000), z = 0, the depth bound and, with
    depth_test, the +-2.4 window around the sampled depth."""
    H, W, fx, fy, cx, cy = (CAM[k] for k in ("H", "W", "fx", "fy", "cx", "cy"))
    p = pts.astype(np.float64)
    margin = np.full(p.shape[0], np.inf)
    zmin = np.full(p.shape[0], np.inf)
    for k, c2w in enumerate(poses):
        w2c = np.linalg.inv(c2w).astype(np.float32).astype(np.float64)
        cam = p @ w2c[:3, :3].T + w2c[:3, 3]
        X, Y, Z = -cam[:, 0], cam[:, 1], cam[:, 2]
        z = Z + 1e-8
        u, v = (fx * X + cx * Z) / z, (fy * Y + cy * Z) / z
        pd = -Z
        cand = [np.abs(z)]
        for edge in (0.0, -1000.0):
            cand += [np.abs(u - (W - edge)), np.abs(u - edge), np.abs(v - (H - edge)), np.abs(v - edge)]
        if not use_all:
            if depth_test:
                ds = _bilinear_zero(depths[k], u, v)
                for s in range(0, p.shape[0], batch):
                    md = ds[s:s + batch].max()
                    margin[s:s + batch] = np.minimum(margin[s:s + batch], np.abs(pd[s:s + batch] - md))
                cand += [np.abs(pd - (ds + 2.4)), np.abs(pd - (ds - 2.4))]
            else:
                md = float(np.float32(depths[k].max()) * np.float32(1.1))
                cand.append(np.abs(pd - md))
        margin = np.minimum(margin, np.min(np.stack(cand, 0), 0))
        zmin = np.minimum(zmin, np.abs(z))
    return margin, zmin
