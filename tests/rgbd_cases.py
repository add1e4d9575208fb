"""Inputs and numpy twins of the odometry's photometric term (nice-slam_amd/odometry.py, csrc/nslam_odometry.hip:
nslam_gray_pyramid, nslam_photo_sums), shared by tests/test_rgbd_cpu.py and tests/test_gpu_rgbd.py.  Everything is
procedural: nothing is stored.

The contract is the one in include/nslam.h.  The grey pyramid is float32 in the contract: `gray_pyramid_f32` rounds
every operation to float32 in the stated order (numpy's elementwise float32 operations are single IEEE operations).
The photometric sums are float64 in the contract: `photo_sums_ref` is their one twin, and it returns the margin,
the pixels at which a decision lies so close to its threshold that two correct float64 evaluations may disagree.
`track_rgbd_ref` is odometry_cases.track_ref's loop with the photometric term.

Two scenes, both seen by odometry_cases' 48 x 64 camera and coloured by a smooth function of the world hit point
(sums of sinusoids with wavelengths of 0.4 m and more), so that views are photo-consistent and the texture survives
pyramid level 2:
  wall     a camera at (0.5, 1.5, 1.5) looking along -x at the plane x = -1, which is all it sees: depth alone
           leaves the normal equations singular
  corner   odometry_cases' trajectory through the room corner with the sphere
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import odometry_cases as oc
import tsdf_cases as tc

CAM = oc.CAM
N_FRAMES = oc.N_FRAMES
PIXEL_MARGIN = oc.PIXEL_MARGIN     # a projection against a rounding boundary, in pixels of the level it is used at
GATE_MARGIN = oc.GATE_MARGIN       # |dz| and |r| against their thresholds
MARGIN_CAP = 0.01                  # the margins may leave out at most this share of the pixels of a case
PHOTO_OFF = 1.0e300
SWEEP = (0.01, 0.1, 1.0, 10.0, 100.0)      # the photo_weight decades of DESIGN.md §7k


# ------------------------------------------------------------------------------------------------
# texture, scenes
# ------------------------------------------------------------------------------------------------
# (amplitude, wave vector in rad / m, phase per channel); wavelength 2 pi / |k|
_WAVES = [(0.16, np.array([0.0, 9.0, 4.0]), (0.3, 1.1, 2.3)),            # 0.64 m
          (0.14, np.array([3.0, -5.0, 11.0]), (1.7, 0.2, 4.0)),          # 0.50 m
          (0.12, np.array([7.5, 11.0, -6.5]), (2.9, 3.6, 0.8)),          # 0.42 m
          (0.10, np.array([-2.0, 2.5, 3.5]), (4.4, 5.0, 1.5))]           # 1.33 m


def texture(p):
    """Colour uint8 [..., 3] of the world points p [..., 3]: floor(255 clip(f) + 0.5), f smooth in p."""
    p = np.asarray(p, dtype=np.float64)
    out = np.empty(p.shape[:-1] + (3,), np.uint8)
    for c in range(3):
        f = 0.5 + sum(a * np.sin(p @ k + ph[c]) for a, k, ph in _WAVES)
        out[..., c] = np.floor(255.0 * np.clip(f, 0.0, 1.0) + 0.5).astype(np.uint8)
    return out


def shortest_wavelength():
    return min(2.0 * math.pi / float(np.linalg.norm(k)) for _, k, _ in _WAVES)


def wall_pose0():
    """The first wall camera: at (0.5, 1.5, 1.5), +z (forward) along world -x, x (right) along +y, y (down) along -z."""
    R = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    return tc._pose(R, np.array([0.5, 1.5, 1.5]))


def wall_twist(k):
    return np.array([0.004 * math.sin(k), 0.005, -0.008 * math.cos(k), 0.02, -0.012 * math.sin(0.7 * k), 0.004])


def trajectory(scene, n=N_FRAMES):
    if scene == "corner":
        return oc.trajectory(n)
    assert scene == "wall"
    poses = [wall_pose0()]
    for k in range(1, n):
        poses.append(poses[-1] @ oc._od().se3_exp(wall_twist(k)))
    return poses


def hit_points(depth, c2w, cam=None):
    """World points [H,W,3] of a z-depth image seen from c2w."""
    cam = cam or CAM
    H, W = depth.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.asarray(depth, dtype=np.float64)
    pc = np.stack([(u - cam["cx"]) / cam["fx"] * d, (v - cam["cy"]) / cam["fy"] * d, d], -1)
    return pc @ c2w[:3, :3].T + c2w[:3, 3]


def frames(scene, n=N_FRAMES, cam=None):
    """n frames of `scene` → SimpleNamespace(depth float32 [H,W], color uint8 [H,W,3]: the texture at the hit
    point (mid grey where a ray hits nothing), c2w: the ground truth relative to the first camera)."""
    poses = trajectory(scene, n)
    out = []
    for p, r in zip(poses, oc.relative(poses)):
        z = oc.cast(p, cam)
        color = np.where((z > 0)[..., None], texture(hit_points(z, p, cam)), np.uint8(128))
        out.append(SimpleNamespace(depth=z.astype(np.float32), color=np.ascontiguousarray(color, dtype=np.uint8),
                                   c2w=np.asarray(r, dtype=np.float64), world=p))
    return out


# ------------------------------------------------------------------------------------------------
# grey pyramid (float32)
# ------------------------------------------------------------------------------------------------
def gray_pyramid_f32(rgb, levels):
    """→ list of float32 [ceil(H / 2^l), ceil(W / 2^l)]: nslam_gray_pyramid's levels, operation for operation."""
    f = np.float32
    c = np.asarray(rgb, dtype=np.uint8).astype(f)
    out = [((f(0.299) * c[..., 0] + f(0.587) * c[..., 1]) + f(0.114) * c[..., 2]) / f(255.0)]
    for _ in range(1, levels):
        g = out[-1]
        h, w = g.shape
        x1 = 2 * np.arange((w + 1) // 2)
        y1 = 2 * np.arange((h + 1) // 2)
        x0, x2 = np.maximum(x1 - 1, 0), np.minimum(x1 + 1, w - 1)
        y0, y2 = np.maximum(y1 - 1, 0), np.minimum(y1 + 1, h - 1)
        rows = (f(0.25) * g[:, x0] + f(0.5) * g[:, x1]) + f(0.25) * g[:, x2]
        out.append((f(0.25) * rows[y0] + f(0.5) * rows[y1]) + f(0.25) * rows[y2])
        assert out[-1].dtype == f
    return out


# ------------------------------------------------------------------------------------------------
# photometric sums (float64)
# ------------------------------------------------------------------------------------------------
def photo_sums_ref(sv, sg, rg, level, rv, T, w2c, cam=None, depth_th=oc.DIST_TH, photo_th=PHOTO_OFF):
    """The 29 sums of nslam_photo_sums → SimpleNamespace(sums float64 [29], accept bool [Hs,Ws], margin bool
    [Hs,Ws], abs_sums [29]: the sums of the terms' absolute values, n_terms: the strided pixel count, r float64
    [Hs,Ws] and J [Hs,Ws,6]: the accepted pixels' residual and Jacobian row, NaN elsewhere)."""
    cam = cam or CAM
    sv, sg, rg, rv = (np.asarray(a, dtype=np.float32) for a in (sv, sg, rg, rv))
    T, M = np.asarray(T, dtype=np.float64), np.asarray(w2c, dtype=np.float64)
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    Hs, Ws = sv.shape[:2]
    Hr, Wr = rv.shape[:2]
    S = 1 << level
    scale = float(S)
    rh, rw = rg.shape
    assert sg.shape == (-(-Hs // S), -(-Ws // S)) and rg.shape == (-(-Hr // S), -(-Wr // S))
    vv, uu = np.meshgrid(np.arange(0, Hs, S), np.arange(0, Ws, S), indexing="ij")
    vv, uu = vv.reshape(-1), uu.reshape(-1)
    s = sv[vv, uu].astype(np.float64)
    isrc = sg.reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = ~np.isnan(s).any(-1)
        s = np.where(ok[:, None], s, 0.0)
        p = oc._rigid(T, s[:, 0], s[:, 1], s[:, 2])
        pc = oc._rigid(M, p[0], p[1], p[2])
        ok &= pc[2] > 0
        z = np.where(ok, pc[2], 1.0)
        x0, y0 = (pc[0] * fx) / z + cx, (pc[1] * fy) / z + cy
        xn, yn = x0 + 0.5, y0 + 0.5
        margin = ok & ((np.abs(xn - np.rint(xn)) < PIXEL_MARGIN) | (np.abs(yn - np.rint(yn)) < PIXEL_MARGIN))
        ok &= (xn >= 0) & (xn < Wr) & (yn >= 0) & (yn < Hr)
        un, vn = np.where(ok, xn, 0.0).astype(np.int64), np.where(ok, yn, 0.0).astype(np.int64)
        q = rv[vn, un].astype(np.float64)
        ok &= ~np.isnan(q).any(-1)
        dz = np.abs(z - np.where(ok, q[:, 2], 0.0))
        margin |= ok & (np.abs(dz - depth_th) < GATE_MARGIN)
        ok &= dz <= depth_th
        xl, yl = x0 / scale, y0 / scale
        fi, fj = np.floor(xl), np.floor(yl)
        margin |= ok & ((np.abs(xl - np.rint(xl)) < PIXEL_MARGIN) | (np.abs(yl - np.rint(yl)) < PIXEL_MARGIN))
        ok &= (fi >= 0) & (fi + 1.0 <= rw - 1) & (fj >= 0) & (fj + 1.0 <= rh - 1)
        i0, j0 = np.where(ok, fi, 0.0).astype(np.int64), np.where(ok, fj, 0.0).astype(np.int64)
        a, b = xl - fi, yl - fj
        i1, j1 = np.minimum(i0 + 1, rw - 1), np.minimum(j0 + 1, rh - 1)     # (clamped only where rejected)
        I00, I10 = rg[j0, i0].astype(np.float64), rg[j0, i1].astype(np.float64)
        I01, I11 = rg[j1, i0].astype(np.float64), rg[j1, i1].astype(np.float64)
        iref = (1.0 - b) * ((1.0 - a) * I00 + a * I10) + b * ((1.0 - a) * I01 + a * I11)
        gx = ((1.0 - b) * (I10 - I00) + b * (I11 - I01)) / scale
        gy = ((1.0 - a) * (I01 - I00) + a * (I11 - I10)) / scale
        r = iref - isrc
        margin |= ok & (np.abs(np.abs(r) - photo_th) < GATE_MARGIN)
        ok &= np.abs(r) <= photo_th
        zz = z * z
        gc = [gx * (fx / z), gy * (fy / z), gx * (-((fx * pc[0]) / zz)) + gy * (-((fy * pc[1]) / zz))]
        gw = [(M[0, c] * gc[0] + M[1, c] * gc[1]) + M[2, c] * gc[2] for c in range(3)]
        J = [p[1] * gw[2] - p[2] * gw[1], p[2] * gw[0] - p[0] * gw[2], p[0] * gw[1] - p[1] * gw[0],
             gw[0], gw[1], gw[2]]
        terms = [J[x] * J[y] for x in range(6) for y in range(x, 6)] + [J[x] * r for x in range(6)] + \
            [r * r, np.ones_like(r)]
    sums = np.array([t[ok].sum() for t in terms])
    abs_sums = np.array([np.abs(t[ok]).sum() for t in terms])
    accept = np.zeros((Hs, Ws), bool)
    accept[vv, uu] = ok
    mg = np.zeros((Hs, Ws), bool)
    mg[vv, uu] = margin
    r_map, J_map = np.full((Hs, Ws), np.nan), np.full((Hs, Ws, 6), np.nan)
    r_map[vv[ok], uu[ok]] = r[ok]
    J_map[vv[ok], uu[ok]] = np.stack(J, -1)[ok]
    return SimpleNamespace(sums=sums, accept=accept, margin=mg, abs_sums=abs_sums, n_terms=len(vv), r=r_map, J=J_map)


def combine(geo, photo, weight):
    """odometry.combine_sums restated: entries 0 to 27 are geo + weight * photo, the count stays geometric."""
    out = np.array(geo, dtype=np.float64, copy=True)
    out[:28] = out[:28] + weight * np.asarray(photo, dtype=np.float64)[:28]
    return out


# ------------------------------------------------------------------------------------------------
# the whole loop
# ------------------------------------------------------------------------------------------------
def track_rgbd_ref(frs, photo_weight, cam=None, extent=oc.EXTENT, strides=(4, 2, 1), iters=(4, 5, 10),
                   min_inliers=50, max_cond=1.0e4, near=oc.NEAR, depth_th=oc.DIST_TH, photo_th=PHOTO_OFF):
    """odometry_cases.track_ref's loop (float64 numpy, every tracked frame fused) with photo_weight times the
    photometric sums against the last frame that was not lost → list of dict(c2w, inliers, rms, lost, cond: the
    largest condition number met, photo_inliers, photo_rms)."""
    od = oc._od()
    cam = cam or CAM
    lo, hi = oc.box(extent)
    far = min(oc.DEPTH_TRUNC, 2.0 * math.sqrt(3.0) * extent)
    levels = max(strides).bit_length()
    poses, fused, out, ref = [], [], [], None
    for i, fr in enumerate(frs):
        src = oc.depth_maps_ref(fr.depth, cam=cam)
        sv, sn = src.vertex.astype(np.float32), src.normal.astype(np.float32)
        gray = gray_pyramid_f32(fr.color, levels) if photo_weight > 0 else None
        if i == 0:
            res = dict(c2w=np.eye(4), inliers=0, rms=0.0, lost=False, cond=0.0, photo_inliers=0, photo_rms=0.0)
        else:
            pred = od.predict(poses)
            v = oc.fuse_ref([frs[j] for j in fused], [poses[j] for j in fused], lo, hi, cam)
            model = oc.raycast_ref(oc.volume_arrays(v.table, lo, hi, v.tsdf, v.weight), poses[-1], cam=cam,
                                   near=near, far=far)
            w2c = np.linalg.inv(poses[-1])
            mv, mn = model.vertex.astype(np.float32), model.normal.astype(np.float32)

            def sums(T, stride):
                geo = oc.icp_sums_ref(sv, sn, T, mv, mn, w2c, stride, cam=cam).sums
                if gray is None:
                    return geo, np.zeros(29)
                level = stride.bit_length() - 1
                pho = photo_sums_ref(sv, gray[level], ref[0][level], level, ref[1], T, np.linalg.inv(ref[2]),
                                     cam=cam, depth_th=depth_th, photo_th=photo_th).sums
                return geo, pho

            T, lost, worst = pred.copy(), False, 0.0
            for stride, n_it in zip(strides, iters):
                for _ in range(n_it):
                    geo, pho = sums(T, stride)
                    xi, n, _, cond = od.icp_step(combine(geo, pho, photo_weight), min_inliers, max_cond)
                    worst = max(worst, cond)
                    if xi is None:
                        lost = True
                        break
                    T = od.se3_exp(xi) @ T
                if lost:
                    break
            if not lost:
                geo, pho = sums(T, strides[-1])
                n = int(round(float(geo[28])))
                lost = n < min_inliers
            res = dict(c2w=pred if lost else T, inliers=n, lost=lost, cond=worst,
                       rms=math.sqrt(geo[27] / geo[28]) if geo[28] > 0 else float("inf"),
                       photo_inliers=int(round(float(pho[28]))),
                       photo_rms=math.sqrt(pho[27] / pho[28]) if pho[28] > 0 else float("inf"))
        if not res["lost"]:
            fused.append(i)
            if gray is not None:
                ref = (gray, sv, res["c2w"])
        poses.append(res["c2w"])
        out.append(res)
    return out


def drift(res, frs):
    """(translation in metres, rotation in degrees) of the last pose against the ground truth."""
    return oc.pose_error(res[-1]["c2w"], frs[-1].c2w)
