"""Depth odometry on the device: frame-to-model tracking against the block-sparse TSDF volume (tsdf.TSDFVolume;
csrc/nslam_odometry.hip, the contract is in include/nslam.h).

KinectFusion's loop: the volume is ray cast from the last pose into a world-space vertex / normal map, the new
depth frame is aligned to that map by projective point-to-plane ICP, and the aligned frame is fused.  It stands in
for the open3d reconstruction system the reference's own-data path needs (scene/trajectory.log and
scene/integrated.ply for src/tools/prep_own_data.py); open3d is not a dependency, and parity with its odometry is
unpinned.  With photo_weight > 0 the alignment also compares the colour images (a photometric term
against the last tracked frame), which holds a pose that sees one textured plane only.  Poses are
camera-to-world matrices in the volume's convention (+z forward, y down),
relative to the first camera.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .tsdf import BLOCK, TSDFVolume


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """exp of the twist xi = (rotation [3], translation [3]) → float64 [4,4]."""
    xi = np.asarray(xi, dtype=np.float64)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    K = hat(w)
    if th < 1e-8:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th ** 3)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    T[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    return T


def se3_log(T):
    """The twist (rotation, translation) of a rigid transform: the inverse of se3_exp for rotations below pi."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    cos = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    th = math.acos(cos)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    w = 0.5 * axis if th < 1e-8 else (th / (2.0 * math.sin(th))) * axis
    K = hat(w)
    if th < 1e-8:
        b, c = 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        b, c = (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th ** 3)
    V = np.eye(3) + b * K + c * (K @ K)
    return np.concatenate([w, np.linalg.solve(V, T[:3, 3])])


def normal_equations(sums):
    """The 29 sums of ops.icp_sums → (A float64 [6,6], b [6], sum r^2, inlier count)."""
    s = np.asarray(sums, dtype=np.float64)
    A = np.zeros((6, 6))
    iu = np.triu_indices(6)
    A[iu] = s[:21]
    A = A + np.triu(A, 1).T
    return A, s[21:27].copy(), float(s[27]), int(round(float(s[28])))


def icp_step(sums, min_inliers, max_cond):
    """One Gauss-Newton step from the sums → (xi or None when the frame is lost, inliers, rms, cond)."""
    A, b, rr, n = normal_equations(sums)
    rms = math.sqrt(rr / n) if n > 0 else float("inf")
    if n < min_inliers or not np.isfinite(A).all():
        return None, n, rms, float("inf")
    cond = float(np.linalg.cond(A))
    if not cond <= max_cond:
        return None, n, rms, cond
    return np.linalg.solve(A, -b), n, rms, cond


def combine_sums(geo, photo, photo_weight):
    """The 29 sums of one hybrid iteration: entries 0 to 27 are geo + photo_weight * photo, entry 28 stays the
    geometric inlier count."""
    out = np.array(geo, dtype=np.float64, copy=True)
    out[:28] = out[:28] + photo_weight * np.asarray(photo, dtype=np.float64)[:28]
    return out


def predict(poses):
    """The constant-velocity prediction of the next pose from a list of poses (the last one repeated twice over)."""
    if len(poses) < 2:
        return poses[-1].copy()
    return poses[-1] @ np.linalg.inv(poses[-2]) @ poses[-1]


def write_trajectory_log(path, poses):
    """scene/trajectory.log as open3d's reconstruction system writes it and datasets.Azure.load_poses reads it: per
    frame a header line `i i i+1` and the four rows of the +z-forward camera-to-world matrix."""
    with open(path, "w") as f:
        for i, m in enumerate(poses):
            m = np.asarray(m, dtype=np.float64)
            f.write(f"{i} {i} {i + 1}\n")
            for r in range(4):
                f.write(" ".join(repr(float(x)) for x in m[r]) + "\n")


PHOTO_OFF = 1.0e300     # a photo_th that gates nothing

# The default weight of the photometric term in tools/prep_own_data.py --photometric: grey residuals are in units
# of [0, 1] per pixel against metres of the point-to-plane term.  Tuned on the synthetic 48 x 64 scenes of
# tests/rgbd_cases.py only (DESIGN.md §7k holds the sweep); no real sequence has been run.
PHOTO_WEIGHT = 1.0


class DepthOdometry(object):

    def __init__(self, H, W, fx, fy, cx, cy, voxel_length, sdf_trunc, extent, device, depth_trunc, max_jump,
                 dist_th=0.1, angle_deg=30, strides=(4, 2, 1), iters=(4, 5, 10), fuse_every=1, color=False,
                 min_inliers=50, max_cond=1.0e4, near=0.1, depth_stride=4, photo_weight=0.0, photo_th=None,
                 photo_depth_th=None):
        """An H x W pinhole camera tracked through a volume of voxel_length / sdf_trunc whose block box is the
        cube of half-edge `extent` around the first camera, fixed for the whole run.  depth_trunc, max_jump: the
        depth validity and the normal maps' discontinuity threshold; dist_th, angle_deg: the association gates;
        strides / iters: the ICP schedule, coarse to fine; a frame is fused when its index is a multiple of
        fuse_every; a frame is lost when an iteration has fewer than min_inliers inliers or a normal matrix whose
        condition number exceeds max_cond; the ray cast starts `near` in front of the camera.

        photo_weight > 0 adds the photometric term (ops.photo_sums) against the last frame that was not lost: the
        sums of every iteration are geometric + photo_weight * photometric, at the pyramid level log2(stride), so
        every stride must be a power of two and track needs the colour image.  photo_th: the residual gate in grey
        units of [0, 1] (None: off); photo_depth_th: the occlusion gate (None: dist_th).  With photo_weight = 0
        (the default) nothing of this runs."""
        if len(strides) != len(iters) or not strides:
            raise ValueError("strides and iters: one iteration count per stride expected")
        self.photo_weight = float(photo_weight)
        if not self.photo_weight >= 0.0 or not math.isfinite(self.photo_weight):
            raise ValueError("photo_weight must be finite and not negative")
        if self.photo_weight > 0 and any(int(s) < 1 or int(s) > 128 or int(s) & (int(s) - 1) for s in strides):
            raise ValueError("photo_weight > 0: every stride must be a power of two (at most 128)")
        self.photo_th = PHOTO_OFF if photo_th is None else float(photo_th)
        self.photo_depth_th = float(dist_th if photo_depth_th is None else photo_depth_th)
        if not self.photo_th >= 0.0 or not self.photo_depth_th >= 0.0:
            raise ValueError("photo_th and photo_depth_th must not be negative")
        self._ref = None      # the photometric reference: (grey pyramid, vertex map, pose) of the last tracked frame
        self._src = None      # the same of the frame being tracked
        if not float(extent) > 0:
            raise ValueError("extent must be positive")
        self.H, self.W = int(H), int(W)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.extent = float(extent)
        self.depth_trunc, self.max_jump = float(depth_trunc), float(max_jump)
        self.dist_th, self.cos_th = float(dist_th), math.cos(math.radians(float(angle_deg)))
        self.strides, self.iters = [int(s) for s in strides], [int(n) for n in iters]
        self.fuse_every = int(fuse_every)
        self.min_inliers, self.max_cond = int(min_inliers), float(max_cond)
        # a ray leaves the box after at most its diagonal
        self.near, self.far = float(near), min(float(depth_trunc), 2.0 * math.sqrt(3.0) * self.extent)
        self.device = torch.device(device)
        b = BLOCK * float(voxel_length)
        lo = int(math.floor(-self.extent / b))
        hi = int(math.floor(self.extent / b)) + 1
        self.volume = TSDFVolume(voxel_length, sdf_trunc, [lo] * 3, [hi] * 3, self.device, color=color,
                                 depth_stride=depth_stride, depth_trunc=depth_trunc)
        self.poses = []       # float64 [4,4] per tracked frame
        self.lost = []        # indices of the lost frames
        self.fused = []       # indices of the fused frames

    # ---------------------------------------------------------------------------------------------
    def _fuse(self, depth, color, c2w):
        if self.volume.with_color and color is None:
            raise ValueError("an odometry with colour needs a colour image per frame")
        col = None if not self.volume.with_color else color.to(self.device).reshape(1, self.H, self.W, 3).contiguous()
        st = self.volume.integrate(depth[None], col, c2w[None], self.fx, self.fy, self.cx, self.cy)
        if st["n_outside"] > 0:
            raise ValueError(f"{st['n_outside']} depth samples of frame {len(self.poses)} reach blocks outside the "
                             f"volume: extent = {self.extent} around the first camera is too small")
        self.fused.append(len(self.poses))

    def align(self, depth, T, gray=None):
        """ICP of a depth frame against the ray cast from the last pose, from the estimate T →
        (T, inliers, rms, lost).  One 29-double download per iteration.  With `gray` (the frame's grey pyramid) and
        a photometric reference, every iteration adds photo_weight times the photometric sums against that
        reference (a second download) and self.photo holds (photo_inliers, photo_rms) of the final pose."""
        sv, sn = ops.depth_maps(depth, self.fx, self.fy, self.cx, self.cy, self.depth_trunc, self.max_jump)
        last = self.poses[-1]
        mv, mn = self.volume.raycast(last, self.H, self.W, self.fx, self.fy, self.cx, self.cy, self.near, self.far)
        w2c = np.linalg.inv(last)

        def sums(T, stride):
            return ops.icp_sums(sv, sn, T, mv, mn, w2c, self.fx, self.fy, self.cx, self.cy, stride, self.dist_th,
                                self.cos_th).cpu().numpy()

        if gray is None:
            T = T.copy()
            for stride, n_it in zip(self.strides, self.iters):
                for _ in range(n_it):
                    xi, n, rms, _ = icp_step(sums(T, stride), self.min_inliers, self.max_cond)
                    if xi is None:
                        return T, n, rms, True
                    T = se3_exp(xi) @ T
            _, _, rr, n = normal_equations(sums(T, self.strides[-1]))
            return T, n, (math.sqrt(rr / n) if n > 0 else float("inf")), n < self.min_inliers

        self._src = (gray, sv)      # frame 0 is never lost: from frame 1 on there is a reference
        ref_gray, ref_vertex, ref_pose = self._ref
        ref_w2c = np.linalg.inv(ref_pose)

        def photo(T, stride):
            level = stride.bit_length() - 1
            return ops.photo_sums(sv, gray[level], ref_gray[level], level, ref_vertex, T, ref_w2c, self.fx, self.fy,
                                  self.cx, self.cy, self.photo_depth_th, self.photo_th).cpu().numpy()

        def rms_of(s):
            return math.sqrt(s[27] / s[28]) if s[28] > 0 else float("inf")

        T = T.copy()
        for stride, n_it in zip(self.strides, self.iters):
            for _ in range(n_it):
                geo, pho = sums(T, stride), photo(T, stride)
                xi, n, _, _ = icp_step(combine_sums(geo, pho, self.photo_weight), self.min_inliers, self.max_cond)
                if xi is None:
                    self.photo = (int(round(float(pho[28]))), rms_of(pho))
                    return T, n, rms_of(geo), True
                T = se3_exp(xi) @ T
        geo, pho = sums(T, self.strides[-1]), photo(T, self.strides[-1])
        self.photo = (int(round(float(pho[28]))), rms_of(pho))
        n = int(round(float(geo[28])))
        return T, n, rms_of(geo), n < self.min_inliers

    def track(self, depth, color=None):
        """Track one frame → dict(c2w float64 [4,4], inliers, rms, lost; with photo_weight > 0 also photo_inliers,
        photo_rms, while inliers and rms stay the geometric ones).  depth: float32 [H,W] (tensor or array, moved to
        the device); color: uint8 [H,W,3] for a volume with colour or a photometric term.

        Frame 0 gets the identity.  Later frames start from the constant-velocity prediction and run ICP against
        the ray cast from the last pose; every iteration downloads its 29 sums and solves the 6x6 system on the
        host in float64, T <- exp(xi) T: one small synchronising copy per iteration, accepted because this is an
        offline tool.  A lost frame keeps the prediction and is not fused."""
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))
        depth = depth.to(self.device, torch.float32).contiguous()
        if tuple(depth.shape) != (self.H, self.W):
            raise ValueError(f"depth: [{self.H},{self.W}] expected")
        if color is not None and not isinstance(color, torch.Tensor):
            color = torch.from_numpy(np.ascontiguousarray(color, dtype=np.uint8))
        gray = None
        if self.photo_weight > 0:
            if color is None:
                raise ValueError("an odometry with a photometric term needs a colour image per frame")
            rgb = color.to(self.device).contiguous()
            if tuple(rgb.shape) != (self.H, self.W, 3) or rgb.dtype != torch.uint8:
                raise ValueError(f"color: uint8 [{self.H},{self.W},3] expected")
            gray = ops.gray_pyramid(rgb, max(self.strides).bit_length())
        index = len(self.poses)
        self.photo = (0, 0.0)
        if index == 0:
            c2w, inliers, rms, lost = np.eye(4), 0, 0.0, False
            if gray is not None:
                self._src = (gray, ops.depth_maps(depth, self.fx, self.fy, self.cx, self.cy, self.depth_trunc,
                                                  self.max_jump)[0])
        else:
            pred = predict(self.poses)
            c2w, inliers, rms, lost = self.align(depth, pred, gray)
            if lost:
                c2w = pred
                self.lost.append(index)
        if not lost and index % self.fuse_every == 0:
            self._fuse(depth, color, c2w)
        if gray is not None and not lost:       # the tracked frame's buffers become the reference
            self._ref, self._src = (self._src[0], self._src[1], c2w.copy()), None
        self.poses.append(c2w)
        out = {"c2w": c2w.copy(), "inliers": inliers, "rms": rms, "lost": lost}
        if gray is not None:
            out["photo_inliers"], out["photo_rms"] = self.photo
        return out
