"""Block-sparse TSDF volume on the device (csrc/nslam_tsdf.hip; the contract is in include/nslam.h).

The volume the reference fuses in Mesher.get_bound_from_frames (src/utils/Mesher.py:214-279): open3d's
ScalableTSDFVolume algorithm restated — blocks of 16^3 voxels, a projective signed distance truncated at
sdf_trunc, a running average with weight 1 per observation, marching cubes over the voxel centres.  open3d is
not a dependency; parity with the library itself is unpinned.

Storage is a dense int32 block table over a box of block indices given at construction (the scene is bounded;
TSDFVolume.block_range measures the box a set of frames needs) and a pool of blocks that torch grows before
every integrate launch.  Pool order is (integrate call of first touch, block key): the same from run to run.
Poses are camera-to-world matrices in the +z-forward, y-down convention; opengl_to_cv converts the package's
est_c2w on a copy.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import MAX_FRAMES  # frames per touch / integrate call (one bit each)

BLOCK = 16
BLOCK_VOXELS = BLOCK ** 3
MAX_CELLS = 1 << 27      # block-table cells


def opengl_to_cv(c2w):
    """A float copy of c2w [...,4,4] (tensor or array) with its y and z axes flipped: the package's camera
    looks down -z, the volume's down +z (the reference's c2w[:3, 1] *= -1; c2w[:3, 2] *= -1).  Keeps the dtype."""
    if isinstance(c2w, torch.Tensor):
        c2w = c2w.detach().cpu().numpy()
    out = np.array(c2w, copy=True)
    out[..., :3, 1] *= -1.0
    out[..., :3, 2] *= -1.0
    return out


def _poses(c2w):
    """c2w [K,4,4] (tensor or array, any float dtype) → (c2w float64 [K,4,4], w2c float32 [K,4,4]) numpy; the
    inverse is taken on the host in the pose's own dtype, as the reference does."""
    if isinstance(c2w, torch.Tensor):
        c2w = c2w.detach().cpu().numpy()
    c2w = np.asarray(c2w)
    if c2w.ndim != 3 or c2w.shape[1:] != (4, 4):
        raise ValueError("c2w: [K,4,4] expected")
    if c2w.dtype not in (np.float32, np.float64):
        c2w = c2w.astype(np.float64)
    w2c = np.stack([np.linalg.inv(m) for m in c2w], 0).astype(np.float32) if len(c2w) else \
        np.zeros((0, 4, 4), np.float32)
    return np.ascontiguousarray(c2w.astype(np.float64)), np.ascontiguousarray(w2c)


def _check_box(lo, hi):
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("block_lo and block_hi hold three block indices each")
    dims = [h - l for l, h in zip(lo, hi)]
    if min(dims) <= 0:
        raise ValueError(f"the block range [{lo}, {hi}) is empty")
    if dims[0] * dims[1] * dims[2] > MAX_CELLS or max(abs(v) for v in lo + hi) > 1 << 26:
        raise ValueError(f"the block range [{lo}, {hi}) needs a table of {dims[0] * dims[1] * dims[2]} cells, more "
                         f"than 2^27: an outlier depth is the usual cause (lower depth_trunc or clip the range)")
    return lo, hi, dims


class TSDFVolume(object):

    def __init__(self, voxel_length, sdf_trunc, block_lo, block_hi, device, color=True, depth_stride=4,
                 depth_trunc=1000.0):
        """voxel_length, sdf_trunc: world units, 2 sdf_trunc <= 16 voxel_length (a sample then touches at most
        two blocks per axis).  block_lo / block_hi: the table's box of block indices [lo, hi) per axis, a block
        being 16 voxels wide and anchored at the world origin.  color: keep a float32 RGB per voxel."""
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        if not self.voxel_length > 0 or not self.sdf_trunc > 0:
            raise ValueError("voxel_length and sdf_trunc must be positive")
        if 2.0 * self.sdf_trunc > BLOCK * self.voxel_length:
            raise ValueError("sdf_trunc may be at most 8 voxel_length (half a block)")
        if int(depth_stride) < 1 or not float(depth_trunc) > 0:
            raise ValueError("depth_stride >= 1 and depth_trunc > 0 expected")
        self.block_lo, self.block_hi, self.dims = _check_box(block_lo, block_hi)
        self.device = torch.device(device)
        self.depth_stride, self.depth_trunc = int(depth_stride), float(depth_trunc)
        self.with_color = bool(color)
        self.n_blocks = 0
        self.table = torch.full((self.dims[0] * self.dims[1] * self.dims[2],), -1, dtype=torch.int32,
                                device=self.device)
        self._key = torch.empty(0, dtype=torch.int32, device=self.device)
        self._tsdf = torch.empty(0, BLOCK_VOXELS, dtype=torch.float32, device=self.device)
        self._weight = torch.empty(0, BLOCK_VOXELS, dtype=torch.float32, device=self.device)
        self._color = torch.empty(3, 0, BLOCK_VOXELS, dtype=torch.float32, device=self.device) if color else None

    # ---------------------------------------------------------------------------------------------
    @staticmethod
    def block_range(depth, c2w, H, W, fx, fy, cx, cy, voxel_length, sdf_trunc, depth_stride=4, depth_trunc=1000.0):
        """The box of blocks that the strided samples of the frames reach (nslam_tsdf_block_range) →
        (block_lo, block_hi, n_valid): lists of three ints, hi exclusive, and the number of valid samples;
        (None, None, 0) when no sample is valid.  depth: device float32 [K,H,W]; c2w [K,4,4], +z forward."""
        c2w64, _ = _poses(c2w)
        if c2w64.shape[0] != depth.shape[0]:
            raise ValueError("one pose per depth image expected")
        if depth.shape[0] == 0:
            return None, None, 0
        c2w_d = torch.from_numpy(c2w64).to(depth.device)
        bounds, n_valid = ops.tsdf_block_range(depth, c2w_d, H, W, fx, fy, cx, cy, depth_stride, depth_trunc,
                                               voxel_length, sdf_trunc)
        n = int(n_valid)
        if n == 0:
            return None, None, 0
        b = bounds.cpu().tolist()
        return b[:3], [v + 1 for v in b[3:]], n

    # ---------------------------------------------------------------------------------------------
    def _reserve(self, n):
        cap = self._tsdf.shape[0]
        if n <= cap:
            return
        new = max(n, cap + cap // 2)
        tsdf = torch.zeros(new, BLOCK_VOXELS, dtype=torch.float32, device=self.device)
        weight = torch.zeros(new, BLOCK_VOXELS, dtype=torch.float32, device=self.device)
        tsdf[:cap], weight[:cap] = self._tsdf, self._weight
        self._tsdf, self._weight = tsdf, weight
        if self.with_color:
            color = torch.zeros(3, new, BLOCK_VOXELS, dtype=torch.float32, device=self.device)
            color[:, :cap] = self._color
            self._color = color

    def integrate(self, depth, color, c2w, fx, fy, cx, cy):
        """Fuse K frames.  depth: device float32 [K,H,W]; color: device uint8 [K,H,W,3] (None for a volume
        without colour); c2w [K,4,4] (+z forward; tensor or array, inverted on the host in its own dtype).
        More than 32 frames are fused in calls of 32.  Returns {n_new_blocks, n_outside}: the blocks allocated,
        and the valid samples that reach a block outside the table (those blocks are not fused)."""
        if depth.dim() != 3:
            raise ValueError("depth: [K,H,W] expected")
        K, H, W = (int(v) for v in depth.shape)
        c2w64, w2c32 = _poses(c2w)
        if c2w64.shape[0] != K:
            raise ValueError("one pose per depth image expected")
        if self.with_color and color is None:
            raise ValueError("a volume with colour needs colour images")
        if not self.with_color:
            color = None
        c2w_d = torch.from_numpy(c2w64).to(self.device)
        w2c_d = torch.from_numpy(w2c32).to(self.device)
        n_new = n_out = 0
        for s in range(0, K, MAX_FRAMES):
            e = min(K, s + MAX_FRAMES)
            d = depth[s:e].contiguous()
            mask, outside = ops.tsdf_touch(d, c2w_d[s:e].contiguous(), H, W, fx, fy, cx, cy, self.depth_stride,
                                           self.depth_trunc, self.voxel_length, self.sdf_trunc, self.block_lo,
                                           self.block_hi)
            keys = torch.nonzero(mask).reshape(-1)          # ascending: block-key order
            fresh = keys[self.table[keys] < 0]
            k_new = int(fresh.shape[0])
            if k_new:
                self.table[fresh] = torch.arange(self.n_blocks, self.n_blocks + k_new, dtype=torch.int32,
                                                 device=self.device)
                self._key = torch.cat([self._key, fresh.to(torch.int32)])
                self._reserve(self.n_blocks + k_new)
                self.n_blocks += k_new
            n_new += k_new
            n_out += int(outside)
            if keys.shape[0]:
                ops.tsdf_integrate(d, None if color is None else color[s:e].contiguous(), w2c_d[s:e].contiguous(),
                                   H, W, fx, fy, cx, cy, self.depth_trunc, self.voxel_length, self.sdf_trunc,
                                   self.block_lo, self.block_hi, keys.to(torch.int32), self.table[keys].contiguous(),
                                   mask[keys].contiguous(), self.n_blocks, self._tsdf, self._weight, self._color)
        return {"n_new_blocks": n_new, "n_outside": n_out}

    def extract_mesh(self):
        """Marching cubes over the allocated blocks → dict of device tensors: vertices float64 [V,3], faces
        int32 [F,3] (right-hand normals toward the free side), colors uint8 [V,3] (None without colour)."""
        v, f, c = ops.tsdf_marching_cubes(self._tsdf, self._weight, self._color, self._key, self.n_blocks,
                                          self.table, self.block_lo, self.block_hi, self.voxel_length)
        return {"vertices": v, "faces": f, "colors": c}

    def raycast(self, c2w, H, W, fx, fy, cx, cy, near, far):
        """The volume seen from the pose c2w [4,4] (+z forward; tensor or array) by an H x W pinhole camera
        (nslam_tsdf_raycast) → (vertex, normal) device float32 [H,W,3] in the world frame: the zero crossing of
        every pixel's ray between the distances near and far along it, and the TSDF's gradient direction there
        (toward the free side).  NaN where a ray hits nothing."""
        if isinstance(c2w, torch.Tensor):
            c2w = c2w.detach().cpu().numpy()
        c2w = np.asarray(c2w, dtype=np.float64)
        if c2w.shape != (4, 4):
            raise ValueError("c2w: [4,4] expected")
        return ops.tsdf_raycast(self.table, self._key, self._tsdf, self._weight, self.n_blocks, self.block_lo,
                                self.block_hi, self.voxel_length, self.sdf_trunc, c2w, H, W, fx, fy, cx, cy, near, far)

    # the pool's live part (views): [n_blocks,4096] (x * 16 + y) * 16 + z within a block; colour [3,n_blocks,4096]
    @property
    def tsdf(self):
        return self._tsdf[:self.n_blocks]

    @property
    def weight(self):
        return self._weight[:self.n_blocks]

    @property
    def color(self):
        return None if self._color is None else self._color[:, :self.n_blocks]

    @property
    def block_keys(self):
        """int32 [n_blocks]: the table cell of every pool block, ((bx - lo.x) * ny + (by - lo.y)) * nz + bz - lo.z."""
        return self._key

    def block_coords(self):
        """int64 [n_blocks,3]: the block indices of the pool, in pool order."""
        k = self._key.long()
        ny, nz = self.dims[1], self.dims[2]
        lo = torch.tensor(self.block_lo, device=self.device)
        return torch.stack([k // (ny * nz), (k // nz) % ny, k % nz], 1) + lo
