"""Replay of a finished run as rendered frames (src/tools/viz.py, the host side of the reference's visualizer.py),
on the device, with no process, queue or window.

The reference's SLAMFrontend feeds an open3d window from a queue: a mesh, one camera actor per trajectory (a
point cloud of 12 line segments), the two trajectories as point clouds, a screenshot per refresh.  Replay keeps
the same methods and the same state and draws a frame with ONE kernel call (ops.render_scene,
csrc/nslam_raster.hip): the mesh with its vertex colours under a head light, the actors and trajectories as
depth-tested point sprites.  open3d is absent, so what the window adds of its own is restated, not pinned:
  * intrinsics: fx = fy = (H/2) / tan(fov/2), cx = W/2 - 0.5, cy = H/2 - 0.5 with fov = 60 degrees, what open3d's
    window is believed to default to (parity with the library itself is unpinned (absent));
  * shading: the project's own head-light rule (include/nslam.h), not open3d's default material and lights;
  * culling: the reference reverses every triangle and hides back faces (viz.py:95-101,160).  The package's
    mesher takes its triangles from a generated case table whose winding against skimage's has never been
    pinned, so the default is two-sided (cull="none", shading independent of the winding); cull="front" is
    the reference's rule for a mesh with skimage's winding;
  * the background is white (open3d's default, unpinned).
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import ops
from .evaluation import load_mesh
from .mesher import Mesher
from .visualizer import encode_jpeg

Z_FAR = 1000.0                       # viz.py:163-164
GT_KEY = 100000                      # viz.py:67-68
ACTOR_POINTS = np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5],
                         [0.5, 1, 1.5], [0, 1.2, 1.5]], dtype=np.float64)                     # viz.py:15-23
ACTOR_LINES = np.array([[1, 2], [2, 3], [3, 4], [4, 1], [1, 3], [2, 4], [1, 0], [0, 2], [3, 0], [0, 4], [5, 7],
                        [7, 6]])                                                              # viz.py:25-26
ACTOR_STEPS = 100                    # viz.py:31
GT_COLOR, EST_COLOR = (0, 0, 0), (255, 0, 0)       # viz.py:37, 107 ((0, 0, 0) and (1, 0, 0) as uint8)


def camera_actor(is_gt=False, scale=0.005):
    """create_camera_actor (viz.py:14-42) → (points float64 [1200,3], colour uint8 [3]): 12 segments of 100
    linspace points each in the camera's frame; black for the ground truth, red for the estimate."""
    pts = scale * ACTOR_POINTS
    t = np.linspace(0.0, 1.0, ACTOR_STEPS)
    seg = [pts[a][None, :] * (1.0 - t)[:, None] + pts[b][None, :] * t[:, None] for a, b in ACTOR_LINES]
    return np.concatenate(seg), np.array(GT_COLOR if is_gt else EST_COLOR, dtype=np.uint8)


def viewer_extrinsic(init_pose):
    """The viewer's world-to-camera matrix (viz.py:166-171): two units behind the first pose along its z column,
    columns 2 and 1 negated, inverted.  On a copy: the reference edits the caller's array."""
    p = np.array(init_pose, dtype=np.float64, copy=True)
    z = p[:3, 2]
    p[:3, 3] += 2 * (z / np.linalg.norm(z))
    p[:3, 2] *= -1
    p[:3, 1] *= -1
    return np.linalg.inv(p)


def intrinsics(H, W, fov=60.0):
    """(fx, fy, cx, cy) of a window H x W with the vertical field of view `fov` in degrees."""
    f = (H / 2.0) / np.tan(np.deg2rad(fov) / 2.0)
    return float(f), float(f), W / 2.0 - 0.5, H / 2.0 - 0.5


def _np_pose(pose):
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    return np.array(pose, dtype=np.float64, copy=True)


class Replay(object):
    """SLAMFrontend's methods (viz.py:180-209) on a renderer instead of a window.

    render() → uint8 [H, W, 3] on the device (the same buffer every frame: copy it to keep it); save(path) writes
    its JPEG.  The mesh's device buffers (vertices, faces, colours, normals: computed once per file) and the
    workspace are kept between frames; a frame's only host synchronisation is the copy for the JPEG."""

    def __init__(self, output, init_pose, cam_scale=1, near=0, estimate_c2w_list=None, gt_c2w_list=None, H=1080,
                 W=1920, fov=60.0, point_size=4, cull="none", device="cuda:0"):
        self.output = output
        self.cam_scale = cam_scale
        self.near = float(near)
        self.estimate_c2w_list = None if estimate_c2w_list is None else _np_pose(estimate_c2w_list)
        self.gt_c2w_list = None if gt_c2w_list is None else _np_pose(gt_c2w_list)
        self.H, self.W, self.fov = int(H), int(W), float(fov)
        self.point_size, self.cull = point_size, cull
        self.device = torch.device(device)
        if cull not in ops.CULL_MODES:
            raise ValueError(f"Replay: cull must be one of {sorted(ops.CULL_MODES)}, got {cull!r}")
        self.extrinsic = viewer_extrinsic(_np_pose(init_pose))
        self.cameras = {}                      # key → (is_gt, pose); viz.py:49
        self.traj = {False: None, True: None}  # gt → float64 [n,3]; viz.py:55-56
        self.mesh = None                       # (vertices, faces, colours or None, normals) on the device
        self.mesh_path = None
        self._w2c = self._ws = self._out = self._points = None

    # -- SLAMFrontend ----------------------------------------------------------------------------
    def update_pose(self, index, pose, gt=False):
        """viz.py:188-193 and :65-87: the z column flipped (on a copy: the reference flips the caller's array),
        ground truth under index + 100000, the actor placed at the pose (the reference moves it by
        pose @ inv(previous), which is the same placement)."""
        pose = _np_pose(pose)
        pose[:3, 2] *= -1
        self.cameras[index + GT_KEY if gt else index] = (bool(gt), pose)
        self._points = None

    def update_mesh(self, path):
        """viz.py:89-102: read the PLY, upload it and compute the vertex normals, once per file."""
        m = load_mesh(path)
        v = torch.from_numpy(m["vertices"]).to(self.device)
        f = torch.from_numpy(m["faces"]).to(self.device)
        c = None if m["colors"] is None else torch.from_numpy(np.ascontiguousarray(m["colors"][:, :3])).to(self.device)
        n = Mesher.vertex_normals(v, f).contiguous() if f.shape[0] else None
        self.mesh, self.mesh_path = (v, f, c, n), path

    def update_cam_trajectory(self, c2w_list, gt):
        """viz.py:104-125: the translations of list[1:i] of the ground truth or the estimate (c2w_list is i)."""
        poses = self.gt_c2w_list if gt else self.estimate_c2w_list
        if poses is None:
            raise ValueError("update_cam_trajectory: the pose list was not given to the constructor")
        self.traj[bool(gt)] = np.array(poses[1:int(c2w_list), :3, 3], dtype=np.float64, copy=True)
        self._points = None

    def reset(self):
        """viz.py:127-137: the camera actors go; the mesh and the trajectories stay."""
        self.cameras = {}
        self._points = None

    def start(self):
        return self

    def join(self):
        return None

    # -- the frame ---------------------------------------------------------------------------------
    def point_set(self):
        """(positions float64 [n,3], colours uint8 [n,3]) on the host: the live actors, then the trajectories."""
        pos, col = [], []
        for key in sorted(self.cameras):
            is_gt, pose = self.cameras[key]
            pts, c = camera_actor(is_gt, self.cam_scale)
            pos.append(pts @ pose[:3, :3].T + pose[:3, 3])
            col.append(np.broadcast_to(c, pts.shape))
        for gt in (False, True):
            if self.traj[gt] is not None and len(self.traj[gt]):
                pos.append(self.traj[gt])
                col.append(np.broadcast_to(np.array(GT_COLOR if gt else EST_COLOR, dtype=np.uint8),
                                           self.traj[gt].shape))
        if not pos:
            return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint8)
        return np.ascontiguousarray(np.concatenate(pos)), np.ascontiguousarray(np.concatenate(col))

    def render(self):
        if self._w2c is None:
            self._w2c = torch.from_numpy(np.ascontiguousarray(self.extrinsic[None, :3, :])).to(self.device)
            self._ws = ops.scene_workspace(ops.RASTER_WS_BYTES // 8, 1, self.H, self.W, self.device)
            self._out = (torch.empty(1, self.H, self.W, 3, dtype=torch.uint8, device=self.device), None, None)
        if self._points is None:
            p, c = self.point_set()
            self._points = (torch.from_numpy(p).to(self.device), torch.from_numpy(c).to(self.device))
        v, f, c, n = self.mesh if self.mesh is not None else (None, None, None, None)
        fx, fy, cx, cy = intrinsics(self.H, self.W, self.fov)
        ops.render_scene(v, f, c, n, self._points[0], self._points[1], self._w2c, self.H, self.W, fx, fy, cx, cy,
                         self.near, Z_FAR, point_size=self.point_size, cull=self.cull, ws=self._ws, out=self._out)
        return self._out[0][0]

    def save(self, path):
        """Render and write the frame's JPEG (visualizer.encode_jpeg) → its bytes."""
        data = encode_jpeg(self.render().cpu().numpy())
        with open(path, "wb") as fh:
            fh.write(data)
        return data


# ------------------------------------------------------------------------------------------------
# a video without ffmpeg: Motion-JPEG in a RIFF/AVI container
# ------------------------------------------------------------------------------------------------
def _chunk(tag, data):
    return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _list(kind, data):
    return b"LIST" + struct.pack("<I", 4 + len(data)) + kind + data


def write_mjpeg_avi(path, jpeg_bytes_list, fps, W, H):
    """An AVI 1.0 file with one MJPG video stream (every frame a JPEG as it is) and an idx1 index."""
    frames = [bytes(j) for j in jpeg_bytes_list]
    n, fps = len(frames), int(fps)
    if fps <= 0:
        raise ValueError("write_mjpeg_avi: fps must be positive")
    biggest = max([len(j) for j in frames] + [0])
    avih = struct.pack("<14I", 1000000 // fps, biggest * fps, 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, fps, 0, n, biggest, 0xffffffff, 0,
                                           0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi, index, pos = [], [], 4                     # idx1 offsets count from the 'movi' tag
    for j in frames:
        c = _chunk(b"00dc", j)
        index.append(b"00dc" + struct.pack("<III", 0x10, pos, len(j)))
        movi.append(c)
        pos += len(c)
    body = b"AVI " + hdrl + _list(b"movi", b"".join(movi)) + _chunk(b"idx1", b"".join(index))
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def read_mjpeg_avi(path):
    """The files write_mjpeg_avi writes → dict(frames = the JPEGs, fps, W, H, index = idx1's (offset, size) list);
    raises ValueError when a size does not add up."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI " or struct.unpack("<I", data[4:8])[0] != len(data) - 8:
        raise ValueError(f"{path}: not a RIFF/AVI file of its stated size")
    out = {"frames": [], "index": []}

    def walk(lo, hi):
        while lo < hi:
            tag, size = data[lo:lo + 4], struct.unpack("<I", data[lo + 4:lo + 8])[0]
            if lo + 8 + size > hi:
                raise ValueError(f"{path}: chunk {tag!r} passes its parent")
            if tag == b"LIST":
                if data[lo + 8:lo + 12] == b"movi":
                    out["movi"] = lo + 8
                walk(lo + 12, lo + 8 + size)
            elif tag == b"avih":
                f = struct.unpack("<14I", data[lo + 8:lo + 8 + 56])
                out.update(usec=f[0], n=f[4], W=f[8], H=f[9])
            elif tag == b"strh":
                out["fourcc"] = data[lo + 12:lo + 16]
                scale, rate = struct.unpack("<II", data[lo + 28:lo + 36])
                out["fps"] = rate / scale
            elif tag == b"00dc":
                out["frames"].append(data[lo + 8:lo + 8 + size])
            elif tag == b"idx1":
                for k in range(size // 16):
                    _, _, off, sz = struct.unpack("<4sIII", data[lo + 8 + 16 * k:lo + 24 + 16 * k])
                    out["index"].append((off, sz))
            lo += 8 + size + (size & 1)
        if lo != hi and lo != hi + 1:
            raise ValueError(f"{path}: sizes do not add up")

    walk(12, len(data))
    return out
