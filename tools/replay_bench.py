#!/usr/bin/env python3
"""One replayed frame (visualizer.py) at Replica room0 size: ms per stage.

    python tools/replay_bench.py [--resolution 256] [--repeat 5] [--out profiles/replay_frame.json]

Workload: the mesh tools/mesh_bench.py extracts (its analytic room volume at `--resolution`^3, seeded vertex colours),
written to a PLY and read back as visualizer.py reads it, seen at 1920 x 1080 from replay.viewer_extrinsic of a pose
inside the room, with two camera actors and 2 x 2000 trajectory points.  Stages of nslam_scene_render, each its own
launch, timed with device events (the five passes run in order per repetition; medians of `--repeat` after a
warm-up frame):
  clear, faces_inline (the per-(face, view) pass with its inline boxes), faces_list (the listed boxes), points, resolve
then the device-to-host copy of the frame (device events), the Pillow JPEG encode and the whole Replay.save (host
clock, the device idle before and after), and once: the PLY load + upload + vertex normals.
No target is fixed in advance: there is no reference to time (open3d is absent) and no earlier version of this work.
A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import mesh_bench  # noqa: E402

H, W = 1080, 1920
N_TRAJ = 2000


def room_mesh(P, res, dev):
    """mesh_bench's analytic room through the package's marching cubes → (vertices, faces) on the device."""
    cfg = dict(mesh_bench.CFG, meshing=dict(mesh_bench.CFG["meshing"], resolution=res))
    st = P.slam.SlamState(cfg, dev, n_img=2, generator=torch.Generator().manual_seed(2))
    vol, g = mesh_bench.room_volume(st.mesher, res, dev)
    x, y, z = (np.asarray(v) for v in g["xyz"])
    origin, spacing = (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1])
    return P.ops.marching_cubes(vol, 0.0, origin, spacing)


def poses():
    """N_TRAJ + 1 poses (the reference's convention: a camera looks along -z of its pose) walking along +x through the
    room's middle, and the same 10 cm to the side as the ground truth."""
    b = np.asarray(mesh_bench.CFG["mapping"]["marching_cubes_bound"])
    ctr = b.mean(1)
    base = np.eye(4)
    base[:3, :3] = np.array([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])     # columns x, y, z
    t = np.linspace(0.0, 1.0, N_TRAJ + 1)
    est = np.tile(base, (N_TRAJ + 1, 1, 1))
    est[:, 0, 3] = ctr[0] + 3.0 * t
    est[:, 1, 3] = ctr[1] + 0.8 * np.sin(6.0 * t)
    est[:, 2, 3] = ctr[2] + 0.3 * np.cos(4.0 * t)
    gt = est.copy()
    gt[:, 1, 3] += 0.1
    return est, gt


def median_ms(samples):
    return round(statistics.median(samples), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay_frame.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench: no HIP device; nothing here can be measured on the CPU")
    P = importlib.import_module("nice-slam_amd")
    ops = P.ops
    dev = torch.device("cuda:0")
    verts, faces = room_mesh(P, a.resolution, dev)
    col = np.random.default_rng(4).integers(0, 256, (verts.shape[0], 3)).astype(np.uint8)
    est, gt = poses()
    out = {"image": [H, W], "resolution": a.resolution, "V": int(verts.shape[0]), "F": int(faces.shape[0]),
           "actors": 2, "trajectory_points": 2 * N_TRAJ, "repeat": a.repeat, "stages_ms": {}}
    with tempfile.TemporaryDirectory() as tmp:
        ply = os.path.join(tmp, "00000_mesh.ply")
        P.mesher.write_ply(ply, verts.cpu().numpy(), faces.cpu().numpy(), col)
        out["ply_bytes"] = os.path.getsize(ply)
        del verts, faces
        r = P.replay.Replay(tmp, est[0], cam_scale=0.3, near=0, estimate_c2w_list=est, gt_c2w_list=gt, H=H, W=W)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.update_mesh(ply)
        torch.cuda.synchronize()
        out["mesh_load_upload_normals_ms_once"] = round((time.perf_counter() - t0) * 1e3, 2)
        r.update_pose(1, est[N_TRAJ // 2], gt=False)
        r.update_pose(1, gt[N_TRAJ // 2], gt=True)
        r.update_cam_trajectory(N_TRAJ + 1, gt=False)
        r.update_cam_trajectory(N_TRAJ + 1, gt=True)
        frame = r.render()                                   # the warm-up frame: buffers, point upload
        torch.cuda.synchronize()
        out["points"] = int(r._points[0].shape[0])
        out["background_share"] = round(float((frame == 255).all(-1).float().mean()), 4)
        v, f, c, n = r.mesh
        fx, fy, cx, cy = P.replay.intrinsics(H, W, r.fov)
        names = ("clear", "faces_inline", "faces_list", "points", "resolve")
        passes = (ops.RASTER_CLEAR, ops.RASTER_SMALL, ops.RASTER_BIG, ops.SCENE_POINTS, ops.RASTER_RESOLVE)
        per = {k: [] for k in names + ("copy_to_host", "jpeg_encode", "save_whole")}
        listed = None
        for _ in range(a.repeat):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(passes) + 1)]
            ev[0].record()
            for k, p in enumerate(passes):
                ops.render_scene(v, f, c, n, r._points[0], r._points[1], r._w2c, H, W, fx, fy, cx, cy, r.near,
                                 P.replay.Z_FAR, point_size=r.point_size, cull=r.cull, ws=r._ws, out=r._out, passes=p)
                ev[k + 1].record()
            torch.cuda.synchronize()
            for k, name in enumerate(names):
                per[name].append(ev[k].elapsed_time(ev[k + 1]))
            listed = ops.raster_list_length(r._ws)
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            host = r._out[0][0].cpu()
            a1.record()
            torch.cuda.synchronize()
            per["copy_to_host"].append(a0.elapsed_time(a1))
            t0 = time.perf_counter()
            data = P.visualizer.encode_jpeg(host.numpy())
            per["jpeg_encode"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            r.save(os.path.join(tmp, "frame.jpg"))
            per["save_whole"].append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(r._out[0][0], frame)               # the passes one by one draw the warm-up's frame
    out["listed_items"] = int(listed)
    out["jpeg_bytes"] = len(data)
    out["stages_ms"] = {k: median_ms(s) for k, s in per.items()}
    stage = {k: out["stages_ms"][k] for k in names + ("copy_to_host", "jpeg_encode")}
    out["device_ms"] = round(sum(out["stages_ms"][k] for k in names), 4)
    out["bound_by"] = max(stage, key=stage.get)
    out["notes"] = ("device-event medians of the five passes run in order, after one warm-up frame; jpeg_encode and "
                    "save_whole on the host clock; one run on one MI355X")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
