#!/usr/bin/env python3
"""TSDF fusion at Replica room0 size: ms per stage, GB/s on algorithmic bytes, blocks, V and F.

    python tools/tsdf_bench.py [--keyframes 32] [--repeat 5] [--out profiles/tsdf_fuse.json]

Workload: `--keyframes` keyframes of the room0 camera (680x1200) looking at the analytic room of
tests/golden/scenes.py (box depths, random colours), fused at the reference's sizes (voxel 4/512, truncation
0.04: Mesher.get_bound_from_frames at scale 1).  Stages, each timed with device events after a warm-up call
(median of `--repeat`): range, touch, integrate, count, emit (csrc/nslam_tsdf.hip).
  integrate_torch   the integrate formulae of include/nslam.h written with torch operators on the same GPU, one
                    pass per frame over the blocks that frame touched: the bar.  nslam_tsdf_integrate must not
                    be slower than this
GB/s are algorithmic bytes (what the pass must read and write once, from shapes) over the measured time, against
the 8 TB/s HBM peak.  Mesher.get_bound_from_frames is timed with both methods on the same keyframes, wall clock,
one run each.  A run without a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import scenes  # noqa: E402

HBM_PEAK = 8.0e12
VOXEL, TRUNC, STRIDE, DEPTH_TRUNC = 4.0 / 512.0, 0.04, 4, 1000.0


def timed(fn, repeat):
    """Median device-event milliseconds of fn() after one warm-up call; returns (ms, last result)."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def torch_integrate(depth, color, w2c, intr, coords, masks, tsdf, weight, cpool, chunk=2048):
    """nslam_tsdf_integrate's contract in torch operators: per frame, the blocks whose mask has the frame's
    bit, `chunk` blocks at a time; float32 throughout, the operation order of include/nslam.h."""
    fx, fy, cx, cy = (torch.tensor(v, dtype=torch.float32, device=depth.device) for v in intr)
    K, H, W = depth.shape
    dev = depth.device
    loc = torch.arange(16, device=dev)
    lx, ly, lz = (g.reshape(-1) for g in torch.meshgrid(loc, loc, loc, indexing="ij"))
    local = torch.stack([lx, ly, lz], 1)                                          # [4096,3]
    inv_trunc = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(TRUNC, dtype=torch.float32)
    inv_trunc, trunc = float(inv_trunc), float(np.float32(TRUNC))
    for f in range(K):
        sel = torch.nonzero((masks >> f) & 1).reshape(-1)
        M = w2c[f]
        for s in range(0, sel.shape[0], chunk):
            b = sel[s:s + chunk]
            g = coords[b][:, None, :] * 16 + local[None]                          # [n,4096,3]
            p = ((g.double() + 0.5) * VOXEL).float()
            cam = [((M[r, 0] * p[..., 0] + M[r, 1] * p[..., 1]) + M[r, 2] * p[..., 2]) + M[r, 3] for r in range(3)]
            front = cam[2] > 0
            z = torch.where(front, cam[2], torch.ones_like(cam[2]))
            uf = ((cam[0] * fx) / z + cx) + 0.5
            vf = ((cam[1] * fy) / z + cy) + 0.5
            inside = front & (uf >= 1e-4) & (uf < float(np.float32(W) - np.float32(1e-4))) & (vf >= 1e-4) \
                & (vf < float(np.float32(H) - np.float32(1e-4)))
            u = torch.where(inside, uf, torch.ones_like(uf)).long()
            v = torch.where(inside, vf, torch.ones_like(vf)).long()
            pix = v * W + u
            d = depth[f].reshape(-1)[pix]
            valid = inside & (d > 0) & (d <= DEPTH_TRUNC)
            xn, yn = (u.float() - cx) / fx, (v.float() - cy) / fy
            m = torch.sqrt((xn * xn + yn * yn) + 1.0)
            sdf = (d - z) * m
            upd = valid & (sdf > -trunc)
            t = torch.clamp(sdf * inv_trunc, max=1.0)
            w = weight[b]
            w1 = w + 1.0
            tsdf[b] = torch.where(upd, (tsdf[b] * w + t) / w1, tsdf[b])
            if cpool is not None:
                px = color[f].reshape(-1, 3)[pix].float()
                for c in range(3):
                    cpool[c, b] = torch.where(upd, (cpool[c, b] * w + px[..., c]) / w1, cpool[c, b])
            weight[b] = torch.where(upd, w1, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_fuse.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench: no HIP device; nothing here can be measured on the CPU")
    if not 1 <= a.keyframes <= 32:
        raise SystemExit("tsdf_bench: 1 to 32 keyframes (one integrate call)")
    P = importlib.import_module("nice-slam_amd")
    ops, L = P.ops, P._lib.lib()
    dev = torch.device("cuda:0")
    cam = scenes.ROOM0_CAM
    H, W = cam["H"], cam["W"]
    intr = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    b = scenes.enlarge_bound(scenes.ROOM0_BOUND, 0.32)
    ctr = b.mean(1)
    Kf = a.keyframes
    poses = [scenes.look_pose(ctr, 0.6 * k, 0.12 * ((k % 3) - 1), (0.3 * ((k % 4) - 1.5), 0.2 * (k % 2), 0.05 * (k % 8)))
             for k in range(Kf)]
    depth = torch.from_numpy(np.stack([scenes.box_depth(p, cam, b, seed=k) for k, p in enumerate(poses)], 0)).to(dev)
    rng = np.random.default_rng(9)
    color = torch.from_numpy(rng.integers(0, 256, size=(Kf, H, W, 3), dtype=np.uint8)).to(dev)
    c2w = np.stack([P.tsdf.opengl_to_cv(p) for p in poses], 0)
    c2w64, w2c32 = P.tsdf._poses(c2w)
    c2w_d, w2c_d = torch.from_numpy(c2w64).to(dev), torch.from_numpy(w2c32).to(dev)
    out = {"keyframes": Kf, "image": [H, W], "voxel": VOXEL, "trunc": TRUNC, "stride": STRIDE, "repeat": a.repeat,
           "stages_ms": {}, "gbps": {}, "share_of_hbm_peak": {}}

    def rate(name, ms, nbytes):
        out["stages_ms"][name] = round(ms, 4)
        if nbytes:
            out["gbps"][name] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            out["share_of_hbm_peak"][name] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)

    n_samples = Kf * ((H + STRIDE - 1) // STRIDE) * ((W + STRIDE - 1) // STRIDE)
    ms, (bounds, n_valid) = timed(lambda: ops.tsdf_block_range(depth, c2w_d, H, W, *intr, STRIDE, DEPTH_TRUNC, VOXEL,
                                                               TRUNC), a.repeat)
    rate("range", ms, n_samples * 4)
    bl = bounds.cpu().tolist()
    lo, hi = bl[:3], [v + 1 for v in bl[3:]]
    cells = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    ms, (mask, n_out) = timed(lambda: ops.tsdf_touch(depth, c2w_d, H, W, *intr, STRIDE, DEPTH_TRUNC, VOXEL, TRUNC, lo,
                                                     hi), a.repeat)
    rate("touch", ms, n_samples * 4 + cells * 4)
    keys = torch.nonzero(mask).reshape(-1)
    n = int(keys.shape[0])
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    table = torch.full((cells,), -1, dtype=torch.int32, device=dev)
    table[keys] = ids
    key32, masks = keys.to(torch.int32), mask[keys].contiguous()
    out.update({"valid_samples": int(n_valid), "n_outside": int(n_out), "table": [lo, hi], "blocks": n,
                "voxels": n * 4096, "block_frame_pairs": int(sum(int(((masks >> f) & 1).sum()) for f in range(Kf)))})

    def pools():
        return (torch.zeros(n, 4096, device=dev), torch.zeros(n, 4096, device=dev), torch.zeros(3, n, 4096, device=dev))

    def hip(ts, w, cp):
        ops.tsdf_integrate(depth, color, w2c_d, H, W, *intr, DEPTH_TRUNC, VOXEL, TRUNC, lo, hi, key32, ids, masks, n,
                           ts, w, cp)

    scratch = pools()
    ms, _ = timed(lambda: hip(*scratch), a.repeat)
    image_bytes = Kf * H * W * 7
    rate("integrate", ms, n * 4096 * 4 * 10 + image_bytes)
    ny, nz = hi[1] - lo[1], hi[2] - lo[2]
    k64 = keys.long()
    coords = torch.stack([k64 // (ny * nz), (k64 // nz) % ny, k64 % nz], 1) + torch.tensor(lo, device=dev)
    ms_t, _ = timed(lambda: torch_integrate(depth, color, w2c_d, intr, coords, masks, *scratch), max(1, a.repeat // 2))
    rate("integrate_torch", ms_t, n * 4096 * 4 * 10 + image_bytes)
    del scratch
    ts, w, cp = pools()
    hip(ts, w, cp)
    ts2, w2, cp2 = pools()
    torch_integrate(depth, color, w2c_d, intr, coords, masks, ts2, w2, cp2)
    out["integrate"] = {"hip_not_slower_than_torch": bool(ms <= ms_t), "torch_over_hip": round(ms_t / ms, 2),
                        "voxels_whose_weight_differs_from_torch": int((w != w2).sum()),
                        "max_tsdf_difference_from_torch": float((ts - ts2).abs().max())}
    del ts2, w2, cp2

    stream = P._lib.stream_ptr(dev)
    i3 = lambda v: (__import__("ctypes").c_int32 * 3)(*v)  # noqa: E731
    nv = n * 4096
    flags = torch.empty(3 * nv, dtype=torch.uint8, device=dev)
    ntri = torch.empty(nv, dtype=torch.uint8, device=dev)
    ms, _ = timed(lambda: P._lib.check(L.nslam_tsdf_mc_count(ts.data_ptr(), w.data_ptr(), key32.data_ptr(), n,
                                                             table.data_ptr(), i3(lo), i3(hi), flags.data_ptr(),
                                                             ntri.data_ptr(), stream), "nslam_tsdf_mc_count"), a.repeat)
    rate("count", ms, nv * 8 + nv * 4)
    ms_all, (verts, faces, cols) = timed(lambda: ops.tsdf_marching_cubes(ts, w, cp, key32, n, table, lo, hi, VOXEL),
                                         a.repeat)
    out["stages_ms"]["extract_total_with_scans"] = round(ms_all, 4)
    V, Fc = int(verts.shape[0]), int(faces.shape[0])
    voff = (torch.cumsum(flags, 0, dtype=torch.int32) - flags).contiguous()
    foff = (torch.cumsum(ntri, 0, dtype=torch.int32) - ntri).contiguous()
    ms, _ = timed(lambda: P._lib.check(L.nslam_tsdf_mc_emit(ts.data_ptr(), w.data_ptr(), cp.data_ptr(), nv,
                                                            key32.data_ptr(), n, table.data_ptr(), i3(lo), i3(hi),
                                                            VOXEL, flags.data_ptr(), ntri.data_ptr(), voff.data_ptr(),
                                                            foff.data_ptr(), V, Fc, verts.data_ptr(), cols.data_ptr(),
                                                            faces.data_ptr(), stream), "nslam_tsdf_mc_emit"), a.repeat)
    rate("emit", ms, nv * 4 + nv * 16 + V * 27 + Fc * 12)
    out["V"], out["F"] = V, Fc
    del flags, ntri, voff, foff, ts, w, cp, verts, faces, cols

    # Mesher.get_bound_from_frames, both methods, wall clock, one run each
    mcfg = {"coarse": True, "scale": 1, "occupancy": True,
            "meshing": {"resolution": 256, "level_set": 0, "clean_mesh_bound_scale": 1.02,
                        "remove_small_geometry_threshold": 0.2, "color_mesh_extraction_method": "direct_point_query",
                        "get_largest_components": False, "depth_test": True},
            "mapping": {"marching_cubes_bound": [[-2.7, 8.7], [-3.0, 5.3], [-3.3, 3.1]]}}
    slam = SimpleNamespace(renderer=None, bound=torch.tensor(scenes.ROOM0_BOUND, dtype=torch.float64), nice=True,
                           verbose=False, **cam)
    mesher = P.Mesher(mcfg, None, slam)
    kfs = [{"est_c2w": torch.from_numpy(p), "depth": depth[k], "color": color[k].float() / 255.0}
           for k, p in enumerate(poses)]
    bound = {}
    for method in ("points", "tsdf"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        planes = mesher.get_bound_from_frames(kfs, 1, method=method)
        torch.cuda.synchronize()
        bound[method] = {"wall_s": round(time.perf_counter() - t0, 3), "planes": int(planes.shape[0])}
    out["get_bound_from_frames"] = bound
    out["notes"] = ("device-event medians after one warm-up; GB/s on algorithmic bytes vs 8 TB/s HBM; integrate bytes = "
                    "one read and one write of the five floats of every listed voxel plus the images once; "
                    "get_bound_from_frames: wall clock of one call each, host hull included")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
