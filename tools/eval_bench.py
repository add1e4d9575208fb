#!/usr/bin/env python3
"""The evaluation kernels at Replica room0 size: ms per stage against the two bars.

    python tools/eval_bench.py [--poses 2000] [--samples 200000] [--repeat 5] [--views 1000] [--raster_repeat 3]
                               [--out profiles/eval_recon.json]

Workload, made procedurally (timing only): the room0 bound as a tessellated box of ~600 k vertices / 1.2 M faces
with a smooth bump on every wall, 2000 camera poses around the room centre at 680x1200, 200 k surface samples per
cloud, and 600 k / 1 M vertex clouds for ICP.  Stages, device-event medians of `--repeat` after a warm-up call:
  cull_hip          nslam_frustum_seen over every vertex and pose + nslam_mesh_face_cull
  cull_torch        cull_mesh.py's formulae as the reference writes them, in torch on the same GPU with the
                    per-frame device-to-host copy it makes: the bar for cull_hip (run once)
  areas_cdf, sample nslam_face_areas + cumsum, nslam_sample_surface
  nn_build/query    the cell grid over 200 k samples and the 200 k x 200 k query, both directions
  kdtree_*          scipy.spatial.cKDTree build and query on the host threads (workers = 16 at most): the bar
                    for the nearest-neighbour stages (wall-clock; skipped when scipy is absent)
  icp_iteration     one ICP iteration at 600 k source / 1 M target vertices (query within 0.1 + Kabsch sums +
                    transform), icp_align the whole loop; kdtree_icp_query the same query on the host
  depth_l1          the 2D metric's stages on the same mesh: `--views` (1000) views at 500x500 drawn by
                    sample_views, in batches as calc_depth_l1 makes them; per stage (clear, small pass, big pass,
                    resolve, L1, view rejection of 2000 candidates against a 100 k-point cloud) the sum over the
                    batches, median of `--raster_repeat`; the length of the big list; face-views/s and pixels/s;
                    and the small + big time of one batch for a sweep of small_max_pixels.  The reference's path
                    needs an OpenGL window: nothing was compared, no bar exists.
No time or ratio was fixed in advance: the file records what the kernels do against those two bars.  A run without
a HIP device fails: nothing here is measurable on the CPU.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import scenes  # noqa: E402


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


def wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def box_mesh(bound, n, dev, bump=0.05):
    """The box `bound` with every wall an n x n vertex grid pushed in and out by a smooth bump → (vertices
    float64 [6 n², 3], faces int32 [12 (n-1)², 3]) on the device."""
    b = torch.as_tensor(np.asarray(bound, dtype=np.float64), device=dev)
    s = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev)
    u, v = torch.meshgrid(s, s, indexing="ij")
    i, j = torch.meshgrid(torch.arange(n - 1, device=dev), torch.arange(n - 1, device=dev), indexing="ij")
    q = (i * n + j).reshape(-1)
    quad = torch.stack([q, q + n, q + n + 1, q, q + n + 1, q + 1], 1).reshape(-1, 3)
    verts, faces = [], []
    for ax in range(3):
        o = [a for a in range(3) if a != ax]
        for side in range(2):
            p = torch.empty(n, n, 3, dtype=torch.float64, device=dev)
            p[..., o[0]] = b[o[0], 0] + u * (b[o[0], 1] - b[o[0], 0])
            p[..., o[1]] = b[o[1], 0] + v * (b[o[1], 1] - b[o[1], 0])
            p[..., ax] = b[ax, side] + bump * torch.sin(9.0 * u + ax) * torch.cos(7.0 * v + side)
            faces.append(quad + len(verts) * n * n)
            verts.append(p.reshape(-1, 3))
    return torch.cat(verts).contiguous(), torch.cat(faces).to(torch.int32).contiguous()


def torch_cull(points64, poses, H, W, fx, fy, cx, cy):
    """cull_mesh.py:47-71 as the reference writes it (one frame per pass, mask copied to the host and
    accumulated there) → numpy bool [V]: seen by some frame."""
    dev = points64.device
    unseen = np.ones(points64.shape[0], dtype=bool)
    K = torch.tensor([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]], dtype=torch.float64, device=dev)
    for c2w in poses:
        w2c = torch.from_numpy(np.linalg.inv(c2w)).to(dev).float()
        ones = torch.ones_like(points64[:, 0]).reshape(-1, 1)
        homo = torch.cat([points64, ones], dim=1).reshape(-1, 4, 1).float()
        cam = (w2c @ homo)[:, :3]
        cam[:, 0] *= -1
        uv = K.float() @ cam.float()
        z = uv[:, -1:] + 1e-5
        uv = (uv[:, :2] / z).float().squeeze(-1).cpu().numpy()
        zz = z[:, 0, 0].cpu().numpy()
        unseen &= ~((0 <= -zz) & (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0))
    return ~unseen

def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def depth_l1_leg(P, verts, faces, bound, n_views, repeat, dev):
    """The stages of calc_depth_l1 on the procedural mesh → the "depth_l1" entry of the output."""
    E, ops = P.evaluation, P.ops
    H = W = 500
    fx = fy = 300.0
    cx = cy = 249.5
    z_near, z_far = 0.01 * float((bound[:, 1] - bound[:, 0]).max()), 20.0
    ctr, size = bound.mean(1), bound[:, 1] - bound[:, 0]
    box = np.eye(4)
    box[:3, 3] = ctr
    extents = 0.6 * size
    # the unseen cloud: a 1.5 m patch half a metre behind the +x wall
    g = np.random.default_rng(0)
    pc = np.stack([np.full(100000, bound[0, 1] + 0.5), ctr[1] + 1.5 * (g.random(100000) - 0.5),
                   ctr[2] + 1.5 * (g.random(100000) - 0.5)], 1)
    pc_d = torch.from_numpy(pc).to(dev)
    cand = E.sample_views(2000, extents, box, None, 0)
    cw = torch.from_numpy(E._check_proj_w2c(cand)).to(dev).contiguous()
    ms_rej, seen = timed(lambda: ops.views_see_any(pc_d, cw, H, W, fx, fy, cx, cy), repeat)
    views = E.sample_views(n_views, extents, box, pc, 0, H, W, fx, fy, cx, cy)
    w2c = torch.from_numpy(np.linalg.inv(views)[:, :3, :].copy()).to(dev).contiguous()
    rec = (verts + torch.tensor([0.01, -0.005, 0.02], dtype=torch.float64, device=dev)).contiguous()
    per = max(1, E.VIEW_BATCH_BYTES // (2 * 4 * H * W))
    ws = torch.empty(ops.RASTER_WS_BYTES, dtype=torch.uint8, device=dev)
    cap = (ws.numel() - 16) // 8
    args = (H, W, fx, fy, cx, cy, z_near, z_far)
    names = (("clear", ops.RASTER_CLEAR), ("small_pass", ops.RASTER_SMALL), ("big_pass", ops.RASTER_BIG),
             ("resolve", ops.RASTER_RESOLVE))

    def run(small_max, batches):
        """One pass over `batches` view batches of the ground-truth mesh, stage by stage, then the reconstruction
        in one call and the L1 → (stage ms summed over the batches, list lengths, per-view errors)."""
        t = {k: 0.0 for k, _ in names}
        t["l1"] = 0.0
        lens, errs = [], []
        for v0 in batches:
            m = w2c[v0:v0 + per]
            d_gt = torch.empty(m.shape[0], H, W, dtype=torch.float32, device=dev)
            for k, bit in names:
                ms, _ = event_ms(lambda: ops.render_depth(verts, faces, m, *args, small_max_pixels=small_max, ws=ws,
                                                          passes=bit, out=d_gt))
                t[k] += ms
                if bit == ops.RASTER_SMALL:
                    lens.append(ops.raster_list_length(ws))
            d_rec = ops.render_depth(rec, faces, m, *args, small_max_pixels=small_max, ws=ws)
            ms, e = event_ms(lambda: ops.depth_l1(d_gt, d_rec))
            t["l1"] += ms
            errs.append(e)
        return t, lens, torch.cat(errs)

    starts = list(range(0, n_views, per))
    run(None, starts[:1])                                         # warm-up
    sweep = {}
    for sm in (4, 16, 64, 256, 1024, H * W):
        t, lens, _ = run(sm, starts[:1])
        sweep[str(sm)] = {"small_pass_ms": round(t["small_pass"], 3), "big_pass_ms": round(t["big_pass"], 3),
                          "list_items": lens[0], "list_overflowed": bool(lens[0] > cap)}
    # the opposite mesh: the room as 12 triangles, every one of which fills a large part of an image — the work
    # the list pass exists for (a wall of a real ground-truth mesh is a few such triangles)
    fine = (verts, faces, rec)
    verts, faces = box_mesh(bound, 2, dev, bump=0.0)
    rec = verts
    coarse = {}
    run(None, starts[:1])
    for sm in (64, 1024, 16384, H * W):
        t, lens, _ = run(sm, starts[:1])
        coarse[str(sm)] = {"small_pass_ms": round(t["small_pass"], 3), "big_pass_ms": round(t["big_pass"], 3),
                           "list_items": lens[0]}
    verts, faces, rec = fine
    runs = [run(None, starts) for _ in range(repeat)]
    med = {k: round(statistics.median(r[0][k] for r in runs), 3) for k in runs[0][0]}
    med["view_rejection_2000_candidates"] = round(ms_rej, 4)
    lens, errs = runs[-1][1], runs[-1][2]
    raster_ms = med["clear"] + med["small_pass"] + med["big_pass"] + med["resolve"]
    same = all(torch.equal(r[2], errs) for r in runs)
    return {"views": n_views, "image": [H, W], "views_per_batch": per, "z_near": z_near, "z_far": z_far,
            "small_max_pixels": ops.RASTER_SMALL_MAX_PIXELS, "list_capacity": cap,
            "stages_ms_one_mesh": med, "big_list_items_total": int(sum(lens)),
            "big_list_items_max_batch": int(max(lens)),
            "list_overflowed": bool(max(lens) > cap),
            "face_views_per_s": round(faces.shape[0] * n_views / ((med["small_pass"] + med["big_pass"]) * 1e-3), 1),
            "pixels_per_s": round(n_views * H * W / (raster_ms * 1e-3), 1),
            "candidates_rejected_of_2000": int(seen.sum()), "depth_l1_cm": float(errs.mean()) * 100,
            "errors_equal_across_repeats": bool(same), "small_max_pixels_sweep_one_batch": sweep,
            "small_max_pixels_sweep_one_batch_12_triangle_room": coarse,
            "compared_with": "nothing: the reference renders through an open3d OpenGL window; no bar exists",
            "notes": "all figures measured on this run; device-event times, each stage summed over the view batches "
                     "of the ground-truth mesh (the reconstruction costs the same again), median of the repeats; "
                     "the sweep is one batch, run once per value"}


def recon_leg(P, a, verts, faces, bound, dev):
    """cull, sampling, nearest neighbours and ICP → the output's entries for them."""
    E, ops = P.evaluation, P.ops
    cam = scenes.ROOM0_CAM
    ctr = bound.mean(1)
    big, _ = box_mesh(bound, 408, dev)
    poses = np.stack([scenes.look_pose(ctr, 0.011 * k, 1.1 + 0.4 * np.sin(0.05 * k),
                                       (1.5 * np.sin(0.02 * k), 1.0 * np.cos(0.03 * k), 0.3 * np.sin(0.07 * k)))
                      for k in range(a.poses)], 0).astype(np.float32)
    threads = min(16, os.cpu_count() or 1)
    out = {"vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "poses": a.poses, "samples": a.samples,
           "icp_source": int(verts.shape[0]), "icp_target": int(big.shape[0]), "image": [cam["H"], cam["W"]],
           "repeat": a.repeat, "host_threads": threads, "stages_ms": {}}
    st = out["stages_ms"]

    # ---- cull
    w2c = torch.from_numpy(np.stack([np.linalg.inv(p).astype(np.float32) for p in poses], 0)).to(dev).contiguous()
    args = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ms, seen = timed(lambda: ops.frustum_seen(verts, w2c, *args), a.repeat)
    st["frustum_seen_hip"] = round(ms, 4)
    ms, keep = timed(lambda: ops.mesh_face_cull(faces, ~seen), a.repeat)
    st["face_cull_hip"] = round(ms, 4)
    st["cull_hip"] = round(st["frustum_seen_hip"] + st["face_cull_hip"], 4)
    torch_cull(verts, poses[:2], *args)                       # warm-up
    torch.cuda.synchronize()
    ms_t, ref_seen = wall_ms(lambda: torch_cull(verts, poses, *args))
    st["cull_torch"] = round(ms_t, 2)
    out["cull"] = {"seen": int(seen.sum()), "faces_kept": int(keep.sum()),
                   "vertices_differing_from_torch": int((seen.cpu().numpy() != ref_seen).sum()),
                   "torch_over_hip": round(ms_t / st["cull_hip"], 1)}

    # ---- sampling
    ms, area = timed(lambda: torch.cumsum(ops.face_areas(verts, faces), 0), a.repeat)
    st["areas_cdf"] = round(ms, 4)
    ms, (rec_pc, _, _) = timed(lambda: ops.sample_surface(verts, faces, a.samples, 0, cdf=area), a.repeat)
    st["sample_surface"] = round(ms, 4)
    shifted = verts + torch.tensor([0.01, -0.005, 0.02], dtype=torch.float64, device=dev)
    gt_pc, _, _ = ops.sample_surface(shifted.contiguous(), faces, a.samples, 1)

    # ---- nearest neighbours
    ms, grid = timed(lambda: ops.NNGrid(gt_pc), a.repeat)
    st["nn_build"] = round(ms, 4)
    ms, (d_acc, _) = timed(lambda: grid.query(rec_pc), a.repeat)
    st["nn_query"] = round(ms, 4)
    rgrid = ops.NNGrid(rec_pc)
    ms, (d_comp, _) = timed(lambda: rgrid.query(gt_pc), a.repeat)
    st["nn_query_reverse"] = round(ms, 4)
    out["nn"] = {"grid": list(grid.dims), "cell": grid.cell, "accuracy_cm": float(d_acc.mean()) * 100,
                 "completion_cm": float(d_comp.mean()) * 100}
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
        out["nn"]["kdtree"] = "scipy is not installed: no host bar"
    if cKDTree is not None:
        g_h, r_h = gt_pc.cpu().numpy(), rec_pc.cpu().numpy()
        ms_b, tree = wall_ms(lambda: cKDTree(g_h))
        ms_q, (d_h, _) = wall_ms(lambda: tree.query(r_h, workers=threads))
        st["kdtree_build"], st["kdtree_query"] = round(ms_b, 2), round(ms_q, 2)
        out["nn"]["max_abs_vs_kdtree"] = float(np.abs(d_acc.cpu().numpy() - d_h).max())
        out["nn"]["kdtree_over_hip"] = round((ms_b + ms_q) / (st["nn_build"] + st["nn_query"]), 1)

    # ---- ICP
    c, s = np.cos(np.deg2rad(1.0)), np.sin(np.deg2rad(1.0))   # the source: the mesh's vertices, moved a little
    src = ops.transform_points(verts, [[c, -s, 0.0, 0.02], [s, c, 0.0, -0.015], [0.0, 0.0, 1.0, 0.01]])
    ms, tgrid = timed(lambda: ops.NNGrid(big), max(1, a.repeat // 2))
    st["icp_target_build"] = round(ms, 4)

    def iteration():
        _, idx = tgrid.query(src, 0.1)
        s = ops.kabsch_sums(src, idx, big)
        return ops.transform_points(src, np.eye(4)), s
    ms, (_, sums) = timed(iteration, a.repeat)
    st["icp_iteration"] = round(ms, 4)
    ms, (_, idx) = timed(lambda: tgrid.query(src, 0.1), a.repeat)
    st["icp_query"] = round(ms, 4)
    ms, _ = timed(lambda: ops.kabsch_sums(src, idx, big), a.repeat)
    st["kabsch_sums_with_readback"] = round(ms, 4)
    ms_i, trans = wall_ms(lambda: E.icp_align(src, big))
    st["icp_align"] = round(ms_i, 2)
    out["icp"] = {"matched": int(sums[0]), "translation_found": [float(v) for v in trans[:3, 3]]}
    if cKDTree is not None:
        b_h, s_h = big.cpu().numpy(), src.cpu().numpy()
        ms_b, tree = wall_ms(lambda: cKDTree(b_h))
        ms_q, _ = wall_ms(lambda: tree.query(s_h, distance_upper_bound=0.1, workers=threads))
        st["kdtree_icp_build"], st["kdtree_icp_query"] = round(ms_b, 2), round(ms_q, 2)
        out["icp"]["kdtree_query_over_hip_query"] = round(ms_q / st["icp_query"], 1)
    out["notes"] = ("device-event medians after one warm-up; cull_torch, kdtree_* and icp_align are wall-clock, run "
                    "once; procedural room0-sized inputs (timing only); no target was set for these kernels")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--raster_repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_recon.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no HIP device; nothing here can be measured on the CPU")
    P = importlib.import_module("nice-slam_amd")
    dev = torch.device("cuda:0")
    bound = np.asarray(scenes.ROOM0_BOUND)
    verts, faces = box_mesh(bound, 316, dev)
    out = recon_leg(P, a, verts, faces, bound, dev)
    out["depth_l1"] = depth_l1_leg(P, verts, faces, bound, a.views, a.raster_repeat, dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
