"""Golden vectors for the evaluation module, produced by the reference's own evaluation code (build container
only; the .npz it writes is what the tests read).

Run:  PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py

Recorded into tests/golden/eval_fixtures.npz (scenes: tests/golden/eval_scene.py):
  nn.dist, nn.idx, nn.second   scipy's cKDTree (the tree src/tools/eval_recon.py:24-42 builds) over the 4099 wall
                               targets, queried with the 4096 noisy wall points: nearest distance, its index and
                               the second-nearest distance (indices are compared only where the two differ)
  nn.metrics                   the reference's OWN accuracy, completion, completion_ratio (eval_recon.py:24-42) with
                               gt_points = the targets and rec_points = the queries
  cull.seen1 / seen9           per-vertex "inside some frustum" for the first pose and for all nine
  cull.margin1 / margin9       float64: the smallest of |u|, |u-W|, |v|, |v-H| and 100 |z| over the frames up to
                               the first in which the vertex is seen
  e2e.metrics                  accuracy [cm], completion [cm], completion ratio [%] of the two small meshes: the host
                               restatement of the sampler (eval_scene.sample_surface_host, seeds 0 and 1, 20000
                               points) followed by the reference's metric functions
  ate.values                   the reference's OWN evaluate_ate result dict (eval_ate.py:113-223), values in the
                               order of ATE_KEYS, for the 50-pose trajectory (two ground-truth poses masked)
  ate.rot, ate.trans           the reference's OWN align (eval_ate.py:44-78) on the same trajectories

Harness (nothing of the reference is copied or modified; it is imported and called):
  * src/tools/eval_recon.py imports open3d and trimesh at module level; neither is installed and neither is
    touched by the three metric functions.  Empty stand-in modules are registered first.  The functions use
    np.float, which numpy 2 removed: np.float = float is set before the import.
  * src/tools/cull_mesh.py is a script that parses arguments and calls .cuda(), and check_proj calls .cuda():
    neither runs here.  The cull fixture is therefore a float32 torch-CPU RESTATEMENT of cull_mesh.py:47-71, the
    same ops in the same order with .cuda() dropped: it pins the formulae, not the reference's run.
  * the share of vertices within 1e-3 of a decision threshold (left out of the GPU comparison) is asserted to
    stay under 1 %; if it does not, change the scene's seed, never the cap.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import eval_scene  # noqa: E402

for _name in ("open3d", "trimesh"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
if not hasattr(np, "float"):
    np.float = float

from scipy.spatial import cKDTree  # noqa: E402
from src.tools import eval_recon as ref_recon  # noqa: E402  (reference)
from src.tools import eval_ate as ref_ate  # noqa: E402  (reference)

ATE_KEYS = ("compared_pose_pairs", "absolute_translational_error.rmse", "absolute_translational_error.mean",
            "absolute_translational_error.median", "absolute_translational_error.std",
            "absolute_translational_error.min", "absolute_translational_error.max")


def cull_restatement(verts, poses, H, W, fx, fy, cx, cy):
    """The frustum test of cull_mesh.py:47-71 restated for the CPU: float32 torch ops in the reference's order
    ((4,4) @ (N,4,1) batched product, x negated in place, K @ cam, z = uv_z + 1e-5, uv / z, strict edges) →
    (seen bool [V], margin float64 [V])."""
    n = verts.shape[0]
    k32 = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64).float()
    p64 = torch.from_numpy(verts.copy())
    homo = torch.cat([p64, torch.ones(n, 1, dtype=p64.dtype)], dim=1).reshape(-1, 4, 1).float()
    seen = np.zeros(n, dtype=bool)
    margin = np.full(n, np.inf)
    for pose in poses:
        inv32 = torch.from_numpy(np.linalg.inv(pose)).float()   # float32 in, float32 out, as the reference's
        cam = (inv32 @ homo)[:, :3]
        cam[:, 0] *= -1
        pix = k32 @ cam
        depth = pix[:, -1:] + 1e-5
        pix = (pix[:, :2] / depth).squeeze(-1).numpy()
        front = 0 <= -depth[:, 0, 0].numpy()
        hit = front & (pix[:, 0] < W) & (pix[:, 0] > 0) & (pix[:, 1] < H) & (pix[:, 1] > 0)
        # float64 distances to the thresholds, from the float32 inputs those ops read
        m64 = inv32.numpy().astype(np.float64)
        q64 = verts.astype(np.float32).astype(np.float64)
        c64 = q64 @ m64[:3, :3].T + m64[:3, 3]
        zz = c64[:, 2] + 1e-5
        u, v = (fx * -c64[:, 0] + cx * c64[:, 2]) / zz, (fy * c64[:, 1] + cy * c64[:, 2]) / zz
        d = np.min(np.stack([np.abs(u), np.abs(u - W), np.abs(v), np.abs(v - H), 100.0 * np.abs(zz)], 0), 0)
        margin = np.where(seen, margin, np.minimum(margin, d))  # frames after the first hit are not read
        seen |= hit
    return seen, margin


def main():
    torch.set_num_threads(8)
    out = {}

    targets, queries = eval_scene.nn_scene()
    d, i = cKDTree(targets).query(queries, k=2)
    out["nn.dist"], out["nn.idx"], out["nn.second"] = d[:, 0], i[:, 0].astype(np.int32), d[:, 1]
    out["nn.metrics"] = np.array([ref_recon.accuracy(targets, queries), ref_recon.completion(targets, queries),
                                  ref_recon.completion_ratio(targets, queries)], dtype=np.float64)
    print("nn: mean dist", d[:, 0].mean(), "ties", int((d[:, 1] - d[:, 0] <= 1e-12).sum()), "metrics", out["nn.metrics"])

    verts, poses = eval_scene.cull_scene()
    cam = eval_scene.CAM
    for k in (1, eval_scene.N_POSES):
        seen, margin = cull_restatement(verts, poses[:k], cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"],
                                        cam["cy"])
        left_out = float((margin < eval_scene.CULL_MARGIN).mean())
        assert left_out <= eval_scene.CULL_MAX_LEFT_OUT, (k, left_out)
        assert 0.05 < seen.mean() < 0.95, (k, seen.mean())
        out[f"cull.seen{k}"], out[f"cull.margin{k}"] = seen.astype(np.uint8), margin
        print(f"cull {k} poses: seen {int(seen.sum())} of {seen.shape[0]}, left out {left_out:.4%}")

    # every seed of the sampling test keeps its per-face counts within 5 sigma (checked here, on the host
    # restatement, before the seeds are committed)
    sv, sf = eval_scene.sample_mesh()
    cdf = eval_scene.face_cdf(sv, sf)
    share = np.diff(np.concatenate([[0.0], cdf])) / cdf[-1]
    for seed in eval_scene.SAMPLE_SEEDS:
        _, fid, _ = eval_scene.sample_surface_host(sv, sf, cdf, eval_scene.SAMPLE_COUNT, seed)
        cnt = np.bincount(fid, minlength=sf.shape[0])
        sig = np.sqrt(eval_scene.SAMPLE_COUNT * share * (1 - share))
        dev = np.abs(cnt - eval_scene.SAMPLE_COUNT * share) / np.where(sig > 0, sig, 1.0)
        assert cnt[share == 0].sum() == 0 and dev.max() < 5.0, (seed, dev.max())
        print(f"sampler seed {seed}: worst face {dev.max():.2f} sigma")

    (gv, gf), (rv, rf) = eval_scene.e2e_meshes()
    gv, rv = (a.astype(np.float32).astype(np.float64) for a in (gv, rv))  # what the PLY stores
    rec_pc, _, _ = eval_scene.sample_surface_host(rv, rf, eval_scene.face_cdf(rv, rf), eval_scene.E2E_POINTS,
                                                  eval_scene.E2E_SEED)
    gt_pc, _, _ = eval_scene.sample_surface_host(gv, gf, eval_scene.face_cdf(gv, gf), eval_scene.E2E_POINTS,
                                                 eval_scene.E2E_SEED + 1)
    out["e2e.metrics"] = np.array([ref_recon.accuracy(gt_pc, rec_pc) * 100, ref_recon.completion(gt_pc, rec_pc) * 100,
                                   ref_recon.completion_ratio(gt_pc, rec_pc) * 100], dtype=np.float64)
    print("e2e: accuracy, completion [cm], ratio [%]", out["e2e.metrics"])

    gt, est = eval_scene.ate_scene()
    ok = np.array([bool(np.isfinite(p).all()) for p in gt])
    first = {int(k): gt[j][:3, 3] for k, j in enumerate(np.nonzero(ok)[0])}
    second = {int(k): est[j][:3, 3] for k, j in enumerate(np.nonzero(ok)[0])}
    res = ref_ate.evaluate_ate(first, second, "", [])
    out["ate.values"] = np.array([float(res[k]) for k in ATE_KEYS], dtype=np.float64)
    rot, trans, err = ref_ate.align(np.matrix(np.stack([second[k] for k in sorted(second)], 1).astype(np.float64)),
                                    np.matrix(np.stack([first[k] for k in sorted(first)], 1).astype(np.float64)))
    out["ate.rot"], out["ate.trans"] = np.asarray(rot), np.asarray(trans)
    print("ate:", dict(zip(ATE_KEYS, out["ate.values"])))

    path = os.path.join(HERE, "eval_fixtures.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
