"""Golden vectors for the mesher, produced by the reference's own Mesher code (build container only; the
.npz it writes is what the tests read).

Run:  PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mesh.py

Recorded into tests/golden/mesh_fixtures.npz:
  grid_points, grid_x/y/z   Mesher.get_grid_uniform (Mesher.py:321-347) at resolution 7 over the tiny
                            scene's marching-cubes bound
  masks.<case>              Mesher.point_masks (Mesher.py:53-212) → uint8 [3,4096] (seen, forecast, unseen)
                            for the scene of tests/golden/mesh_scene.py: 4096 points over and around the tiny
                            bound, 3 keyframes with 32x24 depth images.  Cases: depth_test on / off with the
                            reference chunking points_batch_size = 1024 (four chunks: the per-chunk depth
                            maximum of Mesher.py:166 matters) and with one chunk of 4096, and
                            get_mask_use_all_frames.

Harness (nothing of the reference is copied or modified; it is imported and called):
  * src/utils/Mesher.py imports open3d, skimage and trimesh at module level and src/utils/datasets.py
    imports cv2; none is installed and none is touched by the two methods recorded.  Empty stand-in
    modules are registered first.
  * the Mesher is built without __init__ (which would construct a dataset reader); the attributes the two
    methods read are set by hand.
  * every point keeps |z| > 1e-3 in every keyframe (asserted): the NaN / inf path of a point on a camera
    plane (z = -1e-8) is not pinned by this fixture.
  * the share of points within 1e-4 of a decision threshold (left out of the GPU comparison) is asserted to
    stay under 2 %; if it does not, change mesh_scene.SEED, never the cap.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mesh_scene  # noqa: E402

for _name in ("open3d", "skimage", "trimesh", "cv2"):
    sys.modules.setdefault(_name, types.ModuleType(_name))

from src.utils.Mesher import Mesher as RefMesher  # noqa: E402  (reference)


def ref_mesher(depth_test, batch):
    m = object.__new__(RefMesher)
    m.points_batch_size = batch
    m.depth_test = depth_test
    m.scale = 1
    m.marching_cubes_bound = torch.from_numpy(np.array(mesh_scene.MC_BOUND) * m.scale)
    for k, v in mesh_scene.CAM.items():
        setattr(m, k, v)
    return m


def main():
    torch.set_num_threads(8)
    out = {}
    g = ref_mesher(True, mesh_scene.BATCH).get_grid_uniform(mesh_scene.GRID_RES)
    out["grid_points"] = g["grid_points"].numpy()
    for name, ax in zip("xyz", g["xyz"]):
        out["grid_" + name] = np.asarray(ax, dtype=np.float64)

    pts, poses, depths = mesh_scene.mask_scene()
    kfs = [{"est_c2w": torch.from_numpy(p.copy()), "depth": torch.from_numpy(d.copy())} for p, d in zip(poses, depths)]
    c2w_list = torch.from_numpy(np.stack(poses, 0))
    cases = {"dt1_b1024": (True, mesh_scene.BATCH, False), "dt1_b4096": (True, mesh_scene.N_POINTS, False),
             "dt0_b1024": (False, mesh_scene.BATCH, False), "dt0_b4096": (False, mesh_scene.N_POINTS, False),
             "all_b1024": (True, mesh_scene.BATCH, True)}
    for name, (dt, batch, use_all) in cases.items():
        m = ref_mesher(dt, batch)
        s, f, u = m.point_masks(torch.from_numpy(pts.copy()), kfs, c2w_list, len(poses) - 1, "cpu",
                                get_mask_use_all_frames=use_all)
        out["masks." + name] = np.stack([s, f, u], 0).astype(np.uint8)
        margin, zmin = mesh_scene.mask_margins(pts, poses, depths, dt, use_all, batch)
        left_out = float((margin < mesh_scene.MARGIN).mean())
        assert zmin.min() > 1e-3, (name, zmin.min())
        assert left_out <= mesh_scene.MAX_LEFT_OUT, (name, left_out)
        print(f"{name}: seen {int(s.sum())} forecast {int(f.sum())} unseen {int(u.sum())} "
              f"left out {left_out:.4f} min|z| {zmin.min():.2e}")
    # the chunking must matter in depth_test mode, and only there
    assert (out["masks.dt1_b1024"] != out["masks.dt1_b4096"]).any()
    assert (out["masks.dt0_b1024"] == out["masks.dt0_b4096"]).all()
    path = os.path.join(HERE, "mesh_fixtures.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
