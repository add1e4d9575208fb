"""Golden vectors for the TUM-RGBD pieces, produced by the reference's own code (build container only; the
.npz it writes is what tests/test_tum_cpu.py and tests/test_gpu_tum.py read).

Run:  PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tum.py

Cases (reference file:line they execute):
  tumrgbd   src/utils/datasets.py TUM_RGBD (:234-321: parse_list, associate_frames, the frame_rate=32 thinning,
            pose_matrix_from_quaternion, poses relative to the first kept frame) + BaseDataset.__getitem__
            (:77-113, with cam.distortion: the undistortion of the colour image, :85-88) on the synthetic
            folder of tum_scene.tum_sequence: '#' header lines, a colour frame without a depth and one without
            a pose within 0.08 s, two colour frames closer than 1/32 s, a tie between two depth stamps.
  track2    the seperate_LR camera loop (Tracker.py:202-247) over Tracker.optimize_cam_in_batch (:71-128), 4
            iterations on the tiny scene: quad / T leaves in two Adam groups (0.001, 0.0002), camera_tensor =
            cat([quad, T]) at the top of every iteration, the candidate kept by loss < current_min_loss.

Harness (nothing of the reference is copied or modified; it is imported and called):
  * cv2 (absent) is make_golden_io.py's stand-in plus `undistort`, tum_scene.undistort_u8: the numpy
    restatement of cv2.undistort's defaults.  The fixture therefore pins the reference's code AROUND that
    call (where it is applied: the colour image only, before /255, before the crops); parity of the
    undistortion with OpenCV itself stays unpinned (library absent).
  * parse_list asks for dtype=np.unicode_, which numpy 2 removed: it is aliased to np.str_ for the call.
  * scipy is present here, so the reference's Rotation.from_quat runs as it is.
  * the tracking case uses make_golden_loop.py's harness (FixedDraws for select_uv, CPU get_device,
    quat_from_c2w for get_tensor_from_camera) and the `track` case's scene and start pose.
  * The input files are stored in the .npz, so the tests rebuild exactly the folder the reference read.
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import tum_scene  # noqa: E402
from make_golden_io import install_cv2, write_files  # noqa: E402


def install_undistort():
    install_cv2()
    cv2 = sys.modules["cv2"]

    def undistort(src, K, dist):
        K = np.asarray(K, dtype=np.float64)
        return tum_scene.undistort_u8(src, K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.asarray(dist).reshape(-1))

    cv2.undistort = undistort


def tum_case(out):
    from src.utils import datasets as R  # (reference)
    if not hasattr(np, "unicode_"):
        np.unicode_ = np.str_
    files = tum_scene.tum_sequence()
    cam = dict(tum_scene.SEQ_CAM)
    with tempfile.TemporaryDirectory() as d:
        write_files(d, files)
        cfg = {"dataset": "tumrgbd", "data": {"input_folder": d}, "cam": cam}
        ds = R.TUM_RGBD(cfg, SimpleNamespace(input_folder=None), tum_scene.SEQ_SCALE, device="cpu")
        out["tumrgbd.n"] = np.array(len(ds))
        out["tumrgbd.color_paths"] = np.array([os.path.relpath(p, d) for p in ds.color_paths])
        out["tumrgbd.depth_paths"] = np.array([os.path.relpath(p, d) for p in ds.depth_paths])
        for i in range(len(ds)):
            idx, color, depth, pose = ds[i]
            out[f"tumrgbd.{i}.index"] = np.array(idx)
            out[f"tumrgbd.{i}.color"] = color.numpy()
            out[f"tumrgbd.{i}.depth"] = depth.numpy()
            out[f"tumrgbd.{i}.pose"] = pose.numpy()
    names = sorted(files)
    out["tumrgbd.files"] = np.array(names)
    for k, rel in enumerate(names):
        out[f"tumrgbd.file{k}"] = np.frombuffer(files[rel], dtype=np.uint8)
    out["tumrgbd.scale"] = np.array(tum_scene.SEQ_SCALE)
    for k, v in cam.items():
        out[f"tumrgbd.cam.{k}"] = np.array(v)
    kept = [(f"rgb/{tum_scene.SEQ_COLOR_T[i]}.png", f"depth/{tum_scene.SEQ_DEPTH_T[j]}.png")
            for i, j, _ in tum_scene.SEQ_KEPT]
    assert [tuple(p) for p in zip(out["tumrgbd.color_paths"], out["tumrgbd.depth_paths"])] == kept, \
        (out["tumrgbd.color_paths"], out["tumrgbd.depth_paths"])


def track2_case(out, iters=4, draw_seed=26):
    import make_golden_loop as L  # (registers its stand-ins, imports the reference's Tracker)
    import scenes
    from make_golden import ref_nice, ref_renderer
    bound, sd, grids = L.tiny_inputs()
    cam = SimpleNamespace(**scenes.TINY_CAM)
    b, _, cur = scenes.tiny_window()
    c2w = torch.from_numpy(cur)
    depth = torch.from_numpy(scenes.box_depth(cur, scenes.TINY_CAM, b, seed=40))
    color = torch.from_numpy(scenes.color_image(scenes.TINY_CAM, seed=41))
    r = ref_renderer(bound)
    r.H, r.W, r.fx, r.fy, r.cx, r.cy = cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy
    tr = object.__new__(L.ref_tracker_mod.Tracker)
    tr.__dict__.update(device="cpu", H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, ignore_edge_W=20,
                       ignore_edge_H=20, nice=True, bound=bound, renderer=r, c={k: v.clone() for k, v in grids.items()},
                       decoders=ref_nice(sd, bound), handle_dynamic=True, use_color_in_tracking=True, w_color_loss=0.5)
    start = c2w.clone()
    start[:3, 3] += torch.tensor([0.03, -0.02, 0.015])
    cam0 = L.quat_from_c2w(start)
    lr = 0.001
    # Tracker.py:202-214
    T = cam0[-3:].clone().requires_grad_(True)
    quad = cam0[:4].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [T], "lr": lr}, {"params": [quad], "lr": lr * 0.2}])
    tops, losses = [], []
    candidate, current_min_loss, best_iter = None, 10000000000., -1
    with L.cpu_get_device(), L.fixed_draws(draw_seed):
        for it in range(iters):  # Tracker.py:225-247
            camera_tensor = torch.cat([quad, T], 0)
            tops.append(camera_tensor.detach().clone())
            loss = tr.optimize_cam_in_batch(camera_tensor, color, depth, 200, opt)
            losses.append(loss)
            if loss < current_min_loss:
                current_min_loss = loss
                candidate = camera_tensor.clone().detach()
                best_iter = it
    final = torch.cat([quad, T], 0).detach().clone()
    out.update({"track2.cam0": cam0.numpy(), "track2.losses": np.asarray(losses), "track2.tops": torch.stack(tops).numpy(),
                "track2.final": final.numpy(), "track2.candidate": candidate.numpy(),
                "track2.best_iter": np.int64(best_iter), "track2.lr": np.float64(lr), "track2.lr_quat": np.float64(lr * 0.2),
                "track2.depth_seed": np.int64(40), "track2.color_seed": np.int64(41),
                "track2.draw_seed": np.int64(draw_seed), "track2.pixels": np.int64(200)})


def main():
    install_undistort()
    out = {}
    tum_case(out)
    track2_case(out)
    path = os.path.join(HERE, "tum_fixtures.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.1f} kB")
    print("kept", list(out["tumrgbd.color_paths"]), list(out["tumrgbd.depth_paths"]))
    print("track2 losses", out["track2.losses"], "best", out["track2.best_iter"])


if __name__ == "__main__":
    main()
