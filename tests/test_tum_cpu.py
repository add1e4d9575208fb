"""TUM-RGBD on the host: the loader against the reference's own output, the host undistortion against the
independent numpy restatement, and the two new entry points' argument checks (no GPU calls).

tests/golden/tum_fixtures.npz was written by tests/golden/make_golden_tum.py, which ran the reference's
src/utils/datasets.py TUM_RGBD (parse_list, associate_frames, the frame_rate=32 thinning, scipy's quaternion
conversion, BaseDataset.__getitem__ with cam.distortion) in the build container on the synthetic folder of
tests/golden/tum_scene.py; the folder's files are stored in the fixture.  Pinned to the reference: the '#'
lines and the skipped first pose row, the association (nearest stamp, first index on a tie, both gaps < 0.08 s),
the thinning, the relative poses and their y/z flip, where the undistortion is applied (the colour image only,
before /255 and the crops), png_depth_scale, crop_size, crop_edge, scale.  Unpinned (cv2 absent): OpenCV's own
undistortion — the reference ran tum_scene.undistort_u8, the numpy restatement of cv2.undistort's defaults.
"""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import tum_scene  # noqa: E402

P = importlib.import_module("nice-slam_amd")
FIX = os.path.join(GOLDEN, "tum_fixtures.npz")


@pytest.fixture(scope="module")
def fx():
    with np.load(FIX) as z:
        return {k: z[k] for k in z.files}


def rebuild_tum(fx, root):
    """The folder the reference read, and its config."""
    for k, rel in enumerate(fx["tumrgbd.files"]):
        p = os.path.join(root, str(rel))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(fx[f"tumrgbd.file{k}"].tobytes())
    cam = {}
    for key in fx:
        if key.startswith("tumrgbd.cam."):
            v = fx[key]
            cam[key[len("tumrgbd.cam."):]] = v.tolist() if v.ndim else v.item()
    return {"dataset": "tumrgbd", "data": {"input_folder": str(root)}, "cam": cam}


def test_tum_loader_matches_reference(fx, tmp_path):
    cfg = rebuild_tum(fx, tmp_path)
    assert len(cfg["cam"]["distortion"]) == 5 and cfg["cam"]["crop_size"] == [40, 52] and cfg["cam"]["crop_edge"] == 2
    ds = P.get_dataset(cfg, None, float(fx["tumrgbd.scale"]), device="cpu")
    assert isinstance(ds, P.datasets.TUM_RGBD)
    assert len(ds) == int(fx["tumrgbd.n"]) == len(tum_scene.SEQ_KEPT)
    # the chosen files: the thinned-out frame, the frame without a depth and the one without a pose are gone,
    # and the tie between two depth stamps went to the first
    assert [os.path.relpath(p, tmp_path) for p in ds.color_paths] == [str(s) for s in fx["tumrgbd.color_paths"]]
    assert [os.path.relpath(p, tmp_path) for p in ds.depth_paths] == [str(s) for s in fx["tumrgbd.depth_paths"]]
    assert [os.path.basename(p) for p in ds.depth_paths][2] == "11.9375.png"
    for i in range(len(ds)):
        idx, color, depth, pose = ds[i]
        assert idx == int(fx[f"tumrgbd.{i}.index"])
        ref_c, ref_d, ref_p = fx[f"tumrgbd.{i}.color"], fx[f"tumrgbd.{i}.depth"], fx[f"tumrgbd.{i}.pose"]
        assert color.dtype == torch.float64 and tuple(color.shape) == ref_c.shape == (36, 48, 3)
        assert depth.dtype == torch.float32 and tuple(depth.shape) == ref_d.shape
        assert pose.dtype == torch.float32
        assert np.array_equal(depth.numpy(), ref_d), i
        # numpy's quaternion conversion here, scipy's there: float64 rounding before the float32 cast
        np.testing.assert_allclose(pose.numpy(), ref_p, rtol=1e-6, atol=0, err_msg=str(i))
        err = float(np.abs(color.numpy() - ref_c).max())
        assert err < 1e-12, (i, err)
    # the first kept pose is exactly eye(4) before the y/z flip (and so is the reference's)
    flip = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    first = P.get_dataset(cfg, None, float(fx["tumrgbd.scale"]), device="cpu").poses[0].numpy()
    assert np.array_equal(first @ flip, np.eye(4, dtype=np.float32))
    assert np.array_equal(fx["tumrgbd.0.pose"] @ flip, np.eye(4, dtype=np.float32))


def test_tum_pose_file_fallback_and_first_row(fx, tmp_path):
    """pose.txt is read when groundtruth.txt is absent, and the pose file's first row is skipped whatever it
    holds (skiprows=1): the same folder with the file renamed gives the same frames."""
    cfg = rebuild_tum(fx, tmp_path)
    os.rename(tmp_path / "groundtruth.txt", tmp_path / "pose.txt")
    ds = P.get_dataset(cfg, None, 1.0, device="cpu")
    assert len(ds) == int(fx["tumrgbd.n"])
    rows = P.datasets.TUM_RGBD.parse_list(str(tmp_path / "pose.txt"), skiprows=1)
    assert rows.shape == (len(tum_scene.SEQ_POSE_T), 8)
    assert P.datasets.TUM_RGBD.parse_list(str(tmp_path / "rgb.txt")).shape == (len(tum_scene.SEQ_COLOR_T), 2)


@pytest.mark.parametrize("shape,scale", [((48, 64, 3), 0.1), ((37, 53, 1), 0.085)])
def test_host_undistort_equals_restatement(shape, scale):
    img = tum_scene.random_u8(*shape, seed=3)
    intr = tum_scene.intrinsics(scale)
    got = P.datasets.undistort_u8(img, *intr, tum_scene.FREIBURG1_DIST)
    want = tum_scene.undistort_u8(img, *intr, tum_scene.FREIBURG1_DIST)
    assert got.dtype == np.uint8 and got.shape == img.shape
    assert np.array_equal(got, want)
    assert not np.array_equal(got, img)
    # zero coefficients: the identity, exactly
    assert np.array_equal(P.datasets.undistort_u8(img, *intr, [0.0] * 5), img)
    assert np.array_equal(tum_scene.undistort_u8(img, *intr, [0.0] * 5), img)
    # a [H, W] image is its [H, W, 1] image
    if shape[2] == 1:
        assert np.array_equal(P.datasets.undistort_u8(img[:, :, 0], *intr, tum_scene.FREIBURG1_DIST), want[:, :, 0])


def test_zero_border_is_exercised():
    """At 48×64 with freiburg1's lens, 257 of the 3072 destination pixels have a tap outside the image."""
    assert tum_scene.taps_outside(48, 64, *tum_scene.intrinsics(0.1), tum_scene.FREIBURG1_DIST) == 257


def test_distortion_length_and_cofusion(fx, tmp_path):
    cfg = rebuild_tum(fx, tmp_path)
    for bad in ([0.1, 0.2, 0.0, 0.0], [0.1] * 8, []):
        cfg["cam"]["distortion"] = bad
        with pytest.raises(ValueError):
            P.get_dataset(cfg, None, 1.0, device="cpu")
    with pytest.raises(ValueError):
        P.datasets.undistort_u8(np.zeros((4, 4, 3), np.uint8), 1.0, 1.0, 0.0, 0.0, [0.0] * 4)
    with pytest.raises(NotImplementedError):
        P.get_dataset({"dataset": "cofusion"}, None, 1.0, device="cpu")


def test_distortion_applies_to_every_dataset_class(tmp_path):
    """cam.distortion no longer raises for any dataset class, and touches the colour image only."""
    from PIL import Image
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / "results")
    img = tum_scene.random_u8(48, 64, 3, seed=5)
    Image.fromarray(img).save(tmp_path / "results" / "frame000000.png")
    os.rename(tmp_path / "results" / "frame000000.png", tmp_path / "results" / "frame000000.jpg")  # (PNG bytes)
    d16 = rng.integers(0, 30000, (48, 64)).astype(np.uint16)
    Image.fromarray(d16).save(tmp_path / "results" / "depth000000.png")
    (tmp_path / "traj.txt").write_text(" ".join(str(float(v)) for v in np.eye(4).ravel()) + "\n")
    cam = dict(tum_scene.SEQ_CAM, crop_edge=0)
    del cam["crop_size"]
    outs = {}
    for dist in (None, tum_scene.FREIBURG1_DIST):
        c = dict(cam)
        if dist is None:
            del c["distortion"]
        ds = P.get_dataset({"dataset": "replica", "data": {"input_folder": str(tmp_path)}, "cam": c}, None, 1.0,
                           device="cpu")
        outs[dist is None] = ds[0]
    assert torch.equal(outs[True][2], outs[False][2])  # depth untouched
    want = tum_scene.undistort_u8(img, *tum_scene.intrinsics(0.1), tum_scene.FREIBURG1_DIST) / 255.
    assert np.array_equal(outs[False][1].numpy(), want)
    assert np.array_equal(outs[True][1].numpy(), img / 255.)


def test_abi_stays_24_and_exports(pkg):
    L = pkg._lib.lib()
    assert L.nslam_abi_version() == pkg._lib.ABI_VERSION == 24
    assert hasattr(L, "nslam_undistort_u8") and hasattr(L, "nslam_cam_grad_step_lr2")


def test_undistort_u8_validates_without_gpu(pkg):
    """A null pointer, aliased images, a negative size, C outside 1..4 or a zero focal length are NSLAM_EINVAL
    before any launch; an empty image is no launch and 0."""
    L = pkg._lib.lib()
    dist = (ctypes.c_double * 5)(*tum_scene.FREIBURG1_DIST)
    ok = dict(src=4096, H=48, W=64, C=3, fx=51.7, fy=51.6, cx=31.8, cy=25.5, dist=dist, dst=8192)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nslam_undistort_u8(a["src"], a["H"], a["W"], a["C"], a["fx"], a["fy"], a["cx"], a["cy"], a["dist"],
                                    a["dst"], None)

    assert call(src=None) == -1
    assert call(dst=None) == -1
    assert call(dist=None) == -1
    assert call(dst=4096) == -1   # src and dst may not alias
    assert call(H=-1) == -1
    assert call(W=-5) == -1
    assert call(C=0) == -1
    assert call(C=5) == -1
    assert call(fx=0.0) == -1
    assert call(fy=float("nan")) == -1
    assert call(H=0) == 0         # an empty image: no launch
    assert call(W=0) == 0
    assert call(H=0, src=None) == -1
    assert call(H=65536, W=65536) == -2  # H*W >= 2^31


def test_cam_grad_step_lr2_validates_without_gpu(pkg):
    """nslam_cam_grad_step_lr2 checks what nslam_cam_grad_step checks (test_abi_cpu.py), before any launch."""
    L = pkg._lib.lib()
    T, T2 = pkg._lib.NslamCamTail, pkg._lib.NslamCamTailLr2
    assert ctypes.sizeof(T2) == ctypes.sizeof(T) + 8
    bufs = (ctypes.c_void_p * 1)(4096)

    def call(tail, c2w=4096, n_parts=1):
        return L.nslam_cam_grad_step_lr2(None if tail is None else ctypes.byref(tail), c2w, bufs, n_parts, 4096, 4096,
                                         10, 4, 4096, 4096, 4096, None)

    def tail(lr_quat=0.0002, before=1, **kw):
        f = dict(cam=4096, exp_avg=4096, exp_avg_sq=4096, step=4096, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-8,
                 ray_loss=4096, n_rays=10, loss_out=4096, best_loss=None, best=None)
        f.update(kw)
        return T2(T(**f), lr_quat, before)

    assert call(None) == -1
    for field in ("cam", "exp_avg", "exp_avg_sq", "step", "loss_out", "ray_loss"):
        assert call(tail(**{field: None})) == -1, field
    assert call(tail(n_rays=-1)) == -1
    assert call(tail(best_loss=4096)) == -1     # a best loss without the best pose
    assert call(tail(), c2w=None) == -1         # the gradient's own checks
    assert call(tail(), n_parts=0) == -1
    assert call(tail(), n_parts=5) == -1
