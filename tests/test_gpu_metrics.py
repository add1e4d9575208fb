"""csrc/nslam_metrics.hip on the device against the numpy twins of tests/metrics_cases.py, render_metrics against the
same twins, and tools/eval_render.py end to end on a four-frame run of the synthetic Replica folder.

SSIM / CS means: every output is compared with the float64 twin; the bar per output is 4 x the float32 floor of its
case (tests/test_metrics_cpu.py prints them: the float32 twin's deviation from the float64 twin).  Measured floors
(per case, the largest over the shapes here, at one level / at the later levels of five): noise 2.9e-7 / 3.4e-5; ramp
6.6e-6 / 6.5e-6; y = 1 - x 6.5e-7 / 1.8e-5; two constants 5.8e-5 / 6.0e-5 (a vanishing variance over C2); y = x
exactly 0.  The kernel keeps the twin's float32 order, so at the T+10 shape its means are also held to
the float32 twin's within the float64 summation bound n 2^-52.  Measured on one MI355X: the device's deviation from
the float64 twin equals the floor in every case (the largest 6.0e-5, the constants at 161 x 176 x 3, bar 2.4e-4).
Error sums: against the float64 twin within n 2^-52 relative (summation order only); counts exactly.
"""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_cases as mc
import ordered_sum_ref as osr

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
ops = P.ops
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_against_twin(got, r64, floor, what):
    """got, r64 [B,levels,C,2]; floor [B,levels,2]: every output within 4 x its case's floor."""
    err = np.abs(got - r64)
    bar = 4.0 * floor[:, :, None, :]
    print(f"{what}: largest deviation from the float64 twin {err.max():.2e} (bar there "
          f"{bar.repeat(err.shape[2], 2).ravel()[err.argmax()]:.2e}); per kind "
          + " ".join(f"{k} {err[b].max():.1e}/{4 * floor[b].max():.1e}" for b, k in enumerate(mc.KINDS)))
    assert np.all(err <= bar), (what, err.max())


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", mc.SSIM_SHAPES)
def test_ssim_one_level(H, W, C):
    x, y = mc.image_batch(H, W, C)
    r64, r32, floor = mc.floors(x, y, 1.0, 1)
    dx, dy = dev(x), dev(y)
    out = ops.ssim(dx, dy)
    assert out.shape == (len(mc.KINDS), 1, C, 2) and out.dtype == torch.float64 and out.is_cuda
    got = out.cpu().numpy()
    check_against_twin(got, r64, floor, f"ssim {H}x{W}x{C}")
    same = mc.KINDS.index("same")
    assert np.all(got[same] == 1.0)                       # y = x: exactly 1
    assert torch.equal(ops.ssim(dx, dy), out)             # two calls: the same bits
    for b in range(len(mc.KINDS)):                        # an image of a batch equals its single-image call
        assert torch.equal(ops.ssim(dx[b:b + 1].contiguous(), dy[b:b + 1].contiguous())[0], out[b]), b
    assert torch.equal(ops.ssim(dx[1:4].contiguous(), dy[1:4].contiguous()), out[1:4])  # B = 3
    if (H, W) == (mc.TILE + 10, mc.TILE + 10):
        # the kernel's float32 order is the twin's: only the float64 sums of the (h-10)(w-10) map values differ
        n = (H - 10) * (W - 10)
        assert np.abs(got - r32).max() <= n * 2.0 ** -52 * max(1.0, np.abs(r32).max())


def test_ssim_refuses_small_sides_on_the_device():
    z = torch.zeros(1, 10, 40, 3, device=DEV)
    with pytest.raises(ValueError, match="at least 11"):
        ops.ssim(z, z)
    z = torch.zeros(1, 200, 160, 3, device=DEV)
    with pytest.raises(ValueError, match="at least 161"):
        ops.ssim(z, z, levels=5)
    assert ops.ssim(z, z, levels=1).shape == (1, 1, 3, 2)
    with pytest.raises(TypeError):
        ops.ssim(z.double(), z.double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.ssim(z.permute(0, 2, 1, 3), z.permute(0, 2, 1, 3))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", mc.MS_SSIM_SHAPES)
def test_ssim_five_levels(H, W, C):
    x, y = mc.image_batch(H, W, C)
    r64, r32, floor = mc.floors(x, y, 1.0, 5)
    dx, dy = dev(x), dev(y)
    out = ops.ssim(dx, dy, levels=5)
    assert out.shape == (len(mc.KINDS), 5, C, 2)
    got = out.cpu().numpy()
    check_against_twin(got, r64, floor, f"ms-ssim {H}x{W}x{C}")
    assert np.all(got[mc.KINDS.index("same")] == 1.0)
    assert torch.equal(ops.ssim(dx, dy, levels=5), out)
    assert torch.equal(ops.ssim(dx[:1].contiguous(), dy[:1].contiguous(), levels=5)[0], out[0])
    assert torch.equal(ops.ssim(dx, dy, levels=1)[:, 0], out[:, 0])  # level 1 of five is the one-level call
    neg = mc.KINDS.index("negative")
    assert np.all(got[neg, 0, :, 1] < 0) and mc.ms_ssim_from(got[neg]) == 0.0  # (one negative factor is enough)


def test_ssim_data_range():
    """L = 255 on images scaled by 255 gives the L = 1 result up to float32 rounding of the scaled products."""
    x, y = mc.image_batch(43, 43, 3, kinds=("noise", "ramp"))
    x, y = (x * 255).astype(np.float32), (y * 255).astype(np.float32)
    r64 = mc.ssim_ref(x, y, 255.0, 1)
    r32 = mc.ssim_ref(x, y, 255.0, 1, np.float32)
    got = ops.ssim(dev(x), dev(y), data_range=255.0).cpu().numpy()
    assert np.all(np.abs(got - r64) <= 4 * np.abs(r32 - r64).max(axis=2)[:, :, None, :])


ERR_SHARE_GRID = 1024 * 1024  # a workgroup's share (256 threads x 4 pixels) times the largest grid per image


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n_pix", [1, 255, 256, 257, ERR_SHARE_GRID + 1])
def test_image_errors(n_pix, C):
    B = 2
    color, gt_color, depth, gt_depth = mc.error_case(B, 1, n_pix, C, invalid_image=1 if n_pix > 1 else None)
    d = [dev(a) for a in (color, gt_color, depth, gt_depth)]
    for mode, name in ((0, "none"), (1, "depth")):
        want = mc.errors_ref(color, gt_color, depth, gt_depth, mode)
        out = ops.image_errors(*d, mask=name)
        assert out.shape == (B, 4) and out.dtype == torch.float64 and out.is_cuda
        got = out.cpu().numpy()
        assert np.array_equal(got[:, [1, 3]], want[:, [1, 3]])           # counts: exact
        for k, n in ((0, n_pix * C), (2, n_pix)):
            assert np.all(np.abs(got[:, k] - want[:, k]) <= n * 2.0 ** -52 * want[:, k]), (name, k)
        assert torch.equal(ops.image_errors(*d, mask=name), out)         # two calls: the same bits
    if n_pix > 1:
        assert got[1, 3] == 0 and got[1, 2] == 0 and got[1, 1] == 0      # the image without a valid depth
    # a missing pair leaves its sums 0 and the other pair's unchanged; gt_depth alone may mask the colours
    full = ops.image_errors(*d, mask="depth")
    only_color = ops.image_errors(d[0], d[1], None, d[3], mask="depth")
    assert torch.equal(only_color[:, :2], full[:, :2]) and not only_color[:, 2:].any()
    only_depth = ops.image_errors(None, None, d[2], d[3])
    assert torch.equal(only_depth[:, 2:], full[:, 2:]) and not only_depth[:, :2].any()
    unmasked = ops.image_errors(d[0], d[1])
    assert torch.equal(unmasked[:, :2], ops.image_errors(*d, mask="none")[:, :2])
    # the clamp: colours outside [0,1] count as the clamped value
    raw = mc.errors_ref(color, gt_color, clamp=False)
    got_raw = ops.image_errors(d[0], d[1], clamp=False).cpu().numpy()
    assert np.all(np.abs(got_raw[:, 0] - raw[:, 0]) <= n_pix * C * 2.0 ** -52 * raw[:, 0])
    if n_pix >= 255:
        assert np.all(got_raw[:, 0] > unmasked.cpu().numpy()[:, 0])
    with pytest.raises(ValueError, match="needs gt_depth"):
        ops.image_errors(d[0], d[1], mask="depth")
    with pytest.raises(ValueError, match="differ in shape"):
        ops.image_errors(d[0], d[1], torch.zeros(B, 1, n_pix + 1, device=DEV), torch.zeros(B, 1, n_pix + 1, device=DEV))


def _error_partials(color, gt_color, depth, gt_depth, mode):
    """One image's workgroup partials [blocks, 4] in k_image_errors' order: workgroup b, thread t and pass q take
    pixels (q · blocks + b) · 1024 + j · 256 + t for j = 0..3, channels ascending within a pixel; the term is
    (double)v - (double)gt squared with v clamped in float32.  A pixel that is skipped or past the image adds +0."""
    n_pix, C = color.shape
    blocks = min(-(-n_pix // 1024), 1024)
    passes = -(-n_pix // (blocks * 1024))

    def lay(a):  # [n_pix, ...] -> [passes, blocks, 4, 256, ...], zero past the image
        full = np.zeros((passes * blocks * 1024,) + a.shape[1:])
        full[:n_pix] = a
        return full.reshape((passes, blocks, 4, 256) + a.shape[1:])

    valid = gt_depth > 0
    counted = valid if mode == 1 else np.ones(n_pix, bool)
    d = np.clip(color, np.float32(0), np.float32(1)).astype(np.float64) - gt_color.astype(np.float64)
    sq = lay(np.where(counted[:, None], d * d, 0.0))
    n_col = lay(np.where(counted, float(C), 0.0))
    ad = lay(np.where(valid, np.abs(depth.astype(np.float64) - gt_depth.astype(np.float64)), 0.0))
    n_dep = lay(valid.astype(np.float64))
    acc = np.zeros((4, blocks, 256))
    for q in range(passes):
        for j in range(4):
            acc[2] = acc[2] + ad[q, :, j]
            acc[3] = acc[3] + n_dep[q, :, j]
            for c in range(C):
                acc[0] = acc[0] + sq[q, :, j, :, c]
            acc[1] = acc[1] + n_col[q, :, j]
    return osr.group_sum(acc).T


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n_pix", [1, 257, 64 * 1024, 64 * 1024 + 1, ERR_SHARE_GRID + 1])
def test_image_errors_bits_are_the_ordered_sum(n_pix, C):
    """All four outputs bit for bit: one thread; two waves, one nearly empty; exactly 64 partials; 65 (the ordered
    sum's second round); the second pass of the grid stride with 1024 partials."""
    B = 2
    color, gt_color, depth, gt_depth = mc.error_case(B, 1, n_pix, C, seed=7)
    d = [dev(a) for a in (color, gt_color, depth, gt_depth)]
    for mode, name in ((0, "none"), (1, "depth")):
        got = ops.image_errors(*d, mask=name).cpu().numpy()
        want = np.stack([osr.ordered_sum(_error_partials(color[b].reshape(n_pix, C), gt_color[b].reshape(n_pix, C),
                                                         depth[b].ravel(), gt_depth[b].ravel(), mode))
                         for b in range(B)])
        assert want[0, 3] > 0 or n_pix == 1
        assert np.array_equal(osr.bits(got), osr.bits(want)), (name, got - want)


def _frame(H, W, seed=4):
    """A rendered frame (colours leave [0,1]) and its ground truth as float32 arrays [H,W,3], [H,W]."""
    x, _ = mc.image_pair("ramp", H, W, 3, seed)
    rng = np.random.default_rng(seed)
    color = (x + 0.08 * rng.standard_normal(x.shape)).astype(np.float32)
    _, _, depth, gt_depth = mc.error_case(1, H, W, 3, seed)
    return color, x, depth[0], gt_depth[0]


@pytest.mark.parametrize("H,W", [(96, 128), (161, 176)])
def test_render_metrics_against_the_twins(H, W):
    color, gt_color, depth, gt_depth = _frame(H, W)
    levels = 5 if min(H, W) > 160 else 1
    clamped = np.clip(color, 0, 1)
    r64, r32, floor = mc.floors(clamped[None], gt_color[None], 1.0, levels)
    for mask, mode in (("depth", 1), ("none", 0)):
        m = P.evaluation.render_metrics(dev(color), dev(gt_color), dev(depth).double(), dev(gt_depth), mask=mask)
        e = mc.errors_ref(color[None], gt_color[None], depth[None], gt_depth[None], mode)[0]
        assert abs(m["psnr"] - mc.psnr_from(e[0], e[1])) <= 10 / math.log(10) * e[1] * 2.0 ** -52 + 1e-14
        assert abs(m["depth_l1"] - e[2] / e[3]) <= e[3] * 2.0 ** -52 * e[2] / e[3]
        assert m["valid_depth_pixels"] == e[3]
        assert abs(m["ssim"] - r64[0, 0, :, 0].mean()) <= 4 * floor[0, 0, 0]
        if levels == 1:
            assert m["ms_ssim"] is None
        else:  # d(Π v^w) / Π v^w = Σ w dv / v, each dv within 4 x its floor
            v = np.concatenate([r64[0, :-1, :, 1], r64[0, -1:, :, 0]])
            fl = np.concatenate([floor[0, :-1, 1], floor[0, -1:, 0]])
            rel = (np.asarray(mc.MS_WEIGHTS)[:, None] * 4 * fl[:, None] / v).sum(0).max()
            want = mc.ms_ssim_from(r64[0])
            assert 0 < want < 1 and abs(m["ms_ssim"] - want) <= 1.01 * rel * want
    # numpy arrays and other float types are taken too, and the caller's tensors are left as they were
    dc = dev(color)
    keep = dc.clone()
    assert P.evaluation.render_metrics(dc, gt_color, depth.astype(np.float64), gt_depth, mask="none", device=DEV) == m
    assert torch.equal(dc, keep)


def test_render_metrics_edge_values():
    color, gt_color, depth, gt_depth = _frame(96, 128)
    m = P.evaluation.render_metrics(dev(gt_color), dev(gt_color), dev(gt_depth), dev(gt_depth))
    assert m["psnr"] == float("inf") and m["ssim"] == 1.0 and m["depth_l1"] == 0.0 and m["ms_ssim"] is None
    m = P.evaluation.render_metrics(dev(color), dev(gt_color), dev(depth), dev(np.zeros_like(gt_depth)))
    assert math.isnan(m["psnr"]) and math.isnan(m["depth_l1"]) and m["valid_depth_pixels"] == 0
    assert 0 < m["ssim"] < 1                                    # SSIM has no mask
    m = P.evaluation.render_metrics(dev(color), dev(gt_color), dev(depth), dev(np.zeros_like(gt_depth)), mask="none")
    assert math.isfinite(m["psnr"]) and math.isnan(m["depth_l1"])
    big = np.ascontiguousarray(np.tile(gt_color, (2, 2, 1))[:170, :180])
    assert P.evaluation.render_metrics(dev(big), dev(big), dev(big[:, :, 0]), dev(big[:, :, 0]))["ms_ssim"] == 1.0
    with pytest.raises(ValueError, match="mask"):
        P.evaluation.render_metrics(dev(color), dev(gt_color), dev(depth), dev(gt_depth), mask="all")


# ------------------------------------------------------------------------------------------------
# tools/eval_render.py end to end
# ------------------------------------------------------------------------------------------------
def _eval_tool():
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_render
    return eval_render


def _state(slam):
    return ({k: v.clone() for k, v in slam.shared_c.items()},
            {k: v.clone() for k, v in slam.shared_decoders.state_dict().items()},
            slam.estimate_c2w_list.clone(), slam.gt_c2w_list.clone())


def _same_state(a, b):
    return (all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
            and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]))


def test_eval_render_end_to_end(tmp_path, monkeypatch, tiny):
    import test_gpu_run as run_helpers
    over = {"mapping": {"color_refine": False, "iters_first": 10, "iters": 5, "vis_freq": 50, "ckpt_freq": 50,
                        "mesh_freq": 50},
            "tracking": {"vis_freq": 50}, "meshing": {"resolution": 16}}
    slam, _, _, _ = run_helpers.run_system(tmp_path, monkeypatch, tiny, "render", 4, over, graphs=False)
    before = _state(slam)
    cfg_path, seq, out = str(tmp_path / "configs" / "render.yaml"), str(tmp_path / "seq"), str(tmp_path / "out")
    res = _eval_tool().main([cfg_path, "--input_folder", seq, "--output", out, "--every", "2", "--save_images"])
    torch.cuda.synchronize()
    assert _same_state(before, _state(slam))
    with open(os.path.join(out, "eval_render.json")) as f:
        js = json.load(f)
    assert js["frames"] == [0, 2] and js["every"] == 2 and js["mask"] == "depth" and "lpips" not in js
    assert js["checkpoint"].endswith("00003.tar") and js["args"]["nice"] is True
    H, W = run_helpers.CAM["H"], run_helpers.CAM["W"]
    for j, i in enumerate(js["frames"]):
        _, gt_color, gt_depth, _ = slam.frame_reader[i]
        depth, _, color = slam.renderer.render_img(slam.shared_c, slam.shared_decoders,
                                                   slam.estimate_c2w_list[i].to(DEV), DEV, stage="color",
                                                   gt_depth=gt_depth)
        m = P.evaluation.render_metrics(color, gt_color, depth, gt_depth)
        for k in ("psnr", "ssim", "ms_ssim", "depth_l1"):
            assert js[k][j] == m[k] == res[k][j], (i, k)       # bit for bit (a float survives its JSON form)
        assert m["ms_ssim"] is None and math.isfinite(m["psnr"]) and 0 < m["ssim"] < 1 and m["depth_l1"] > 0
        with Image.open(os.path.join(out, "eval_render", f"{i:05d}.jpg")) as im:
            assert im.size == (2 * W, H) == (256, 96)
    assert sorted(os.listdir(os.path.join(out, "eval_render"))) == ["00000.jpg", "00002.jpg"]
    assert js["mean"]["psnr"] == math.fsum(js["psnr"]) / 2 and js["mean"]["ms_ssim"] is None
    assert js["mean"]["depth_l1_cm"] == js["mean"]["depth_l1"] * 100.0 and js["frames_without_depth"] == 0
    print(f"eval_render on the synthetic run: PSNR {js['mean']['psnr']:.3f} dB, SSIM {js['mean']['ssim']:.4f}, "
          f"depth L1 {js['mean']['depth_l1_cm']:.3f} cm")


def test_eval_render_imap(tmp_path, monkeypatch, tiny):
    import test_gpu_run as run_helpers
    over = {"scale": 1, "mapping": {"iters_first": 6, "iters": 6, "pixels": 400, "ckpt_freq": 50, "mesh_freq": 50,
                                    "vis_freq": 50, "color_refine": False},
            "tracking": {"iters": 3, "pixels": 200, "vis_freq": 50}, "meshing": {"resolution": 16},
            "pretrained_decoders": {"coarse": "nowhere/coarse.pt", "middle_fine": "nowhere/middle_fine.pt"}}
    slam, _, _, _ = run_helpers.run_system(tmp_path, monkeypatch, tiny, "imap_render", 3, over, graphs=False,
                                           nice=False)
    before = _state(slam)
    res = _eval_tool().main([str(tmp_path / "configs" / "imap_render.yaml"), "--input_folder", str(tmp_path / "seq"),
                             "--output", str(tmp_path / "out"), "--every", "2", "--imap"])
    assert _same_state(before, _state(slam))
    assert res["frames"] == [0, 2] and res["args"]["nice"] is False
    assert all(math.isfinite(v) for v in res["psnr"]) and all(0 < v < 1 for v in res["ssim"])
    assert not os.path.exists(str(tmp_path / "out" / "eval_render"))
    print(f"eval_render --imap on the synthetic run: PSNR {res['mean']['psnr']:.3f} dB")
