"""The references of the rendering metrics alone (tests/metrics_cases.py; no device): the twin's filtering against
scipy, closed forms, the pyramid's sides, the wrappers' refusals that need no device — and the float32 floors the
device test's bars are made of (printed: pytest -s)."""
import math

import numpy as np
import pytest
import torch

import metrics_cases as mc


def test_window_sums_to_one_and_is_the_wrappers(pkg):
    g = mc.window()
    assert abs(g.sum() - 1.0) < 1e-15 and np.all(g == g[::-1]) and g.argmax() == 5
    assert abs(float(mc.window(np.float32).astype(np.float64).sum()) - 1.0) < 11 * 2.0 ** -25
    assert list(pkg.ops.ssim_window()) == mc.window(np.float32).tolist()  # the kernel multiplies with these bits
    assert pkg.ops.SSIM_TILE == mc.TILE and pkg.ops.SSIM_WIN == mc.WIN


def test_filtering_matches_scipy():
    from scipy.ndimage import correlate1d
    a = np.random.default_rng(3).random((23, 31))
    g = mc.window()
    full = correlate1d(correlate1d(a, g, axis=1, mode="constant"), g, axis=0, mode="constant")
    assert np.abs(mc.filter2(a, g) - full[5:-5, 5:-5]).max() < 1e-15
    assert mc.filter2(a, g).shape == (13, 21)


def test_constant_images_closed_form():
    a, b, L = 0.25, 0.625, 1.0
    x, y = np.full((1, 20, 17, 1), a), np.full((1, 20, 17, 1), b)
    r = mc.ssim_ref(x, y, L)[0, 0, 0]
    C1 = (0.01 * L) ** 2
    assert abs(r[1] - 1.0) < 1e-12 and abs(r[0] - (2 * a * b + C1) / (a * a + b * b + C1)) < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equal_images_give_exactly_one_at_every_level(dtype):
    x, _ = mc.image_pair("same", 161, 163, 1)
    r = mc.ssim_ref(x[None], x[None], 1.0, 5, dtype)
    assert np.all(r == 1.0)
    assert mc.ms_ssim_from(r[0]) == 1.0


def test_constant_offset_psnr():
    delta = 0.125
    gt = np.random.default_rng(1).random((1, 9, 7, 3)).astype(np.float32) * 0.5
    e = mc.errors_ref(gt + np.float32(delta), gt, clamp=False)
    assert e[0, 1] == 9 * 7 * 3
    assert abs(mc.psnr_from(e[0, 0], e[0, 1]) + 20 * math.log10(delta)) < 1e-5  # (float32 images: 2^-24 relative)
    assert mc.psnr_from(0.0, 5) == float("inf") and math.isnan(mc.psnr_from(0.0, 0))


def test_negative_image_has_negative_cs_and_zero_ms_ssim():
    x, y = mc.image_pair("negative", 161, 161, 1)
    r = mc.ssim_ref(x[None], y[None], 1.0, 5)
    assert r[0, 0, 0, 1] < 0
    assert mc.ms_ssim_from(r[0]) == 0.0


def test_pyramid_sides():
    assert mc.pyramid_sides(161) == [161, 81, 41, 21, 11]
    assert mc.pyramid_sides(176) == [176, 88, 44, 22, 11]
    assert mc.pyramid_sides(160)[-1] == 10  # no window fits: why five levels need sides above 160
    a = np.arange(15.0).reshape(3, 5)
    p = mc.pool2(a)
    assert p.shape == (2, 3) and p[0, 0] == a[0, 0] / 4 and p[1, 1] == (a[1, 1] + a[1, 2] + a[2, 1] + a[2, 2]) / 4


def test_errors_ref_masks_and_clamp():
    color, gt_color, depth, gt_depth = mc.error_case(2, 5, 6, 3, invalid_image=1)
    e0 = mc.errors_ref(color, gt_color, depth, gt_depth, 0)
    e1 = mc.errors_ref(color, gt_color, depth, gt_depth, 1)
    assert e0[0, 1] == 90 and e1[0, 1] == 3 * (gt_depth[0] > 0).sum() and e1[0, 3] == (gt_depth[0] > 0).sum()
    assert e1[1, 1] == 0 and e1[1, 3] == 0 and e1[1, 0] == 0 and e0[1, 0] > 0
    assert mc.errors_ref(color, gt_color, clamp=False)[0, 0] > e0[0, 0]  # the clamp pulls colours towards [0,1]


def test_wrapper_refusals_without_a_device(pkg):
    ops = pkg.ops
    x = torch.zeros(1, 12, 12, 3)
    with pytest.raises(ValueError, match="levels"):
        ops.ssim(x, x, levels=3)
    with pytest.raises(ValueError, match="at least 11"):
        ops.ssim(torch.zeros(1, 10, 12, 3), torch.zeros(1, 10, 12, 3))
    with pytest.raises(ValueError, match="at least 161"):
        ops.ssim(torch.zeros(1, 160, 200, 1), torch.zeros(1, 160, 200, 1), levels=5)
    with pytest.raises(ValueError, match="C = 1 or 3"):
        ops.ssim(torch.zeros(1, 12, 12, 2), torch.zeros(1, 12, 12, 2))
    with pytest.raises(ValueError, match="data_range"):
        ops.ssim(x, x, data_range=0.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ssim(x, x)
    with pytest.raises(ValueError, match="mask"):
        ops.image_errors(x, x, mask="valid")
    with pytest.raises(ValueError, match="pair"):
        ops.image_errors(x, None)
    with pytest.raises(ValueError, match="neither"):
        ops.image_errors()
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.image_errors(x, x)
    # the entry points themselves refuse before any launch
    L = pkg._lib.lib()
    win = ops.ssim_window()
    assert L.nslam_ssim(64, 64, 1, 10, 12, 3, 1.0, win, 1, 64, 64, 1 << 20, None) == -1      # a side below 11
    assert L.nslam_ssim(64, 64, 1, 160, 200, 3, 1.0, win, 5, 64, 64, 1 << 30, None) == -1   # five levels at 160
    assert L.nslam_ssim(64, 64, 1, 12, 12, 2, 1.0, win, 1, 64, 64, 1 << 20, None) == -1      # two channels
    assert L.nslam_ssim(64, 64, 1, 12, 12, 3, 1.0, win, 2, 64, 64, 1 << 20, None) == -1      # two levels
    assert L.nslam_ssim(64, 64, 1, 12, 12, 3, 1.0, None, 1, 64, 64, 1 << 20, None) == -1     # no window
    need = L.nslam_ssim_workspace_size(1, 12, 12, 3, 1)
    assert need > 0 and L.nslam_ssim(64, 64, 1, 12, 12, 3, 1.0, win, 1, 64, 64, need - 1, None) == -3
    assert L.nslam_ssim_workspace_size(1, 10, 12, 3, 1) == 0
    assert L.nslam_image_errors(64, None, None, None, 1, 10, 3, 0, 1, 64, 64, 1 << 20, None) == -1   # half a pair
    assert L.nslam_image_errors(64, 64, None, None, 1, 10, 3, 1, 1, 64, 64, 1 << 20, None) == -1     # mask, no depth
    assert L.nslam_image_errors(64, 64, None, None, 1, 10, 2, 0, 1, 64, 64, 1 << 20, None) == -1     # two channels
    assert L.nslam_image_errors(64, 64, None, None, 1, 10, 3, 0, 1, 64, 64, 8, None) == -3           # short workspace


def test_workspace_holds_the_pyramid_and_the_partials(pkg):
    L = pkg._lib.lib()
    planes = 2 * 3
    a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    need, h, w = 0, 161, 176
    for l in range(5):
        if l:
            h, w = mc.pyramid_sides(h, 2)[1], mc.pyramid_sides(w, 2)[1]
            need += 2 * a256(planes * h * w * 4)
        ty, tx = -(-(h - 10) // mc.TILE), -(-(w - 10) // mc.TILE)
        need += a256(planes * ty * tx * 16)
    assert L.nslam_ssim_workspace_size(2, 161, 176, 3, 5) == need
    assert L.nslam_image_errors_workspace_size(3, 1024 * 1024 + 1) == 3 * 1024 * 32
    assert L.nslam_image_errors_workspace_size(3, 1025) == 3 * 2 * 32


def test_float32_floors_are_printed_and_small():
    """The float32 twin's largest deviation from the float64 twin per output (SSIM mean, CS mean; per level), per
    case of the device test (a shape and an image kind), over the channels: the device test allows 4 x these."""
    for shapes, levels in ((mc.SSIM_SHAPES, 1), (mc.MS_SSIM_SHAPES, 5)):
        for H, W in shapes:
            for C in (1, 3):
                x, y = mc.image_batch(H, W, C)
                _, _, fl = mc.floors(x, y, 1.0, levels)
                for b, kind in enumerate(mc.KINDS):
                    print(f"float32 floor {H}x{W}x{C} levels={levels} {kind:8s}: ssim "
                          + " ".join(f"{v:.1e}" for v in fl[b, :, 0]) + " | cs " + " ".join(f"{v:.1e}" for v in fl[b, :, 1]))
                # float32 arithmetic on O(1) moments whose variances are differences of O(1) terms: 2^-24 relative,
                # over C2 = 9e-4 where the variance vanishes (constant images) — no more than 1e-3 anywhere
                assert np.all(fl < 1e-3)
                assert np.all(fl[mc.KINDS.index("same")] == 0.0)


def test_ordered_sum_ref_is_the_lane_by_lane_tree():
    """tests/ordered_sum_ref.py against a lane-by-lane model of the two spellings of the wave tree: in lane 0 the
    xor butterfly and the shift-down tree add the same operands (a + b and b + a are the same bits), and that is
    wave_tree; group_sum and ordered_sum against their definitions on values whose order of addition matters."""
    import ordered_sum_ref as osr
    rng = np.random.default_rng(1)
    t = rng.standard_normal(256) * 10.0 ** rng.integers(-8, 8, 256)
    xor, down = t[:64].copy(), t[:64].copy()
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        xor = xor + xor[lanes ^ d]
        down = down + down[np.where(lanes + d < 64, lanes + d, lanes)]  # past the wave: the lane's own value
    assert len(set(osr.bits(xor).tolist())) == 1                 # every lane of the butterfly holds the same bits
    assert osr.bits(osr.wave_tree(t[:64])) == osr.bits(xor[0]) == osr.bits(down[0])
    assert osr.bits(osr.wave_tree(t[:64])) != osr.bits(osr.ordered_sum(t[:64]))  # and the order matters here
    w = [osr.wave_tree(t[64 * k:64 * k + 64]) for k in range(4)]
    assert osr.group_sum(t) == ((w[0] + w[1]) + w[2]) + w[3]
    s = 0.0
    for v in t:
        s = s + v
    assert osr.ordered_sum(t) == s and osr.ordered_sum(t[:0]) == 0.0
    assert np.array_equal(osr.ordered_sum(np.stack([t, -t])), np.zeros(256))
