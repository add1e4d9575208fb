"""The visualiser's panel contract on the CPU: the committed plasma table against matplotlib's, the numpy twin's
depth panels against matplotlib's Normalize + Colormap.__call__(bytes=True) bit for bit, its RGB panels against
the stated rule."""
import numpy as np
import pytest

import vis_cases


@pytest.fixture(scope="module")
def vis(pkg):
    return pkg.visualizer


def test_plasma_header_is_matplotlibs_table(vis):
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["plasma"]
    want = cmap(np.arange(256), bytes=True)[:, :3]
    lut = vis.plasma_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(lut, want)


def _mpl_depth(img, vmax):
    import matplotlib
    from matplotlib.colors import Normalize
    with np.errstate(all="ignore"):
        return matplotlib.colormaps["plasma"](Normalize(0, vmax)(img), bytes=True)[..., :3]


@pytest.mark.parametrize("shape", [(5, 7), (24, 32)])
@pytest.mark.parametrize("case", ["edge_case", "zero_case"])
def test_depth_panels_equal_matplotlib(vis, shape, case):
    pytest.importorskip("matplotlib")
    H, W = shape
    gd, gc, d, c = getattr(vis_cases, case)(H, W)
    out = vis.vis_panels_np(gd, gc, d, c)
    assert out.dtype == np.uint8 and out.shape == (2 * H, 3 * W, 3)
    vmax = float(gd.max())
    with np.errstate(invalid="ignore"):
        res = np.abs(gd.astype(np.float64) - d)
    res[gd == 0] = 0.0
    for k, img in enumerate((gd.astype(np.float64), d, res)):
        got = out[:H, k * W:(k + 1) * W]
        want = _mpl_depth(img, vmax)
        assert np.array_equal(got, want), (case, k, np.argwhere((got != want).any(-1))[:5])
    if case == "edge_case":
        lut = vis.plasma_lut()
        gen = out[:H, W:2 * W].reshape(-1, 3)
        assert np.array_equal(gen[3], lut[255]) and np.array_equal(gen[5], lut[255])   # vmax itself, above
        assert np.array_equal(gen[6], [0, 0, 0]) and np.array_equal(gen[7], lut[0])   # NaN, under
        assert np.array_equal(out[1, 2 * W + 2], lut[0])                              # residual where gt depth is 0
    else:
        assert (out[:H] == vis.plasma_lut()[0]).all()


@pytest.mark.parametrize("shape", [(5, 7), (24, 32)])
def test_rgb_panels_follow_the_stated_rule(vis, shape):
    H, W = shape
    gd, gc, d, c = vis_cases.edge_case(H, W)
    out = vis.vis_panels_np(gd, gc, d, c)
    with np.errstate(invalid="ignore"):
        res = np.abs(gc - c)
    res[gd == 0] = 0.0
    for k, img in enumerate((gc, c, res)):
        assert np.array_equal(out[H:, k * W:(k + 1) * W], vis_cases.rgb_rule(img)), k
    # the rule at its named points
    pts = np.array([0.0, 1.0, 3 / 255, 200 / 255, -0.5, 2.0, 0.4 / 255, 0.6 / 255, np.nan], dtype=np.float32)
    assert vis._rgb_np(pts).tolist() == [0, 255, 3, 200, 0, 255, 0, 1, 0]
    assert (out[H + 1, 2 * W + 2] == 0).all()  # colour residual where gt depth is 0 (rendered NaN there)


def test_jpeg_encoding_is_fixed(vis):
    gd, gc, d, c = vis_cases.edge_case(5, 7)
    m = vis.vis_panels_np(gd, gc, d, c)
    a, b = vis.encode_jpeg(m), vis.encode_jpeg(m.copy())
    assert a == b and a[:2] == b"\xff\xd8"
    from PIL import Image
    import io
    assert Image.open(io.BytesIO(a)).size == (21, 10)
