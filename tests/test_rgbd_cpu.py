"""CPU tests of the odometry's photometric term: the numpy twins of tests/rgbd_cases.py against restatements and
finite differences, the scenes' conditions, the photo_weight sweep behind odometry.PHOTO_WEIGHT and
the entry points' argument checks (which return before any device call)."""
import ctypes
import math

import numpy as np
import pytest

import odometry_cases as oc
import rgbd_cases as rc

SIDES = [(1, 1), (1, 7), (2, 3), (47, 63), (48, 64)]


@pytest.fixture(scope="module")
def scenes():
    return {s: rc.frames(s) for s in ("wall", "corner")}


# ------------------------------------------------------------------------------------------------
# grey pyramid
# ------------------------------------------------------------------------------------------------
def _pyramid_loops(rgb, levels):
    """nslam_gray_pyramid restated pixel by pixel with float32 scalars."""
    f = np.float32
    H, W = rgb.shape[:2]
    g = np.empty((H, W), f)
    for y in range(H):
        for x in range(W):
            r, gg, b = (f(v) for v in rgb[y, x])
            g[y, x] = ((f(0.299) * r + f(0.587) * gg) + f(0.114) * b) / f(255.0)
    out = [g]
    for _ in range(1, levels):
        g = out[-1]
        h, w = g.shape
        nxt = np.empty(((h + 1) // 2, (w + 1) // 2), f)
        for j in range(nxt.shape[0]):
            for i in range(nxt.shape[1]):
                rows = []
                for y in (max(2 * j - 1, 0), 2 * j, min(2 * j + 1, h - 1)):
                    a, b, c = g[y, max(2 * i - 1, 0)], g[y, 2 * i], g[y, min(2 * i + 1, w - 1)]
                    rows.append((f(0.25) * a + f(0.5) * b) + f(0.25) * c)
                nxt[j, i] = (f(0.25) * rows[0] + f(0.5) * rows[1]) + f(0.25) * rows[2]
        out.append(nxt)
    return out


@pytest.mark.parametrize("side", SIDES)
def test_gray_pyramid_twin_is_the_plain_loops(scenes, side):
    H, W = side
    rgb = scenes["corner"][2].color[:H, :W]
    levels = 4
    got, want = rc.gray_pyramid_f32(rgb, levels), _pyramid_loops(rgb, levels)
    h, w = H, W
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and a.shape == (h, w) and np.array_equal(a, b)
        h, w = (h + 1) // 2, (w + 1) // 2
    flat = np.full((H, W, 3), 200, np.uint8)
    for lvl in rc.gray_pyramid_f32(flat, levels):
        assert (lvl == lvl.flat[0]).all()      # 1/4 + 1/2 + 1/4 of one value is that value in float32


def test_level_pixels_are_the_strided_pixels():
    """Level l of an H x W image has the sh x sw pixels icp_sums visits at stride 2^l."""
    for H, W in SIDES:
        pyr = rc.gray_pyramid_f32(np.zeros((H, W, 3), np.uint8), 4)
        for lvl, g in enumerate(pyr):
            assert g.shape == (len(range(0, H, 1 << lvl)), len(range(0, W, 1 << lvl)))


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def test_the_wall_camera_sees_the_wall_only(scenes):
    assert rc.shortest_wavelength() >= 0.4
    for f in scenes["wall"]:
        pts = rc.hit_points(f.depth, f.world)
        assert (f.depth > 0).all() and np.abs(pts[..., 0] + 1.0).max() < 1e-5     # float32 depths of the plane x = -1
    for s in ("wall", "corner"):
        g = rc.gray_pyramid_f32(scenes[s][0].color, 3)[2]
        assert g.std() > 0.05, s                                                  # the texture survives level 2


def test_depth_alone_loses_every_wall_frame(scenes):
    res = oc.track_ref(scenes["wall"])
    for k, r in enumerate(res[1:], 1):
        assert r["lost"] and r["cond"] > 1.0e4, k
    print("wall, depth only: condition numbers", ", ".join(f"{r['cond']:.3g}" for r in res[1:]))


# ------------------------------------------------------------------------------------------------
# photometric sums
# ------------------------------------------------------------------------------------------------
def _pair(frs, k):
    """Source maps of frame k, reference maps of frame k - 1, both with their grey pyramids."""
    sv = oc.depth_maps_f32(frs[k].depth).vertex
    rv = oc.depth_maps_f32(frs[k - 1].depth).vertex
    return sv, rc.gray_pyramid_f32(frs[k].color, 3), rv, rc.gray_pyramid_f32(frs[k - 1].color, 3)


@pytest.mark.parametrize("scene", ["wall", "corner"])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_the_jacobian_is_the_gradient_of_the_cost(scenes, scene, level):
    """J^T r against the central difference of 1/2 sum r^2 over the twist of T <- exp(xi) T, on the pixels that stay
    in their bilinear cell (the interpolant has a kink at cell borders) and are accepted at all three poses.

    The bound: with h = 1e-6 the difference quotient carries rounding of about 2^-52 C / h (C = the cost, at most
    a few units) = 1e-9 and truncation h^2 / 6 times a third derivative of the order |g| (f |p|)^2 with f = 30:
    1e-8 |g|.  1e-7 max(1, |g|) covers both."""
    od = oc._od()
    frs = scenes[scene]
    sv, gs, rv, gr = _pair(frs, 4)
    w2c = np.linalg.inv(frs[3].c2w)
    T = od.se3_exp([0.003, -0.002, 0.004, 0.005, -0.004, 0.003]) @ frs[4].c2w

    def at(T):
        return rc.photo_sums_ref(sv, gs[level], gr[level], level, rv, T, w2c)

    base = at(T)
    h = 1e-6
    steps = [(at(od.se3_exp(h * e) @ T), at(od.se3_exp(-h * e) @ T)) for e in np.eye(6)]
    keep = base.accept & ~base.margin
    for plus, minus in steps:
        keep &= plus.accept & minus.accept & ~plus.margin & ~minus.margin
    assert keep.sum() > 0.5 * base.accept.sum() > 50
    g = (base.J[keep] * base.r[keep][:, None]).sum(0)
    fd = np.array([(0.5 * (p.r[keep] ** 2).sum() - 0.5 * (m.r[keep] ** 2).sum()) / (2.0 * h) for p, m in steps])
    err = np.abs(g - fd).max()
    print(f"{scene} level {level}: {int(keep.sum())} pixels, |g| {np.abs(g).max():.3e}, |J^T r - fd| {err:.3e}")
    assert err <= 1e-7 * max(1.0, np.abs(g).max())


def test_margins_stay_under_their_cap(scenes):
    od = oc._od()
    moved = od.se3_exp([0.012, 0.0, 0.0, 0.02, 0.0, 0.0])
    for scene in ("wall", "corner"):
        frs = scenes[scene]
        for k in (1, 4, 9):
            sv, gs, rv, gr = _pair(frs, k)
            for level in (0, 1, 2):
                for T in (frs[k].c2w, moved @ frs[k].c2w):
                    r = rc.photo_sums_ref(sv, gs[level], gr[level], level, rv, T, np.linalg.inv(frs[k - 1].c2w))
                    assert r.margin.sum() <= rc.MARGIN_CAP * max(r.n_terms, 100), (scene, k, level)
                    assert r.sums[28] == r.accept.sum() > 0.5 * r.n_terms


def test_gates_of_the_twin(scenes):
    frs = scenes["corner"]
    sv, gs, rv, gr = _pair(frs, 4)
    w2c = np.linalg.inv(frs[3].c2w)
    full = rc.photo_sums_ref(sv, gs[0], gr[0], 0, rv, frs[4].c2w, w2c)
    th = float(np.median(np.abs(full.r[full.accept])))
    gated = rc.photo_sums_ref(sv, gs[0], gr[0], 0, rv, frs[4].c2w, w2c, photo_th=th)
    assert 0 < gated.accept.sum() < full.accept.sum() and (np.abs(gated.r[gated.accept]) <= th).all()
    far = rv.copy()
    far[10:30, 20:40, 2] += np.float32(2.0 * oc.DIST_TH)
    occluded = rc.photo_sums_ref(sv, gs[0], gr[0], 0, far, frs[4].c2w, w2c)
    assert occluded.accept.sum() < full.accept.sum() - 200
    thin = rc.photo_sums_ref(sv[:1], gs[0][:1], gr[0][:1], 0, rv[:1], frs[4].c2w, w2c)      # a 1 x N reference level
    assert not thin.accept.any() and (thin.sums == 0).all()


# ------------------------------------------------------------------------------------------------
# the sweep behind the default weight
# ------------------------------------------------------------------------------------------------
def test_photo_weight_sweep_and_the_default(pkg, scenes):
    """The decades of rgbd_cases.SWEEP on the float64 twin over both scenes: the default is the weight with the
    smallest corner drift among those that track the wall (DESIGN.md §7k holds this table)."""
    rows = []
    for w in rc.SWEEP:
        row = {"w": w}
        for s in ("wall", "corner"):
            res = rc.track_rgbd_ref(scenes[s], w)
            dt, dr = rc.drift(res, scenes[s])
            row[s] = dict(lost=[i for i, r in enumerate(res) if r["lost"]], cond=max(r["cond"] for r in res),
                          mm=1e3 * dt, deg=dr)
            print(f"photo_weight {w:g} {s}: lost {row[s]['lost']}, largest cond {row[s]['cond']:.1f}, "
                  f"drift {row[s]['mm']:.3f} mm {dr:.4f} deg")
        rows.append(row)
    tracked = [r for r in rows if not r["wall"]["lost"] and not r["corner"]["lost"]]
    assert tracked
    best = min(tracked, key=lambda r: r["corner"]["mm"])
    assert pkg.odometry.PHOTO_WEIGHT == best["w"]
    assert best["wall"]["cond"] < 1.0e4 and best["wall"]["mm"] < 10.0


# ------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------
def test_gray_pyramid_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    assert L.nslam_gray_pyramid_size(48, 64, 3) == 48 * 64 + 24 * 32 + 12 * 16
    assert L.nslam_gray_pyramid_size(47, 63, 3) == 47 * 63 + 24 * 32 + 12 * 16
    assert L.nslam_gray_pyramid_size(1, 7, 8) == 7 + 4 + 2 + 1 * 5
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, 9)):
        assert L.nslam_gray_pyramid_size(*bad) == 0
    assert L.nslam_gray_pyramid(None, 4, 4, 1, 4096, None) == -1
    assert L.nslam_gray_pyramid(4096, 4, 4, 1, None, None) == -1
    assert L.nslam_gray_pyramid(4096, 0, 4, 1, 4096, None) == -1
    assert L.nslam_gray_pyramid(4096, 4, 4, 0, 4096, None) == -1
    assert L.nslam_gray_pyramid(4096, 4, 4, 9, 4096, None) == -1
    assert L.nslam_gray_pyramid(4096, 1 << 15, 1 << 15, 1, 4096, None) == -2


def test_photo_sums_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    nan = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    nan[3] = math.nan
    groups = L.nslam_icp_partials(48, 64, 2)

    def call(**kw):
        a = dict(sv=4096, Hs=48, Ws=64, sg=4096, sh=24, sw=32, rg=4096, rh=24, rw=32, level=1, rv=4096, Hr=48, Wr=64,
                 T=eye, M=eye, fx=30.0, fy=30.0, cx=31.5, cy=23.5, dth=0.1, pth=1e300, partial=4096, n=groups,
                 out=4096, mask=None)
        a.update(kw)
        return L.nslam_photo_sums(a["sv"], a["Hs"], a["Ws"], a["sg"], a["sh"], a["sw"], a["rg"], a["rh"], a["rw"],
                                  a["level"], a["rv"], a["Hr"], a["Wr"], a["T"], a["M"], a["fx"], a["fy"], a["cx"],
                                  a["cy"], a["dth"], a["pth"], a["partial"], a["n"], a["out"], a["mask"], None)

    for name in ("sv", "sg", "rg", "rv", "T", "M", "partial", "out"):
        assert call(**{name: None}) == -1, name
    for kw in (dict(Hs=0), dict(Wr=0), dict(level=-1), dict(level=8), dict(sh=23), dict(sw=33), dict(rh=25),
               dict(rw=31), dict(fx=0.0), dict(fy=0.0), dict(cx=math.inf), dict(dth=-1.0), dict(pth=-1.0),
               dict(pth=math.nan), dict(T=nan), dict(M=nan)):
        assert call(**kw) == -1, kw
    assert call(level=0, sh=48, sw=64, rh=48, rw=64, n=L.nslam_icp_partials(48, 64, 1) - 1) == -3
    assert call(n=groups - 1) == -3
    assert call(Hs=1 << 15, Ws=1 << 15, sh=1 << 14, sw=1 << 14) == -2


def test_wrappers_and_constructor_check_their_arguments(pkg):
    import torch
    ops = pkg.ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gray_pyramid(torch.zeros(4, 4, 3, dtype=torch.uint8), 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.photo_sums(torch.zeros(4, 4, 3), torch.zeros(4, 4), torch.zeros(4, 4), 0, torch.zeros(4, 4, 3), np.eye(4),
                       np.eye(4), 30.0, 30.0, 1.5, 1.5, 0.1, 1e300)
    with pytest.raises(ValueError, match="level"):
        ops.photo_sums(None, None, None, 8, None, np.eye(4), np.eye(4), 30.0, 30.0, 1.5, 1.5, 0.1, 1e300)
    args = (48, 64, 30.0, 30.0, 31.5, 23.5, oc.L, oc.TRUNC, oc.EXTENT, "cpu", oc.DEPTH_TRUNC, oc.MAX_JUMP)
    with pytest.raises(ValueError, match="power of two"):
        pkg.odometry.DepthOdometry(*args, strides=(3, 1), iters=(2, 2), photo_weight=1.0)
    with pytest.raises(ValueError, match="photo_weight"):
        pkg.odometry.DepthOdometry(*args, photo_weight=-1.0)
    with pytest.raises(ValueError, match="photo_th"):
        pkg.odometry.DepthOdometry(*args, photo_weight=1.0, photo_th=-0.1)
    g, p = np.arange(29.0), np.ones(29)
    c = pkg.odometry.combine_sums(g, p, 0.5)
    assert np.array_equal(c[:28], g[:28] + 0.5) and c[28] == 28.0 and np.array_equal(c, rc.combine(g, p, 0.5))
