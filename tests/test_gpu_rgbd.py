"""GPU tests of the odometry's photometric term (csrc/nslam_odometry.hip: nslam_gray_pyramid, nslam_photo_sums;
nice-slam_amd/odometry.py) against the numpy twins of tests/rgbd_cases.py: the grey pyramid bit for bit, the
photometric sums within the project's bound for icp_sums, the tracker on the textured wall and corner, and
tools/prep_own_data.py --photometric end to end.  The tracker is held to twice the float64 twin's error on the
same frames (DESIGN.md §7i's rule: the device fuses and ray-casts in float32)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import odometry_cases as oc
import rgbd_cases as rc
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = oc.CAM
INTR = (K["fx"], K["fy"], K["cx"], K["cy"])
THREADS, MAX_GROUPS = 256, 1024          # csrc/nslam_odometry.hip: kThreads, kMaxGroups


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


@pytest.fixture(scope="module")
def scenes():
    return {s: rc.frames(s) for s in ("wall", "corner")}


@pytest.fixture(scope="module")
def weight(pkg):
    return pkg.odometry.PHOTO_WEIGHT


@pytest.fixture(scope="module")
def twins(scenes, weight):
    """The float64 twin's runs at the default weight, computed once."""
    return {s: rc.track_rgbd_ref(scenes[s], weight) for s in ("wall", "corner")}


# ------------------------------------------------------------------------------------------------
# grey pyramid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [(1, 1), (1, 7), (2, 3), (47, 63), (48, 64)])
def test_gray_pyramid_is_the_float32_twin(pkg, scenes, side):
    H, W = side
    rgb = np.ascontiguousarray(scenes["corner"][2].color[:H, :W])
    for levels in (1, 4, 8):
        got = pkg.ops.gray_pyramid(_dev(rgb, np.uint8), levels)
        want = rc.gray_pyramid_f32(rgb, levels)
        assert len(got) == levels
        for g, w in zip(got, want):
            assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32))
    flat = pkg.ops.gray_pyramid(_dev(np.full((H, W, 3), 200, np.uint8), np.uint8), 4)
    assert all(bool((g == g.flatten()[0]).all()) for g in flat)          # a constant image stays constant


# ------------------------------------------------------------------------------------------------
# photometric sums
# ------------------------------------------------------------------------------------------------
def _maps(frs, k):
    """Source maps of frame k and reference maps of frame k - 1 (float32 twins), with their grey pyramids."""
    return dict(sv=oc.depth_maps_f32(frs[k].depth).vertex, gs=rc.gray_pyramid_f32(frs[k].color, 3),
                rv=oc.depth_maps_f32(frs[k - 1].depth).vertex, gr=rc.gray_pyramid_f32(frs[k - 1].color, 3),
                T=frs[k].c2w, w2c=np.linalg.inv(frs[k - 1].c2w))


def _check(pkg, sv, sg, rg, level, rv, T, w2c, depth_th=oc.DIST_TH, photo_th=rc.PHOTO_OFF, what=""):
    ref = rc.photo_sums_ref(sv, sg, rg, level, rv, T, w2c, depth_th=depth_th, photo_th=photo_th)
    args = (_dev(sv), _dev(sg), _dev(rg), level, _dev(rv), T, w2c, *INTR, depth_th, photo_th)
    got, mask = pkg.ops.photo_sums(*args, return_mask=True)
    again = pkg.ops.photo_sums(*args)
    got, mask = got.cpu().numpy(), mask.cpu().numpy().astype(bool)
    assert np.array_equal(got.view(np.int64), again.cpu().numpy().view(np.int64))       # the same bits
    assert ref.margin.sum() <= rc.MARGIN_CAP * max(ref.n_terms, 100)
    same = bool((mask == ref.accept).all())
    assert same or ((mask == ref.accept) | ref.margin).all()
    assert abs(got[28] - ref.sums[28]) <= ref.margin.sum() and got[28] == mask.sum()
    bound = ref.n_terms * 2.0 ** -52 * ref.abs_sums[:28]
    diff = np.abs(got[:28] - ref.sums[:28])
    print(f"photo_sums {what} level {level}: {int(got[28])} of {ref.n_terms} pixels, {int(ref.margin.sum())} margin "
          f"pixels, same set: {same}, largest difference / bound {float((diff / np.maximum(bound, 1e-300)).max()):.3f}")
    if same:      # the same terms: only the order of the float64 additions differs
        assert (diff <= bound).all(), diff / np.maximum(bound, 1e-300)
    return ref, got


@pytest.mark.parametrize("scene", ["wall", "corner"])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_photo_sums_match_the_twin(pkg, scenes, scene, level):
    m = _maps(scenes[scene], 4)
    ref, got = _check(pkg, m["sv"], m["gs"][level], m["gr"][level], level, m["rv"], m["T"], m["w2c"], what=scene)
    assert got[28] > 0.5 * ref.n_terms
    moved = oc._od().se3_exp([0.012, 0.0, 0.0, 0.02, 0.0, 0.0]) @ m["T"]                # 0.7 degrees and 2 cm
    far, _ = _check(pkg, m["sv"], m["gs"][level], m["gr"][level], level, m["rv"], moved, m["w2c"], what=scene + " moved")
    assert far.sums[27] > ref.sums[27]                 # the true pose has the smaller photometric cost


@pytest.mark.parametrize("level", [0, 1, 2])
def test_photo_sums_at_47x63(pkg, scenes, level):
    fr = scenes["corner"]
    sv, rv = (np.ascontiguousarray(oc.depth_maps_f32(fr[k].depth).vertex[:47, :63]) for k in (4, 3))
    gs, gr = (rc.gray_pyramid_f32(fr[k].color[:47, :63], 3) for k in (4, 3))
    ref, got = _check(pkg, sv, gs[level], gr[level], level, rv, fr[4].c2w, np.linalg.inv(fr[3].c2w), what="47x63")
    assert got[28] > 0.5 * ref.n_terms


@pytest.mark.parametrize("n", [THREADS - 1, THREADS, THREADS + 1, MAX_GROUPS * THREADS + 1])
def test_photo_sums_at_the_launch_edges(pkg, scenes, n):
    """A 1 x n source (the corner frame's pixels, repeated) against the 48 x 64 reference at level 0: one workgroup
    less one, exactly one, one more, and one pixel more than kMaxGroups workgroups take in one pass."""
    m = _maps(scenes["corner"], 4)
    sv = np.resize(m["sv"].reshape(-1, 3), (n, 3)).reshape(1, n, 3)
    sg = np.resize(m["gs"][0].reshape(-1), n).reshape(1, n)
    ref, got = _check(pkg, sv, sg, m["gr"][0], 0, m["rv"], m["T"], m["w2c"], what=f"1 x {n}")
    assert got[28] > 0.5 * n


@pytest.mark.parametrize("case", ["one pixel", "no valid pixel", "1 x N reference", "holes"])
def test_photo_sums_edge_inputs(pkg, scenes, case):
    m = _maps(scenes["corner"], 4)
    sv, sg, rg, rv = m["sv"], m["gs"][0], m["gr"][0], m["rv"]
    if case == "one pixel":
        sv, sg = np.ascontiguousarray(sv[20:21, 30:31]), np.ascontiguousarray(sg[20:21, 30:31])
    elif case == "no valid pixel":
        sv = np.full_like(sv, np.nan)
    elif case == "1 x N reference":
        rg, rv = np.ascontiguousarray(rg[20:21]), np.ascontiguousarray(rv[20:21])
    else:
        sv, rv = sv.copy(), rv.copy()
        sv[5:15, 7:30] = np.nan
        sv[40, 3, 1] = np.nan           # one component alone
        rv[20:30, 25:40] = np.nan
        rv[11, 50, 2] = np.nan
    ref, got = _check(pkg, sv, sg, rg, 0, rv, m["T"], m["w2c"], what=case)
    if case == "one pixel":
        assert got[28] == 1
    elif case == "holes":
        full = rc.photo_sums_ref(m["sv"], sg, rg, 0, m["rv"], m["T"], m["w2c"])
        assert 0 < got[28] < full.sums[28] - 200
    else:
        assert (got == 0).all()


def test_photo_sums_gates(pkg, scenes):
    m = _maps(scenes["corner"], 4)
    sv, sg, rg, rv = m["sv"], m["gs"][0], m["gr"][0], m["rv"]
    full = rc.photo_sums_ref(sv, sg, rg, 0, rv, m["T"], m["w2c"])
    th = float(np.median(np.abs(full.r[full.accept])))
    ref, got = _check(pkg, sv, sg, rg, 0, rv, m["T"], m["w2c"], photo_th=th, what="photo_th")
    assert 0 < got[28] < full.sums[28]
    far = rv.copy()
    far[10:30, 20:40, 2] += np.float32(2.0 * oc.DIST_TH)
    ref, got = _check(pkg, sv, sg, rg, 0, far, m["T"], m["w2c"], what="occluded")
    assert got[28] < full.sums[28] - 200


def test_wrappers_check_their_arguments(pkg, scenes):
    import torch
    m = _maps(scenes["corner"], 4)
    sv, rv, g0, g1 = _dev(m["sv"]), _dev(m["rv"]), _dev(m["gs"][0]), _dev(m["gs"][1])
    tail = (np.eye(4), np.eye(4), *INTR, 0.1, 1e300)
    with pytest.raises(ValueError, match="src_gray"):
        pkg.ops.photo_sums(sv, g0, g1, 1, rv, *tail)              # level 0 where level 1 is expected
    with pytest.raises(TypeError, match="ref_gray"):
        pkg.ops.photo_sums(sv, g1, g1.double(), 1, rv, *tail)
    with pytest.raises(ValueError, match="4x4"):
        pkg.ops.photo_sums(sv, g1, g1, 1, rv, np.eye(3), *tail[1:])
    with pytest.raises(ValueError, match="levels"):
        pkg.ops.gray_pyramid(torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV), 9)
    with pytest.raises(TypeError, match="rgb"):
        pkg.ops.gray_pyramid(torch.zeros(4, 4, 3, device=DEV), 2)


# ------------------------------------------------------------------------------------------------
# the tracker
# ------------------------------------------------------------------------------------------------
def _odometry(pkg, **kw):
    return pkg.odometry.DepthOdometry(K["H"], K["W"], *INTR, oc.L, oc.TRUNC, oc.EXTENT, DEV, oc.DEPTH_TRUNC,
                                      oc.MAX_JUMP, dist_th=oc.DIST_TH, angle_deg=oc.ANGLE_DEG, near=oc.NEAR, **kw)


def _within_twice_the_twin(res, twin, frs, what):
    dt, dr = oc.pose_error(res[-1]["c2w"], frs[-1].c2w)
    tt, tr = oc.pose_error(twin[-1]["c2w"], frs[-1].c2w)
    print(f"{what} final error: device {1e3 * dt:.3f} mm {dr:.4f} deg, float64 twin {1e3 * tt:.3f} mm {tr:.4f} deg; "
          f"photo inliers {res[-1]['photo_inliers']} / {twin[-1]['photo_inliers']}, photo rms "
          f"{res[-1]['photo_rms']:.4f} / {twin[-1]['photo_rms']:.4f}")
    assert dt <= 2.0 * tt and dr <= 2.0 * tr, what


def test_the_wall_is_lost_without_colour_and_tracked_with_it(pkg, scenes, twins, weight):
    frs = scenes["wall"]
    od = _odometry(pkg)
    res = [od.track(f.depth, f.color) for f in frs]
    assert od.lost == list(range(1, len(frs))) and all("photo_inliers" not in r for r in res)
    assert not any(r["lost"] for r in twins["wall"])
    od = _odometry(pkg, photo_weight=weight)
    res = [od.track(f.depth, f.color) for f in frs]
    assert od.lost == [] and od.fused == list(range(len(frs))) and not any(r["lost"] for r in res)
    assert all(r["photo_inliers"] > 0.5 * K["H"] * K["W"] for r in res[1:]) and res[0]["photo_inliers"] == 0
    _within_twice_the_twin(res, twins["wall"], frs, "wall")


def test_the_textured_corner_tracks_within_twice_the_twin(pkg, scenes, twins, weight):
    frs = scenes["corner"]
    od = _odometry(pkg, photo_weight=weight)
    res = [od.track(f.depth, f.color) for f in frs]
    assert od.lost == [] and not any(r["lost"] for r in twins["corner"])
    _within_twice_the_twin(res, twins["corner"], frs, "corner")


def test_weight_zero_is_todays_odometry_bit_for_bit(pkg, scenes):
    frs = scenes["corner"][:6]
    plain = pkg.odometry.DepthOdometry(K["H"], K["W"], *INTR, oc.L, oc.TRUNC, oc.EXTENT, DEV, oc.DEPTH_TRUNC,
                                       oc.MAX_JUMP, dist_th=oc.DIST_TH, angle_deg=oc.ANGLE_DEG, near=oc.NEAR)
    zero = _odometry(pkg, photo_weight=0.0, photo_th=0.05, photo_depth_th=0.01)
    for f in frs:
        a, b = plain.track(f.depth), zero.track(f.depth, f.color)
        assert np.array_equal(a["c2w"].view(np.int64), b["c2w"].view(np.int64))
        assert a["inliers"] == b["inliers"] and a["rms"] == b["rms"] and set(b) == {"c2w", "inliers", "rms", "lost"}
    assert zero._ref is None


def test_a_blank_colour_frame_still_tracks(pkg, scenes, weight):
    """A black colour image with valid depth: against the textured reference nearly every residual is far above
    the gate photo_th = 0.1, so the term falls silent and the depth tracks alone (without a gate the residuals of
    about 0.5 would pull the pose away: the float64 twin loses that frame too).  The next frame meets a reference
    without gradients, which constrains nothing."""
    frs = scenes["corner"]
    od = _odometry(pkg, photo_weight=weight, photo_th=0.1)
    for f in frs[:3]:
        od.track(f.depth, f.color)
    r = od.track(frs[3].depth, np.zeros_like(frs[3].color))
    dt, dr = oc.pose_error(r["c2w"], frs[3].c2w)
    assert not r["lost"] and dt < 0.01 and dr < 0.5 and r["photo_inliers"] < 0.1 * K["H"] * K["W"]
    r = od.track(frs[4].depth, frs[4].color)             # against the blank reference
    dt, dr = oc.pose_error(r["c2w"], frs[4].c2w)
    assert not r["lost"] and dt < 0.01 and dr < 0.5 and od.fused == [0, 1, 2, 3, 4]


def test_the_photometric_odometry_needs_colour(pkg, scenes):
    od = _odometry(pkg, photo_weight=1.0)
    with pytest.raises(ValueError, match="colour"):
        od.track(scenes["wall"][0].depth)
    with pytest.raises(ValueError, match="color"):
        od.track(scenes["wall"][0].depth, scenes["wall"][0].color[:, :32])


# ------------------------------------------------------------------------------------------------
# tools/prep_own_data.py --photometric
# ------------------------------------------------------------------------------------------------
def test_prep_own_data_tracks_the_wall_with_photometric(pkg, scenes, weight, tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("prep_own_data", os.path.join(REPO, "tools", "prep_own_data.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    frs = scenes["wall"]
    folder = tmp_path / "wall"
    os.makedirs(folder / "color")
    os.makedirs(folder / "depth")
    for i, f in enumerate(frs):
        Image.fromarray(f.color).save(str(folder / "color" / f"{i:05d}.jpg"))
        Image.fromarray(np.round(f.depth * 1000.0).astype(np.uint16)).save(str(folder / "depth" / f"{i:05d}.png"))
    (folder / "intrinsic.json").write_text(json.dumps(
        {"width": K["W"], "height": K["H"], "intrinsic_matrix": [K["fx"], 0, 0, 0, K["fy"], 0, K["cx"], K["cy"], 1]}))
    out = tmp_path / "own.yaml"
    argv = ["--scene_folder", str(folder), "--output_config", str(out), "--base",
            os.path.join(GOLDEN, "configs", "own.yaml"), "--voxel", str(oc.L), "--trunc", str(oc.TRUNC), "--extent",
            str(oc.EXTENT), "--fuse_every", "1", "--depth_trunc", "20"]
    assert tool.main(argv + ["--photometric"]) == 0
    log = folder / "scene" / "trajectory.log"
    lines = log.read_text().splitlines()
    assert len(lines) == 5 * len(frs)
    last = np.array([[float(x) for x in row.split()] for row in lines[-4:]])
    # the twin on the images as the tool decodes them
    decoded = [rc.SimpleNamespace(depth=pkg.datasets._read_depth(str(folder / "depth" / f"{i:05d}.png")).astype(np.float32)
                                  / np.float32(1000.0),
                                  color=pkg.datasets._read_color(str(folder / "color" / f"{i:05d}.jpg")), c2w=f.c2w)
               for i, f in enumerate(frs)]
    twin = rc.track_rgbd_ref(decoded, weight)
    assert not any(r["lost"] for r in twin)
    err = float(np.linalg.norm(last[:3, 3] - frs[-1].c2w[:3, 3]))
    twin_err = float(np.linalg.norm(twin[-1]["c2w"][:3, 3] - frs[-1].c2w[:3, 3]))
    print(f"prep_own_data --photometric: final position error {1e3 * err:.3f} mm, float64 twin {1e3 * twin_err:.3f} mm")
    assert err <= 2.0 * twin_err
    assert tool.main(argv + ["--force"]) == 2            # depth alone: every later frame is lost
