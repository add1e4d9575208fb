"""GPU tests of the depth-L1 metric (csrc/nslam_raster.hip, nslam_views_see_any / nslam_depth_l1 in
csrc/nslam_eval.hip, evaluation.calc_depth_l1): the rasteriser against a float64 brute-force ray caster, its paths
against each other bit for bit, degenerate input, the view rejection against nslam_frustum_seen, the per-view error
against torch's float64 mean, the view sampler, and the metric end to end.  Only the seeded scenes of
tests/golden/raster_scene.py and eval_scene.py are read: never the reference, never scipy, trimesh or open3d."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

DEV = "cuda:0"


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the shared reference stays read-only
    return t if dtype is None else t.to(dtype)


def _w2c(c2w):
    return _t(np.linalg.inv(c2w)[:, :3, :].copy())


def _render(pkg, v, f, c2w, **kw):
    import raster_scene as R
    return pkg.ops.render_depth(_t(v), _t(f), _w2c(c2w), R.CAM["H"], R.CAM["W"], R.CAM["fx"], R.CAM["fy"], R.CAM["cx"],
                                R.CAM["cy"], R.Z_NEAR, R.Z_FAR, **kw)


@pytest.fixture(scope="module")
def ref():
    """The scene, its views and the oracle's images, computed once and left unchanged."""
    import raster_scene as R
    v, f = R.scene()
    c2w = R.views()
    lo, hi, dec = zip(*(R.oracle(v, f, m) for m in c2w))
    out = dict(v=v, f=f, c2w=c2w, lo=np.stack(lo), hi=np.stack(hi), decided=np.stack(dec))
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def image(pkg, ref):
    return _render(pkg, ref["v"], ref["f"], ref["c2w"])


# ------------------------------------------------------------------------------------------------
# the rasteriser
# ------------------------------------------------------------------------------------------------
def test_scene_is_the_one_described(ref):
    import raster_scene as R
    assert ref["v"].shape == (68, 3) and ref["f"].shape == (122, 3)
    assert [int((m == 0).sum()) for m in ref["lo"]] == [802, 2160, 1002, 383, 0, 0]
    near = ref["lo"][1]
    assert abs(near[near > 0].min() - 0.1013) < 1e-4 and near[near > 0].min() > R.Z_NEAR
    assert ref["lo"][2].max() <= R.Z_FAR and ref["lo"][2].max() > R.Z_FAR - 0.01


def test_depth_matches_ray_caster(image, ref):
    """Decided pixels (the casters with edge tolerance +1e-6 and -1e-6 agree to 1e-9) within 2 float32 ulps of
    the oracle cast to float32 — the float64 intersection error is far below half an ulp, the rounding can land
    on either side of a boundary, one ulp of margin; undecided pixels equal to one of the two casters under the
    same rule; at most 1 % undecided."""
    import torch

    import raster_scene as R
    assert image.dtype == torch.float32 and tuple(image.shape) == (6, R.CAM["H"], R.CAM["W"])
    got = image.cpu().numpy()
    for b in range(6):
        und, worst, neither = R.check_image(got[b], ref["lo"][b], ref["hi"][b], ref["decided"][b])
        bg = int((got[b] == 0).sum())
        print(f"view {b}: undecided {und}, worst ulp distance {worst}, matching neither {neither}, background {bg}")
        assert und <= R.MAX_UNDECIDED * got[b].size
        assert worst <= 2
        assert neither == 0
    # background is exactly 0, and every hit lies in (z_near, z_far]
    assert bool(((image == 0) | ((image > R.Z_NEAR) & (image <= R.Z_FAR))).all())


def test_paths_give_the_same_bits(pkg, image, ref):
    """Everything through the list, everything inline, the default, and a list of one item (the overflow path:
    the producer draws what does not fit), each twice: the same bits."""
    import torch
    ops = pkg.ops
    hw = image.shape[1] * image.shape[2]
    one = ops.raster_workspace(1, DEV)
    assert one.numel() == pkg._lib.lib().nslam_raster_workspace_size(1)
    big_ws = ops.raster_workspace(1 << 16, DEV)
    for name, kw in (("list", dict(small_max_pixels=0, ws=big_ws)), ("inline", dict(small_max_pixels=hw)),
                     ("inline+", dict(small_max_pixels=hw + 7)), ("default", dict()),
                     ("overflow", dict(small_max_pixels=0, ws=one))):
        for rep in range(2):
            got = _render(pkg, ref["v"], ref["f"], ref["c2w"], **kw)
            assert torch.equal(got.view(torch.int32), image.view(torch.int32)), (name, rep)
        if name == "list":      # every (face, view) with a pixel box went to the list, and it held them all
            n = ops.raster_list_length(big_ws)
            print("listed items", n)
            assert 6 * 12 < n <= 6 * 122
        if name == "overflow":
            assert ops.raster_list_length(one) > 1


def test_single_views_equal_the_batch(pkg, image, ref):
    import torch
    for b in (1, 4):
        got = _render(pkg, ref["v"], ref["f"], ref["c2w"][b:b + 1])
        assert torch.equal(got[0].view(torch.int32), image[b].view(torch.int32))
    # a 4x4 world-to-camera matrix is taken as well as its 3x4 part
    import raster_scene as R
    full = _t(np.linalg.inv(ref["c2w"]))
    got = pkg.ops.render_depth(_t(ref["v"]), _t(ref["f"]), full, R.CAM["H"], R.CAM["W"], R.CAM["fx"], R.CAM["fy"],
                               R.CAM["cx"], R.CAM["cy"], R.Z_NEAR, R.Z_FAR)
    assert torch.equal(got.view(torch.int32), image.view(torch.int32))


def test_degenerate_faces_draw_nothing(pkg, image, ref):
    import torch

    import raster_scene as R
    v, f = R.degenerate_scene()
    assert len(f) == len(ref["f"]) + 4 and np.isnan(v).any()
    for kw in (dict(), dict(small_max_pixels=0)):
        got = _render(pkg, v, f, ref["c2w"], **kw)
        assert torch.equal(got.view(torch.int32), image.view(torch.int32))


def test_huge_coordinates_and_a_nan_view(pkg, image, ref):
    """A face with coordinates of 1e150 (its edge functions overflow) and a view whose matrix holds NaN: the pixel
    boxes stay inside the image, the first draws nothing, the second is all background."""
    import torch

    import raster_scene as R
    n = len(ref["v"])
    v = np.concatenate([ref["v"], [[1e150, 0.0, 0.0], [0.0, 1e150, 0.0], [0.0, 0.0, -1e150]]], 0)
    f = np.concatenate([ref["f"], [[n, n + 1, n + 2]]], 0).astype(np.int32)
    w2c = np.linalg.inv(ref["c2w"])[:, :3, :]
    bad = w2c[:1].copy()
    bad[0, 1, 2] = np.nan
    far = w2c[:1].copy()
    far[0, :, 3] = 1e300                                         # every vertex lands at 1e300: nothing in range
    for kw in (dict(), dict(small_max_pixels=0)):
        got = pkg.ops.render_depth(_t(v), _t(f), _t(np.concatenate([w2c, bad, far], 0)), R.CAM["H"], R.CAM["W"],
                                   R.CAM["fx"], R.CAM["fy"], R.CAM["cx"], R.CAM["cy"], R.Z_NEAR, R.Z_FAR, **kw)
        assert torch.equal(got[:6].view(torch.int32), image.view(torch.int32))
        assert float(got[6:].abs().max()) == 0.0


def test_empty_work(pkg, ref):
    import torch
    none = _render(pkg, ref["v"], ref["f"], ref["c2w"][:0])
    assert tuple(none.shape) == (0, 48, 64) and none.dtype == torch.float32
    flat = _render(pkg, ref["v"], ref["f"][:0], ref["c2w"])
    assert tuple(flat.shape) == (6, 48, 64) and float(flat.abs().max()) == 0.0
    with pytest.raises(ValueError, match="past"):
        _render(pkg, ref["v"][:60], ref["f"], ref["c2w"])


# ------------------------------------------------------------------------------------------------
# view rejection and the per-view error
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [1, 9])
def test_views_see_any_is_frustum_seen(pkg, n_views):
    import torch

    import eval_scene
    pts, poses = eval_scene.cull_scene()
    cam = eval_scene.CAM
    args = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    w2c = _t(np.stack([np.linalg.inv(p).astype(np.float32) for p in poses[:n_views]], 0))
    # the whole cloud, a part no view sees, and single points: some views see them and some do not
    p_all = _t(pts)
    seen_by = torch.stack([pkg.ops.frustum_seen(p_all, w2c[b:b + 1], *args) for b in range(n_views)])
    clouds = [p_all, p_all[~seen_by.any(0)].contiguous(), p_all[:1].contiguous(), p_all[5:6].contiguous(),
              p_all[:300].contiguous(), p_all[:0].contiguous()]
    verdicts = set()
    for cloud in clouds:
        got = pkg.ops.views_see_any(cloud, w2c, *args)
        assert got.dtype == torch.bool and tuple(got.shape) == (n_views,)
        for b in range(n_views):
            want = bool(pkg.ops.frustum_seen(cloud, w2c[b:b + 1], *args).any())
            assert bool(got[b]) == want, (cloud.shape, b)
            verdicts.add(want)
    assert verdicts == {True, False}


def test_depth_l1_matches_torch(pkg, image):
    import torch
    g = torch.Generator().manual_seed(3)
    other = (image.cpu() + 0.05 * torch.rand(image.shape, generator=g)).to(DEV).contiguous()
    other[0] = 0.0                                              # one view of all background against a rendering
    got = pkg.ops.depth_l1(image, other)
    want = (image.double() - other.double()).abs().reshape(6, -1).mean(1)
    print("depth_l1", got.tolist(), "max rel", float(((got - want).abs() / want).max()))
    assert got.dtype == torch.float64 and tuple(got.shape) == (6,)
    assert bool(((got - want).abs() <= 1e-12 * want).all())
    assert float(got[0]) == float(image[0].double().mean())
    assert float(pkg.ops.depth_l1(image, image).abs().max()) == 0.0
    again = pkg.ops.depth_l1(image, other)
    assert torch.equal(again, got)
    odd = pkg.ops.depth_l1(image[:, :7, :9].contiguous(), other[:, :7, :9].contiguous())  # 63 pixels: one short wave
    want = (image[:, :7, :9].double() - other[:, :7, :9].double()).abs().reshape(6, -1).mean(1)
    assert bool(((odd - want).abs() <= 1e-12 * want).all())


@pytest.mark.parametrize("n_pix", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_depth_l1_bits_are_the_ordered_sum(pkg, n_pix):
    """Bit for bit in k_depth_l1's order: thread t adds pixels t, t + 256, ..., the workgroup's sum is
    csrc/nslam_reduce.h's, and the total is divided by n_pix in float64."""
    import ordered_sum_ref as osr
    rng = np.random.default_rng([5, n_pix])
    a = (rng.random((3, 1, n_pix)) * 4.0).astype(np.float32)
    b = (a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32)
    got = pkg.ops.depth_l1(_t(a), _t(b)).cpu().numpy()
    rounds = -(-n_pix // 256)
    terms = np.zeros((3, rounds * 256))                          # a thread past the image adds nothing: +0
    terms[:, :n_pix] = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(3, n_pix)
    per_thread = osr.thread_sum(terms.reshape(3, rounds, 256).transpose(1, 0, 2))
    want = osr.group_sum(per_thread) / float(n_pix)
    assert want.min() > 0
    assert np.array_equal(osr.bits(got), osr.bits(want)), got - want


# ------------------------------------------------------------------------------------------------
# the view sampler
# ------------------------------------------------------------------------------------------------
CAM_BOX = (np.array([0.6, 1.5, 2.0]), np.array([[0.0, 0.0, 1.0, 2.0], [0.0, 1.0, 0.0, 1.5], [-1.0, 0.0, 0.0, 1.25],
                                                [0.0, 0.0, 0.0, 1.0]]))


def _unseen_cloud():
    """Points on a patch of the x = 4 plane (the open wall): a good share of the views see some of them."""
    g = np.random.default_rng(5)
    p = g.random((200, 3)) * np.array([0.0, 1.0, 0.8]) + np.array([4.0, 1.0, 0.8])
    return p


def test_sample_views(pkg):
    import eval_scene
    E = pkg.evaluation
    cam = eval_scene.CAM
    kw = dict(H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])
    ext, tr = CAM_BOX
    pc = _unseen_cloud()
    views = E.sample_views(12, ext, tr, pc, 7, **kw)
    assert views.dtype == np.float64 and views.shape == (12, 4, 4)
    for batch in (1, 5, 1000):                                   # the seed alone decides, not the batch size
        assert np.array_equal(E.sample_views(12, ext, tr, pc, 7, batch=batch, **kw), views)
    assert not np.array_equal(E.sample_views(12, ext, tr, pc, 8, **kw), views)
    free = E.sample_views(12, ext, tr, np.zeros((0, 3)), 7, **kw)
    assert not np.array_equal(free, views)                       # the rejection rejected something
    assert np.array_equal(E.sample_views(5, ext, tr, None, 7, **kw), free[:5])
    for m in (views, free):
        local = (m[:, :3, 3] - tr[:3, 3]) @ tr[:3, :3]           # back into the box's frame
        assert (np.abs(local) <= ext / 2 + 1e-12).all()
        r = m[:, :3, :3]
        assert np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
        assert np.abs(np.linalg.det(r) - 1.0).max() < 1e-12
        assert np.array_equal(m[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(m), 1)))
    # z = normalised(target - origin), the target drawn from the stream
    u = np.stack([eval_scene.uniforms(7, 64, k) for k in range(6)], 1)
    origin = ((u[:, :3] - 0.5) * ext) @ tr[:3, :3].T + tr[:3, 3]
    target = np.round(u[:, 3:] * 20000.0 - 10000.0, 2)
    z = (target - origin) / np.linalg.norm(target - origin, axis=1, keepdims=True)
    assert np.abs(free[:, :3, 3] - origin[:12]).max() < 1e-12 and np.abs(free[:, :3, 2] - z[:12]).max() < 1e-12
    # no unseen point is visible in any returned view, by nslam_frustum_seen on check_proj's matrices
    flip = views.copy()
    flip[:, :3, 1] *= -1.0
    flip[:, :3, 2] *= -1.0
    w2c = _t(np.linalg.inv(flip).astype(np.float32))
    assert not bool(pkg.ops.frustum_seen(_t(pc), w2c, *[kw[k] for k in ("H", "W", "fx", "fy", "cx", "cy")]).any())


def test_sample_views_gives_up(pkg):
    import eval_scene
    cam = eval_scene.CAM
    ext, tr = CAM_BOX
    g = np.random.default_rng(9)
    d = g.normal(size=(4000, 3))
    shell = np.array([2.0, 1.5, 1.25]) + 50.0 * d / np.linalg.norm(d, axis=1, keepdims=True)   # seen from anywhere
    with pytest.raises(RuntimeError, match="candidates"):
        pkg.evaluation.sample_views(3, ext, tr, shell, 0, H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"],
                                    cx=cam["cx"], cy=cam["cy"])


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
E2E = dict(align=False, n_imgs=8, seed=3, unseen_pc=np.zeros((0, 3)), cam_box=CAM_BOX, H=48, W=64, focal=40.0,
           z_near=0.1, z_far=3.0)


def test_calc_depth_l1_end_to_end(pkg, tmp_path, capsys):
    import raster_scene as R
    E = pkg.evaluation
    gv, gf = R.scene()
    rv, rf = R.scene(box_shift=(0.02, 0.0, 0.0))
    gt, rec = str(tmp_path / "gt.ply"), str(tmp_path / "rec.ply")
    pkg.mesher.write_ply(gt, gv, gf)
    pkg.mesher.write_ply(rec, rv, rf)
    gv, rv = E.load_mesh(gt)["vertices"], E.load_mesh(rec)["vertices"]     # as the file holds them
    same = E.calc_depth_l1(gt, gt, **E2E)
    assert same["depth_l1_cm"] == 0.0 and same["errors"].shape == (8,) and not same["errors"].any()
    capsys.readouterr()
    res = E.calc_depth_l1(rec, gt, **E2E)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Depth L1:")]
    assert len(line) == 1 and float(line[0].split(":")[1]) == res["depth_l1_cm"]
    assert res["views"].shape == (8, 4, 4) and np.array_equal(res["views"], same["views"])
    assert res["depth_l1_cm"] == float(res["errors"].mean() * 100) and res["depth_l1_cm"] > 0.0
    # the errors against the oracle on the returned views: cx = H/2 - 0.5, cy = W/2 - 0.5 as the reference writes
    cam = dict(H=48, W=64, fx=40.0, fy=40.0, cx=23.5, cy=31.5, z_near=0.1, z_far=3.0)
    for b, c2w in enumerate(res["views"]):
        g_lo, g_hi, g_dec = R.oracle(gv, gf, c2w, **cam)
        r_lo, r_hi, r_dec = R.oracle(rv, rf, c2w, **cam)
        want = np.abs(g_lo.astype(np.float32).astype(np.float64) - r_lo.astype(np.float32).astype(np.float64)).mean()
        und = int((~g_dec).sum() + (~r_dec).sum())
        # a decided pixel is within 2 float32 ulps of the oracle in both images, and an ulp is 2^-22 at
        # z <= z_far = 3 (binade [2, 4)): |difference| is off by at most 4 * 2^-22, and so is its mean; the
        # float64 sums add nothing visible.  An undecided pixel may be off by z_far.
        tol = 4 * 2.0 ** -22 + und * cam["z_far"] / (48 * 64)
        print(f"view {b}: error {res['errors'][b]:.9f} oracle {want:.9f} undecided {und}")
        assert abs(res["errors"][b] - want) <= tol
    # the command-line tool returns the same dict
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import eval_recon
    finally:
        sys.path.pop(0)
    np.save(str(tmp_path / "unseen.npy"), np.zeros((0, 3)))
    box = np.zeros((4, 4))
    box[0, :3], box[1:] = CAM_BOX[0], CAM_BOX[1][:3]
    np.save(str(tmp_path / "cam_box.npy"), box)
    cli = eval_recon.main(["--rec_mesh", rec, "--gt_mesh", gt, "-2d", "--no_align", "--n_imgs", "8", "--seed", "3",
                           "--unseen_pc", str(tmp_path / "unseen.npy"), "--cam_box", str(tmp_path / "cam_box.npy"),
                           "--height", "48", "--width", "64", "--focal", "40", "--z_near", "0.1", "--z_far", "3"])
    assert cli["depth_l1_cm"] == res["depth_l1_cm"]
    assert np.array_equal(cli["errors"], res["errors"]) and np.array_equal(cli["views"], res["views"])


def test_render_depth_public_wrapper(pkg, image, ref):
    import torch

    import raster_scene as R
    kw = dict(z_near=R.Z_NEAR, z_far=R.Z_FAR, **R.CAM)
    v, f = np.array(ref["v"]), np.array(ref["f"])             # copies: the shared reference stays read-only
    got = pkg.evaluation.render_depth(v, f, ref["c2w"], **kw)
    assert torch.equal(got.view(torch.int32), image.view(torch.int32))
    got = pkg.evaluation.render_depth(v, f, w2c=np.linalg.inv(ref["c2w"]), **kw)
    assert torch.equal(got.view(torch.int32), image.view(torch.int32))
