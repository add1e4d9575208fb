"""GPU tests of the replay (nslam_scene_render in csrc/nslam_raster.hip, ops.render_scene, replay.Replay, the root
visualizer.py): ids, depth and colour against the numpy twins of tests/replay_cases.py, the point sprites and their
tie rule, the paths against each other bit for bit, the cull modes, degenerate input, and the command line end to
end on a synthetic output folder.  Only seeded scenes are read: never the reference, never open3d."""
import importlib.util
import io
import os

import numpy as np
import pytest

from conftest import REPO

import replay_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = C.CAM["H"], C.CAM["W"]
CAMERA = (H, W, C.CAM["fx"], C.CAM["fy"], C.CAM["cx"], C.CAM["cy"], C.Z_NEAR, C.Z_FAR)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared reference stays read-only


def _w2c(c2w):
    return _t(np.stack([C.w2c_of(m) for m in c2w], 0) if len(c2w) else np.zeros((0, 3, 4)))


def _render(pkg, mesh, c2w, points=None, colours=None, normals32=False, **kw):
    v, f, col, n = (None,) * 4 if mesh is None else [None if a is None else _t(a) for a in mesh]
    if normals32 and n is not None:
        n = n.float()
    kw.setdefault("background", C.BACKGROUND)
    kw.setdefault("ambient", C.AMBIENT)
    return pkg.ops.render_scene(v, f, col, n, None if points is None else _t(points),
                                None if colours is None else _t(colours), _w2c(c2w), *CAMERA, **kw)


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def ref():
    """The meshes, the views, the point set and the twins' answers at point size 4: computed once, left unchanged."""
    ms, (p, pc), c2w = C.meshes(), C.point_set(), C.views()
    exp = {name: [C.expected(m, v, p, pc, 4) for v in c2w] for name, m in ms.items()}
    for a in (p, pc, c2w) + tuple(x for m in ms.values() for x in m):
        a.setflags(write=False)
    return dict(meshes=ms, p=p, pc=pc, c2w=c2w, exp=exp)


@pytest.fixture(scope="module")
def images(pkg, ref):
    return {name: _render(pkg, m, ref["c2w"], ref["p"], ref["pc"]) for name, m in ref["meshes"].items()}


# ------------------------------------------------------------------------------------------------
# 1. ids and depth
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene", "two_spheres"])
def test_ids_and_depth_match_the_twins(pkg, ref, images, name):
    """Ids equal the twin's on every decided pixel and one of the candidates' elsewhere; depth obeys
    raster_scene.check_image's rule (decided: within 2 float32 ulps; undecided: equal to one of the casters)."""
    import torch
    colour, depth, ids = images[name]
    assert colour.dtype == torch.uint8 and tuple(colour.shape) == (7, H, W, 3)
    assert depth.dtype == torch.float32 and ids.dtype == torch.int32 and tuple(ids.shape) == (7, H, W)
    got_id, got_z = ids.cpu().numpy(), depth.cpu().numpy()
    for b, e in enumerate(ref["exp"][name]):
        dec = e["decided"]
        assert np.array_equal(got_id[b][dec], e["ids_lo"][dec]), b
        und = ~dec
        ok = (got_id[b] == e["ids_lo"]) | (got_id[b] == e["ids_hi"]) | (got_id[b] == -2 - e["point_at"])
        assert ok[und].all(), b
        n_und, worst, neither = C.R.check_image(got_z[b], e["z_lo"], e["z_hi"], dec)
        print(f"{name} view {b}: undecided {n_und}, worst ulp distance {worst}, matching neither {neither}")
        assert n_und <= C.MAX_UNDECIDED * H * W and worst <= 2 and neither == 0
        assert ((got_id[b] == -1) == (got_z[b] == 0)).all()


@pytest.mark.parametrize("name", ["scene", "two_spheres"])
def test_depth_is_the_depth_rasterisers(pkg, ref, name):
    """Culling off and no points: the bits ops.render_depth writes."""
    import torch
    v, f, col, n = ref["meshes"][name]
    _, depth, ids = _render(pkg, ref["meshes"][name], ref["c2w"])
    want = pkg.ops.render_depth(_t(v), _t(f), _w2c(ref["c2w"]), *CAMERA)
    assert torch.equal(depth.view(torch.int32), want.view(torch.int32))
    assert bool(((ids >= 0) == (want > 0)).all()) and int(ids.max()) < len(f) and int(ids.min()) == -1


# ------------------------------------------------------------------------------------------------
# 2. colour
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene", "two_spheres"])
def test_colour_matches_the_twin(pkg, ref, images, name):
    """Within one level of the twin on decided pixels (the device's division and square root may differ from
    numpy's by an ulp, which can cross a rounding boundary); point and background pixels exact."""
    colour, _, ids = (a.cpu().numpy() for a in images[name])
    for b, e in enumerate(ref["exp"][name]):
        dec = e["decided"]
        diff = np.abs(colour[b].astype(np.int64) - e["colour"].astype(np.int64)).max(-1)
        print(f"{name} view {b}: decided pixels whose colour differs at all {int((diff[dec] > 0).sum())}, "
              f"worst {int(diff[dec].max())}")
        assert diff[dec].max() <= 1
        assert (colour[b][ids[b] == -1] == np.array(C.BACKGROUND, dtype=np.uint8)).all()
        pt = ids[b] <= -2
        assert np.array_equal(colour[b][pt], ref["pc"][-2 - ids[b][pt]])
    # float32 normals and a uniform grey are shaded by the same rule
    m = ref["meshes"][name]
    c32 = _render(pkg, m, ref["c2w"][5:6], normals32=True)[0].cpu().numpy()[0]
    assert np.abs(c32.astype(np.int64) - _render(pkg, m, ref["c2w"][5:6])[0].cpu().numpy()[0]).max() <= 1
    grey = _render(pkg, (m[0], m[1], None, m[3]), ref["c2w"][5:6], grey=C.GREY)[0].cpu().numpy()[0]
    fo = ref["exp"][name][5]["fo"]
    want = C.shade(m[0], m[1], None, m[3], ref["c2w"][5], fo["lo"][0], fo["lo"][2])
    dec = fo["decided"] & (fo["lo"][0] >= 0)
    assert np.abs(grey.astype(np.int64) - want)[dec].max() <= 1 and (grey[dec][:, 0] == grey[dec][:, 1]).all()


# ------------------------------------------------------------------------------------------------
# 3. points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 4, 5])
def test_point_sprites(pkg, ref, size):
    """Over the mesh and alone: the sprites cover exactly the twin's pixels, clipped at the border as the twin
    clips them; dropped points (NaN, behind the camera, beyond z_far) do not appear."""
    m, p, pc = ref["meshes"]["scene"], ref["p"], ref["pc"]
    _, _, ids = _render(pkg, m, ref["c2w"], p, pc, point_size=size)
    colour, depth, alone = _render(pkg, None, ref["c2w"], p, pc, point_size=size)
    ids, alone, depth, colour = ids.cpu().numpy(), alone.cpu().numpy(), depth.cpu().numpy(), colour.cpu().numpy()
    clipped = 0
    for b, c2w in enumerate(ref["c2w"]):
        e = C.expected(m, c2w, p, pc, size, fo=ref["exp"]["scene"][b]["fo"])
        dec = e["decided"]
        assert np.array_equal(ids[b][dec], e["ids_lo"][dec]), b
        assert np.array_equal((ids[b] <= -2)[dec], e["point_wins"][dec])
        # no faces: the twin mirrors the point pass operation for operation, so every pixel is exact
        only = C.expected(None, c2w, p, pc, size)
        assert np.array_equal(alone[b], only["ids_lo"]), b
        assert np.array_equal(depth[b], only["z_lo"].astype(np.float32))
        assert np.array_equal(colour[b], only["colour"])
        drawn = set((-2 - np.unique(alone[b][alone[b] <= -2])).tolist())
        assert drawn <= set(only["boxes"]) and len(p) - 1 not in drawn
        clipped += sum(1 for k in only["boxes"].values() if k[4])
    assert clipped > 0 or size == 1                               # (one pixel is inside or outside, never cut)


def test_the_face_wins_the_exact_tie(pkg, ref, images):
    e = ref["exp"]["scene"][6]
    tie = e["tie"]
    ids = images["scene"][2][6].cpu().numpy()
    tie_point = -2 - (len(ref["p"]) - 2)
    assert tie.sum() >= 1 and (ids[tie] >= 0).all() and np.array_equal(ids[tie], e["ids_lo"][tie])
    assert (ids == tie_point).any()                                # beside the box's top the point is drawn
    x0, x1, y0, y1, _ = e["boxes"][len(ref["p"]) - 2]
    assert tie[y0:y1 + 1, x0:x1 + 1].any()


def test_empty_scenes(pkg, ref):
    import torch
    colour, depth, ids = _render(pkg, None, ref["c2w"], background=(9, 200, 31))
    assert bool((colour == torch.tensor([9, 200, 31], dtype=torch.uint8, device=DEV)).all())
    assert float(depth.abs().max()) == 0.0 and bool((ids == -1).all())
    m = ref["meshes"]["scene"]
    none = _render(pkg, (m[0], m[1][:0], m[2], m[3]), ref["c2w"], ref["p"][:0], ref["pc"][:0])
    assert bool((none[2] == -1).all()) and bool((none[0] == 255).all())
    zero = _render(pkg, m, ref["c2w"][:0], ref["p"], ref["pc"])
    assert tuple(zero[0].shape) == (0, H, W, 3) and tuple(zero[2].shape) == (0, H, W)
    colour_only = _render(pkg, m, ref["c2w"], ref["p"], ref["pc"], want_depth=False, want_ids=False)
    assert colour_only[1] is None and colour_only[2] is None


# ------------------------------------------------------------------------------------------------
# 4. path independence
# ------------------------------------------------------------------------------------------------
def test_paths_give_the_same_bits(pkg, ref, images):
    """Everything through the list, everything inline, a list of one item (the producer draws what does not
    fit) and the default again: colour, depth and ids bit for bit."""
    ops = pkg.ops
    m, p, pc = ref["meshes"]["two_spheres"], ref["p"], ref["pc"]
    want = images["two_spheres"]
    one = ops.scene_workspace(1, 7, H, W, DEV)
    assert one.numel() == pkg._lib.lib().nslam_scene_workspace_size(1, 7, H, W)
    big = ops.scene_workspace(1 << 16, 7, H, W, DEV)
    for label, kw in (("list", dict(small_max_pixels=0, ws=big)), ("inline", dict(small_max_pixels=H * W + 7)),
                      ("overflow", dict(small_max_pixels=0, ws=one)), ("default", dict())):
        got = _render(pkg, m, ref["c2w"], p, pc, **kw)
        assert _same(got, want), label
        if label == "list":
            n = ops.raster_list_length(big)
            print("listed items", n)
            assert 7 * 12 < n <= 7 * len(m[1])
        if label == "overflow":
            assert ops.raster_list_length(one) > 1
    single = _render(pkg, m, ref["c2w"][2:3], p, pc)
    assert _same(single, [a[2:3] for a in want])


# ------------------------------------------------------------------------------------------------
# 5. cull modes
# ------------------------------------------------------------------------------------------------
def test_cull_modes(pkg):
    import torch
    v, f, col, n = C.outward_box()
    c2w = C.R.look(*C.CULL_VIEW)[None]
    out = {k: _render(pkg, (v, f, col, n), c2w, cull=k) for k in ("none", "back", "front")}
    exp = {k: C.expected((v, f, col, n), c2w[0], cull=k) for k in ("none", "front")}
    assert _same(out["back"], out["none"])                         # a closed box from outside: every nearest hit is a front
    for k in ("none", "front"):
        ids, z = out[k][2][0].cpu().numpy(), out[k][1][0].cpu().numpy()
        dec = exp[k]["decided"]
        assert np.array_equal(ids[dec], exp[k]["ids_lo"][dec])
        _, worst, neither = C.R.check_image(z, exp[k]["z_lo"], exp[k]["z_hi"], dec)
        assert worst <= 2 and neither == 0
        diff = np.abs(out[k][0][0].cpu().numpy().astype(np.int64) - exp[k]["colour"])[dec]
        assert diff.max() <= 1
    box = (out["none"][2][0] >= 0) & (out["none"][2][0] < 12)
    assert int(box.sum()) > 100
    assert bool((out["front"][1][0][box] > out["none"][1][0][box]).all())      # what lies behind the box's fronts
    assert bool((out["front"][2][0][~box] == -1).all())                       # the floor is a front
    # reversed faces (their vertex normals reverse with them): back and front swap, two-sided shading stays
    rev = (v, np.ascontiguousarray(f[:, ::-1]), col, -n)
    r = {k: _render(pkg, rev, c2w, cull=k) for k in ("none", "back", "front")}
    for a, b in (("back", "front"), ("front", "back"), ("none", "none")):
        dec = _t(exp["none" if a != "front" else "front"]["decided"])
        assert torch.equal(r[a][2][0][dec], out[b][2][0][dec]), (a, b)
        ulp = (r[a][1][0].view(torch.int32) - out[b][1][0].view(torch.int32)).abs()
        level = (r[a][0][0].int() - out[b][0][0].int()).abs()
        print(f"reversed {a} against {b}: depth differs on {int((ulp > 0).sum())} pixels, colour on "
              f"{int((level > 0).any(-1).sum())}")
        # the reversed face sums its edge functions in another order: an ulp of float64, which can cross one
        # float32 rounding boundary of z and one rounding boundary of a colour level
        assert int(ulp[dec].max()) <= 1 and int(level[dec].max()) <= 1


# ------------------------------------------------------------------------------------------------
# 6. degenerate input
# ------------------------------------------------------------------------------------------------
def test_degenerate_faces_draw_nothing(pkg, ref):
    """raster_scene.degenerate_scene() (a NaN vertex, faces of no area, put in the middle of the list) renders as
    scene() does; the ids skip the four bad faces."""
    import torch
    v0, f0 = C.R.scene()
    v1, f1 = C.R.degenerate_scene()
    col = np.random.default_rng(5).integers(0, 256, (len(v1), 3)).astype(np.uint8)
    n0 = C.vertex_normals(v0, f0)
    n1 = np.concatenate([n0, [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]], 0)
    c2w = ref["c2w"][:6]
    for kw in (dict(), dict(small_max_pixels=0)):
        want = _render(pkg, (v0, f0, col[:len(v0)], n0), c2w, ref["p"], ref["pc"], **kw)
        got = _render(pkg, (v1, f1, col, n1), c2w, ref["p"], ref["pc"], **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
        ids = got[2]
        assert not bool(((ids >= 40) & (ids < 44)).any())
        assert torch.equal(torch.where(ids >= 44, ids - 4, ids), want[2])


def test_argument_checks(pkg, ref):
    m = ref["meshes"]["scene"]
    with pytest.raises(ValueError, match="point_size"):
        _render(pkg, m, ref["c2w"], ref["p"], ref["pc"], point_size=65)
    with pytest.raises(ValueError, match="cull"):
        _render(pkg, m, ref["c2w"], cull="both")
    with pytest.raises(ValueError, match="past"):
        _render(pkg, (m[0][:60], m[1], m[2][:60], m[3][:60]), ref["c2w"])
    with pytest.raises(ValueError, match="shape"):
        _render(pkg, (m[0], m[1], m[2][:60], m[3]), ref["c2w"])
    with pytest.raises(TypeError):
        _render(pkg, (m[0], m[1], m[2], m[3].astype(np.float16)), ref["c2w"])
    # the entry point's own codes, before any launch (device pointers that are never read)
    L = pkg._lib.lib()
    import ctypes
    bg = (ctypes.c_uint8 * 3)(0, 0, 0)
    ws = pkg.ops.scene_workspace(4, 1, H, W, DEV)
    w2c, img = _w2c(ref["c2w"][:1]), _t(np.zeros((1, H, W, 3), np.uint8))
    pts = _t(ref["p"])
    args = lambda size, wsb: (None, 0, None, 0, None, None, 1, bg, pts.data_ptr(), _t(ref["pc"]).data_ptr(), 5, size,  # noqa: E731
                              w2c.data_ptr(), 1, H, W, 40.0, 40.0, 31.5, 23.5, 0.0, 3.0, 0, bg, 0.3, 64, 31,
                              img.data_ptr(), None, None, ws.data_ptr(), wsb, None)
    assert L.nslam_scene_render(*args(64.5, ws.numel())) == -2
    assert L.nslam_scene_render(*args(4.0, 24)) == -1
    assert L.nslam_scene_render(*args(-1.0, ws.numel())) == -1


# ------------------------------------------------------------------------------------------------
# 7. end to end
# ------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("replay_cli", os.path.join(REPO, "visualizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


E2E_H, E2E_W, SCALE = 96, 128, 2.0


def _decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.int64)


def test_visualizer_end_to_end(pkg, tmp_path):
    """A synthetic output folder (a checkpoint of 12 poses, meshes at frames 0 and 5) through the root
    visualizer.py at 96 x 128."""
    import torch
    out = tmp_path / "out"
    (out / "ckpts").mkdir(parents=True)
    (out / "mesh").mkdir()
    (tmp_path / "configs").mkdir()
    (tmp_path / "configs" / "nice_slam.yaml").write_text("scale: 1\ndata:\n  output: nowhere\n")
    (tmp_path / "configs" / "scene.yaml").write_text(f"scale: {SCALE}\n")
    g = np.random.default_rng(8)

    def colours(n):       # bright, never red and never dark: the actors are told from the mesh by colour
        return np.stack([g.integers(0, 60, n), g.integers(200, 256, n), g.integers(200, 256, n)], 1).astype(np.uint8)

    # the poses look along -z (the reference's convention), so the viewer sits at z = +2 and sees the mesh at z < 0
    bv, bf = C.eval_scene.box_mesh((-0.9, -0.6, -1.6), (0.9, 0.6, -1.0))
    sv, sf = C.R.sphere_mesh(np.array([0.0, 0.0, -1.3]), 0.7)
    pkg.mesher.write_ply(str(out / "mesh" / "00000_mesh.ply"), bv, bf, colours(len(bv)))
    pkg.mesher.write_ply(str(out / "mesh" / "00005_mesh.ply"), sv, sf, colours(len(sv)))
    est = torch.eye(4).repeat(12, 1, 1)
    est[:, 0, 3] = torch.linspace(-0.55, 0.55, 12) * SCALE
    gt = est.clone()
    gt[:, 1, 3] = 0.5 * SCALE
    ckpt = {"estimate_c2w_list": est.clone(), "gt_c2w_list": gt.clone(), "idx": torch.tensor(11)}
    torch.save(ckpt, str(out / "ckpts" / "00005.tar"))
    torch.save({"estimate_c2w_list": est[:3], "gt_c2w_list": gt[:3], "idx": 2}, str(out / "ckpts" / "00002.tar"))
    argv = [str(tmp_path / "configs" / "scene.yaml"), "--output", str(out), "--save_rendering", "--height", str(E2E_H),
            "--width", str(E2E_W)]
    cli = _cli()
    res = cli.main(argv)
    names = sorted(os.listdir(out / "tmp_rendering"))
    assert names == [f"{k:06d}.jpg" for k in range(1, 13)] and res["frames"] == 12
    data = [open(out / "tmp_rendering" / n, "rb").read() for n in names]
    frames = [_decode(d) for d in data]
    assert all(f.shape == (E2E_H, E2E_W, 3) for f in frames)
    # the mesh changes with frame 6 (index 5); its region: where either frame is not the white background
    region = (np.abs(frames[4] - 255).max(-1) > 40) | (np.abs(frames[5] - 255).max(-1) > 40)
    assert region.sum() > 500 and (np.abs(frames[5] - frames[4]).max(-1)[region] > 30).mean() > 0.2
    assert np.abs(frames[3] - frames[4]).max(-1)[region].mean() < np.abs(frames[5] - frames[4]).max(-1)[region].mean()
    # the estimate's trajectory: list[1:10] is first given at index 10, so its first point shows from frame 11 on
    pose0 = est[0].double().numpy().copy()
    pose0[:3, 3] /= SCALE
    ext = pkg.replay.viewer_extrinsic(pose0)
    fx, fy, cx, cy = pkg.replay.intrinsics(E2E_H, E2E_W, 60.0)
    p1 = ext[:3, :3] @ (est[1, :3, 3].double().numpy() / SCALE) + ext[:3, 3]
    u, v = int(round(fx * p1[0] / p1[2] + cx)), int(round(fy * p1[1] / p1[2] + cy))
    assert 2 <= u < E2E_W - 2 and 2 <= v < E2E_H - 2

    def red(img):
        return (img[..., 0] > 170) & (img[..., 1] < 90) & (img[..., 2] < 90)

    def dark(img):
        return img.max(-1) < 40

    for k, f in enumerate(frames):
        if k >= 5:                                                    # (before, the estimate's actor passes over it)
            assert bool(red(f)[v, u]) == (k >= 10), k
        assert red(f).any() and dark(f).any()                         # both actors, every frame
    # the video: ffmpeg is used when it is there, else the AVI written here
    if res["written"].endswith(".avi"):
        avi = pkg.replay.read_mjpeg_avi(res["written"])
        assert avi["frames"] == data and avi["fps"] == 30.0 and (avi["W"], avi["H"]) == (E2E_W, E2E_H)
        assert len(avi["index"]) == 12
    video = open(res["written"], "rb").read()
    # again: the same bytes, and the checkpoint as it was
    res2 = cli.main(argv)
    assert [open(out / "tmp_rendering" / n, "rb").read() for n in names] == data
    if res2["written"].endswith(".avi"):
        assert open(res2["written"], "rb").read() == video
    after = torch.load(str(out / "ckpts" / "00005.tar"), map_location="cpu")
    assert torch.equal(after["estimate_c2w_list"], est) and torch.equal(after["gt_c2w_list"], gt)
    # without the ground truth: no black actor
    cli.main(argv + ["--no_gt_traj"])
    for n in names:
        f = _decode(open(out / "tmp_rendering" / n, "rb").read())
        assert red(f).any() and not dark(f).any(), n
    # without --save_rendering: the last frame alone
    res3 = cli.main(argv[:3] + argv[4:])
    assert res3["written"] == str(out / "vis_last.jpg") and res3["frames"] == 0
    last = _decode(open(out / "vis_last.jpg", "rb").read())
    assert np.abs(last - frames[-1]).max() == 0
