"""Host-side checks of the evaluation module (nice-slam_amd/evaluation.py): evaluate_ate against the reference's own
result dict, the PLY and trajectory readers, the numpy restatement of the surface sampler, and the argument checks
of the evaluation entry points (no GPU calls)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

ATE_KEYS = ("compared_pose_pairs", "absolute_translational_error.rmse", "absolute_translational_error.mean",
            "absolute_translational_error.median", "absolute_translational_error.std",
            "absolute_translational_error.min", "absolute_translational_error.max")


@pytest.fixture(scope="module")
def eval_fix():
    with np.load(os.path.join(GOLDEN, "eval_fixtures.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------
# ATE
# ------------------------------------------------------------------------------------------------
def test_evaluate_ate_matches_reference(pkg, eval_fix):
    import torch

    import eval_scene
    E = pkg.evaluation
    gt, est = eval_scene.ate_scene()
    gt_l, est_l = [torch.from_numpy(p) for p in gt], [torch.from_numpy(p) for p in est]
    n = len(gt_l) - 1
    poses_gt, mask = E.convert_poses(gt_l, n, 1.0)
    poses_est, all_ok = E.convert_poses(est_l, n, 1.0, gt=False)
    assert mask.dtype == torch.bool and mask.shape == (n + 1,) and bool(all_ok.all())
    assert [i for i in range(n + 1) if not mask[i]] == [7, 31]
    assert poses_gt.shape == (n - 1, 3) and poses_est.shape == (n + 1, 3)
    assert np.array_equal(gt_l[3].numpy(), gt[3])                # the input is left alone
    res = E.evaluate_ate(poses_gt, poses_est[mask])
    assert tuple(res.keys()) == ATE_KEYS
    for k, want in zip(ATE_KEYS, eval_fix["ate.values"]):
        print(k, float(res[k]), want)
        assert abs(float(res[k]) - want) <= 1e-12 * max(1.0, abs(want)), k
    # the same through the checkpoint form, and the Horn alignment itself
    ck = {"idx": n, "gt_c2w_list": torch.from_numpy(gt), "estimate_c2w_list": torch.from_numpy(est)}
    res2 = E.evaluate_ate_checkpoint(ck, 1.0)
    assert all(float(res2[k]) == float(res[k]) for k in ATE_KEYS)
    ok = mask.numpy()
    rot, trans, _ = E.align_horn(est[ok][:, :3, 3].T, gt[ok][:, :3, 3].T)
    assert np.abs(rot - eval_fix["ate.rot"]).max() <= 1e-12 and np.abs(trans - eval_fix["ate.trans"]).max() <= 1e-12


def test_eval_ate_tool_reads_a_package_checkpoint(pkg, eval_fix, tmp_path, capsys):
    """tools/eval_ate.py on a checkpoint the package wrote: the last one of DIR/ckpts, the config's scale."""
    import torch

    import eval_scene
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import eval_ate
    finally:
        sys.path.pop(0)
    gt, est = eval_scene.ate_scene(scale=2.0)
    os.makedirs(tmp_path / "ckpts")
    for idx in (10, 49):
        pkg.datasets.save_checkpoint(str(tmp_path / "ckpts" / f"{idx:05d}.tar"), {}, torch.nn.Linear(1, 1),
                                     torch.from_numpy(gt), torch.from_numpy(est), [0], idx)
    (tmp_path / "base.yaml").write_text("scale: 2\n")
    (tmp_path / "run.yaml").write_text(f"inherit_from: {tmp_path / 'base.yaml'}\ndata:\n  output: {tmp_path}\n")
    res = eval_ate.main([str(tmp_path / "run.yaml")])
    out = capsys.readouterr().out
    assert "00049.tar" in out and "absolute_translational_error.rmse" in out
    assert res["compared_pose_pairs"] == 48
    for k, want in zip(ATE_KEYS, eval_fix["ate.values"]):        # scale 2 on both sides: the scene's own metres
        assert abs(float(res[k]) - want) <= 1e-6 * max(1.0, abs(want)), k


def test_convert_poses_scale(pkg):
    import torch

    import eval_scene
    E = pkg.evaluation
    gt1, _ = eval_scene.ate_scene()
    gt4, est4 = eval_scene.ate_scene(scale=4.0)
    p1, m1 = E.convert_poses([torch.from_numpy(p) for p in gt1], 49, 1.0)
    p4, m4 = E.convert_poses([torch.from_numpy(p) for p in gt4], 49, 4.0)
    assert bool((m1 == m4).all()) and p4.dtype == torch.float32
    want = torch.stack([torch.from_numpy(gt4[i])[:3, 3] / 4.0 for i in range(50) if m4[i]])
    assert torch.equal(p4, want)
    assert float((p4 - p1).abs().max()) < 1e-6
    # frames past N are not read
    p, m = E.convert_poses([torch.from_numpy(q) for q in gt4], 5, 4.0)
    assert p.shape == (6, 3) and m.shape == (6,)


def test_evaluate_ate_degenerate_trajectories(pkg):
    E = pkg.evaluation
    s = np.linspace(0.0, 1.0, 12)
    line = np.stack([s, 2.0 * s, -s], 1)                         # collinear: the alignment's SVD has rank 1
    res = E.evaluate_ate(line, line + np.array([0.1, 0.0, 0.0]))
    assert res["compared_pose_pairs"] == 12 and res["absolute_translational_error.rmse"] < 1e-9
    res = E.evaluate_ate(np.zeros((5, 3)), np.zeros((5, 3)))   # a camera that never moved
    assert res["absolute_translational_error.max"] == 0.0
    with pytest.raises(ValueError):
        E.evaluate_ate(line[:1], line[:1])
    with pytest.raises(ValueError):
        E.evaluate_ate(line, line[:5])


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
_QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], dtype=np.float64)


def _ascii_ply(path, cut=None):
    lines = ["ply", "format ascii 1.0", "comment made by a test", "element vertex 5", "property float x",
             "property float y", "property float z", "property float nx", "property float ny", "property float nz",
             "element face 3", "property list uchar int vertex_indices", "end_header"]
    lines += [f"{v[0]} {v[1]} {v[2]} 0 0 1" for v in _QUAD_V]
    lines += ["4 0 1 2 3", "3 0 1 4", "3 1 2 4"]
    txt = "\n".join(lines) + "\n"
    with open(path, "w") as f:
        f.write(txt if cut is None else txt[:-cut])


def _binary_ply(path, cut=None):
    head = ["ply", "format binary_little_endian 1.0", "element vertex 5", "property double x", "property double y",
            "property double z", "property uchar red", "property uchar green", "property uchar blue",
            "property float quality", "property int label", "element face 2",
            "property list uint8 uint vertex_index", "end_header"]
    vdt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("q", "<f4"),
                    ("l", "<i4")])
    v = np.zeros(5, dtype=vdt)
    v["x"], v["y"], v["z"] = _QUAD_V[:, 0], _QUAD_V[:, 1], _QUAD_V[:, 2]
    v["r"], v["g"], v["b"] = np.arange(5) * 10, 7, 200
    body = v.tobytes()
    body += np.array([4], "u1").tobytes() + np.array([0, 1, 2, 3], "<u4").tobytes()      # a quad, then a triangle:
    body += np.array([3], "u1").tobytes() + np.array([2, 3, 4], "<u4").tobytes()         # mixed sizes
    blob = ("\n".join(head) + "\n").encode() + body
    with open(path, "wb") as f:
        f.write(blob if cut is None else blob[:-cut])


def test_load_mesh_reads_ascii_binary_and_own_ply(pkg, tmp_path):
    E = pkg.evaluation
    _ascii_ply(tmp_path / "a.ply")
    m = E.load_mesh(str(tmp_path / "a.ply"))
    assert m["vertices"].dtype == np.float64 and np.array_equal(m["vertices"], _QUAD_V)
    assert m["faces"].dtype == np.int32
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4]] and m["colors"] is None

    _binary_ply(tmp_path / "b.ply")
    m = E.load_mesh(str(tmp_path / "b.ply"))
    assert np.array_equal(m["vertices"], _QUAD_V)
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [2, 3, 4]]
    assert m["colors"].dtype == np.uint8 and m["colors"].tolist() == [[10 * i, 7, 200] for i in range(5)]

    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 2, 4]], dtype=np.int32)
    cols = (np.arange(20).reshape(5, 4) * 3).astype(np.uint8)
    pkg.mesher.write_ply(str(tmp_path / "c.ply"), _QUAD_V, faces, cols)
    m, own = E.load_mesh(str(tmp_path / "c.ply")), pkg.mesher.read_ply(str(tmp_path / "c.ply"))
    assert np.array_equal(m["vertices"], own["vertices"].astype(np.float64))
    assert np.array_equal(m["faces"], own["faces"]) and np.array_equal(m["colors"], own["colors"])
    pkg.mesher.write_ply(str(tmp_path / "d.ply"), _QUAD_V, faces)
    assert E.load_mesh(str(tmp_path / "d.ply"))["colors"] is None


@pytest.mark.parametrize("cut", [1, 9, 40])
def test_load_mesh_rejects_truncated_files(pkg, tmp_path, cut):
    E = pkg.evaluation
    _ascii_ply(tmp_path / "a.ply", cut=cut + 1)      # + 1: the final newline alone is not data
    _binary_ply(tmp_path / "b.ply", cut=cut)
    pkg.mesher.write_ply(str(tmp_path / "c.ply"), _QUAD_V, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    blob = open(tmp_path / "c.ply", "rb").read()
    open(tmp_path / "c.ply", "wb").write(blob[:-cut])
    for name in ("a.ply", "b.ply", "c.ply"):
        with pytest.raises(ValueError):
            E.load_mesh(str(tmp_path / name))


def test_load_mesh_rejects_bad_files(pkg, tmp_path):
    E = pkg.evaluation
    (tmp_path / "x.ply").write_bytes(b"not a mesh\n")
    with pytest.raises(ValueError):
        E.load_mesh(str(tmp_path / "x.ply"))
    (tmp_path / "y.ply").write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                                    "property float z\nelement face 1\nproperty list uchar int vertex_indices\n"
                                    "end_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n")
    with pytest.raises(ValueError, match="past"):
        E.load_mesh(str(tmp_path / "y.ply"))


def test_load_poses_flips(pkg, tmp_path):
    rows = [np.arange(16, dtype=np.float64) + 1.0, np.linspace(-2.0, 2.0, 16)]
    (tmp_path / "traj.txt").write_text("\n".join(" ".join(repr(float(v)) for v in r) for r in rows) + "\n")
    poses = pkg.evaluation.load_poses(str(tmp_path / "traj.txt"))
    assert poses.dtype == np.float32 and poses.shape == (2, 4, 4)
    for got, r in zip(poses, rows):
        want = r.reshape(4, 4).copy()
        want[:3, 1] *= -1
        want[:3, 2] *= -1
        assert np.array_equal(got, want.astype(np.float32))
        assert got[3].tolist() == want[3].astype(np.float32).tolist()   # the last row keeps its signs


# ------------------------------------------------------------------------------------------------
# the sampler's host restatement (what tests/test_gpu_eval.py compares the kernel with)
# ------------------------------------------------------------------------------------------------
def test_host_sampler_distribution_and_reflection():
    import eval_scene as S
    v, f = S.sample_mesh()
    cdf = S.face_cdf(v, f)
    share = np.diff(np.concatenate([[0.0], cdf])) / cdf[-1]
    assert share[5] == 0.0 and abs(cdf[-1] - 2 * (12 + 10 + 7.5)) < 1e-12
    for k in range(3):
        u = S.uniforms(5, 4000, k)
        assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / 4000)
    assert not np.array_equal(S.uniforms(5, 64, 0), S.uniforms(5, 64, 1))
    assert not np.array_equal(S.uniforms(5, 64, 0), S.uniforms(6, 64, 0))
    assert np.array_equal(S.uniforms(5, 64, 2)[:32], S.uniforms(5, 32, 2))      # counter-based: no state
    for seed in S.SAMPLE_SEEDS:
        pts, fid, (u1, u2) = S.sample_surface_host(v, f, cdf, S.SAMPLE_COUNT, seed)
        assert (u1 >= 0).all() and (u2 >= 0).all() and (u1 + u2 <= 1.0).all()
        raw1, raw2 = S.uniforms(seed, S.SAMPLE_COUNT, 1), S.uniforms(seed, S.SAMPLE_COUNT, 2)
        flip = raw1 + raw2 > 1.0
        assert 0.4 < flip.mean() < 0.6
        assert np.array_equal(u1[flip], 1.0 - raw1[flip]) and np.array_equal(u1[~flip], raw1[~flip])
        cnt = np.bincount(fid, minlength=f.shape[0])
        assert cnt[5] == 0
        sig = np.sqrt(S.SAMPLE_COUNT * share * (1 - share))
        assert (np.abs(cnt - S.SAMPLE_COUNT * share) <= 5 * sig).all()
        # every point lies on a wall of the room
        on_wall = np.minimum(np.abs(pts), np.abs(pts - S.ROOM)).min(1)
        assert on_wall.max() <= 1e-12 and (pts >= -1e-12).all() and (pts <= S.ROOM + 1e-12).all()


# ------------------------------------------------------------------------------------------------
# C-ABI argument checks
# ------------------------------------------------------------------------------------------------
def test_eval_entry_points_validate_without_gpu(pkg):
    """The evaluation entry points return NSLAM_EINVAL for null pointers, negative counts, m == 0, non-finite
    grids and a cell grid that does not match its offsets — all before any launch."""
    L = pkg._lib.lib()
    P = 4096  # a fake aligned device pointer, never dereferenced
    assert L.nslam_frustum_seen(None, 10, P, 2, 48, 64, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_frustum_seen(P, 10, None, 2, 48, 64, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_frustum_seen(P, 10, P, 2, 48, 64, 40.0, 40.0, 31.5, 23.5, None, None) == -1
    assert L.nslam_frustum_seen(P, -1, P, 2, 48, 64, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_frustum_seen(P, 10, P, -2, 48, 64, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_frustum_seen(P, 10, P, 2, 0, 64, 40.0, 40.0, 31.5, 23.5, P, None) == -1
    assert L.nslam_frustum_seen(None, 0, None, 0, 48, 64, 40.0, 40.0, 31.5, 23.5, None, None) == 0  # empty: no launch

    assert L.nslam_face_areas(None, 8, P, 12, P, None) == -1
    assert L.nslam_face_areas(P, 8, None, 12, P, None) == -1
    assert L.nslam_face_areas(P, 8, P, 12, None, None) == -1
    assert L.nslam_face_areas(P, 8, P, -1, P, None) == -1
    assert L.nslam_face_areas(P, 0, P, 12, P, None) == -1
    assert L.nslam_face_areas(None, 0, None, 0, None, None) == 0

    assert L.nslam_sample_surface(P, 8, P, P, 12, -5, 1, P, P, None) == -1
    assert L.nslam_sample_surface(P, 8, P, P, 0, 5, 1, P, P, None) == -1          # samples of no faces
    assert L.nslam_sample_surface(P, 8, P, None, 12, 5, 1, P, P, None) == -1
    assert L.nslam_sample_surface(P, 8, P, P, 12, 5, 1, None, P, None) == -1
    assert L.nslam_sample_surface(P, 8, P, P, 12, 5, 1, P, None, None) == -1
    assert L.nslam_sample_surface(None, 0, None, None, 0, 0, 1, None, None, None) == 0

    lo = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    dims = (ctypes.c_int32 * 3)(4, 3, 2)
    bad_lo = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    inf_lo = (ctypes.c_double * 3)(float("inf"), 0.0, 0.0)
    dims0 = (ctypes.c_int32 * 3)(4, 0, 2)
    dims_big = (ctypes.c_int32 * 3)(1024, 1024, 17)
    assert L.nslam_nn_build(P, 0, lo, 0.5, dims, P, None) == -1                   # m == 0
    assert L.nslam_nn_build(P, -3, lo, 0.5, dims, P, None) == -1
    assert L.nslam_nn_build(None, 10, lo, 0.5, dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, 0.5, dims, None, None) == -1
    assert L.nslam_nn_build(P, 10, None, 0.5, dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, 0.5, None, P, None) == -1
    assert L.nslam_nn_build(P, 10, bad_lo, 0.5, dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, inf_lo, 0.5, dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, float("nan"), dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, float("inf"), dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, 0.0, dims, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, 0.5, dims0, P, None) == -1
    assert L.nslam_nn_build(P, 10, lo, 0.5, dims_big, P, None) == -1              # more than 2^24 cells

    def query(q=P, n=5, t=P, o=P, m=10, st=P, nst=25, lo_=lo, cell=0.5, dims_=dims, md=-1.0, d=P, i=P):
        return L.nslam_nn_query(q, n, t, o, m, st, nst, lo_, cell, dims_, md, d, i, None)
    assert query(m=0) == -1
    assert query(n=-1) == -1
    assert query(nst=24) == -1 and query(nst=26) == -1                            # offsets of another grid
    assert query(md=float("nan")) == -1
    assert query(lo_=bad_lo) == -1 and query(cell=-1.0) == -1 and query(dims_=dims0) == -1
    for k in ("q", "t", "o", "st", "d", "i"):
        assert query(**{k: None}) == -1, k
    assert query(n=0, q=None, d=None, i=None) == 0                                # no queries: no launch

    rigid = (ctypes.c_double * 12)(*np.eye(4)[:3].ravel())
    nan_rigid = (ctypes.c_double * 12)(*([float("nan")] + [0.0] * 11))
    assert L.nslam_transform_points(P, 5, None, P, None) == -1
    assert L.nslam_transform_points(None, 5, rigid, P, None) == -1
    assert L.nslam_transform_points(P, 5, rigid, None, None) == -1
    assert L.nslam_transform_points(P, -5, rigid, P, None) == -1
    assert L.nslam_transform_points(P, 5, nan_rigid, P, None) == -1
    assert L.nslam_transform_points(None, 0, rigid, None, None) == 0

    assert L.nslam_kabsch_partials(0) == 0 and L.nslam_kabsch_partials(-4) == 0
    assert L.nslam_kabsch_partials(1) == 1 and L.nslam_kabsch_partials(1024) == 1 and L.nslam_kabsch_partials(1025) == 2
    assert L.nslam_kabsch_sums(P, P, 1025, P, 10, P, 1, None) == -1                # a short partial buffer
    assert L.nslam_kabsch_sums(P, P, 1025, P, 0, P, 2, None) == -1                 # m == 0
    assert L.nslam_kabsch_sums(P, P, -1, P, 10, P, 0, None) == -1
    for k in range(4):
        a = [P, P, 1025, P, 10, P, 2, None]
        a[(0, 1, 3, 5)[k]] = None
        assert L.nslam_kabsch_sums(*a) == -1, k
    assert L.nslam_kabsch_sums(None, None, 0, P, 10, None, 0, None) == 0


def test_nn_cell_grid_choice(pkg):
    """The host's grid choice: one cell on an axis of zero extent, at least one per axis, never more than 2^24."""
    g = pkg.ops.nn_cell_grid
    cell, dims = g([0, 0, 0], [4, 3, 2.5], 4099)
    assert all(d >= 1 for d in dims) and dims[0] * dims[1] * dims[2] <= pkg.ops.NN_MAX_CELLS
    assert all(int(e / cell) < d for e, d in zip((4, 3, 2.5), dims))           # the far corner has a cell
    assert 1.0 < 4099 * cell * cell / 59.0 < 4.0                               # a few targets per surface cell
    assert g([0, 0, 1], [4, 3, 1], 1000)[1][2] == 1                            # coplanar
    assert g([1, 1, 1], [1, 1, 1], 1)[1] == [1, 1, 1]                          # one point
    assert g([0, 1, 1], [5, 1, 1], 100)[1][1:] == [1, 1]                       # collinear
    cell, dims = g([0, 0, 0], [1000, 1000, 1000], 10 ** 9)
    assert dims[0] * dims[1] * dims[2] <= pkg.ops.NN_MAX_CELLS


def test_evaluation_has_no_cpu_fallback(pkg):
    import torch
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.frustum_seen(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(1, 4, 4), 48, 64, 40., 40., 31.5, 23.5)
    with pytest.raises(NotImplementedError):
        pkg.evaluation.calc_2d_metric("a.ply", "b.ply")
