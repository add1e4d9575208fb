"""GPU tests of the evaluation module (csrc/nslam_eval.hip, nice-slam_amd/evaluation.py): nearest neighbours against
the reference's KD-tree recording and brute force, the surface sampler against its host restatement, the frustum
test against the recorded formulae, ICP, and calc_3d_metric end to end.  Only tests/golden/eval_fixtures.npz and
the seeded scenes of tests/golden/eval_scene.py are read: never the reference, never scipy."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

DEV = "cuda:0"


@pytest.fixture(scope="module")
def eval_fix():
    with np.load(os.path.join(GOLDEN, "eval_fixtures.npz")) as z:
        return {k: z[k] for k in z.files}


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _brute(q, t):
    """float64 brute force on the device → (dist [N], lowest index among the nearest [N])."""
    import torch
    d = torch.cdist(q, t, compute_mode="donot_use_mm_for_euclid_dist")
    best = d.min(1).values
    first = (d == best[:, None]).to(torch.int32).argmax(1)     # argmax returns the first maximum
    return best, first.to(torch.int32)


def _close(got, want, tol=1e-12):
    return bool(((got - want).abs() <= tol + tol * want.abs()).all())


# ------------------------------------------------------------------------------------------------
# nearest neighbours
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn_run(pkg):
    import eval_scene
    targets, queries = eval_scene.nn_scene()
    t, q = _t(targets), _t(queries)
    grid = pkg.ops.NNGrid(t)
    dist, idx = grid.query(q)
    return t, q, grid, dist, idx


def test_nn_matches_reference_kdtree(nn_run, eval_fix):
    import torch
    t, q, grid, dist, idx = nn_run
    want_d, want_i = _t(eval_fix["nn.dist"]), _t(eval_fix["nn.idx"])
    err = (dist - want_d).abs()
    print(f"grid {list(grid.dims)} cell {grid.cell:.4f}; max |dist - kdtree| {float(err.max()):.3e}")
    assert dist.dtype == torch.float64 and idx.dtype == torch.int32
    assert _close(dist, want_d)
    clear = _t(eval_fix["nn.second"] - eval_fix["nn.dist"] > 1e-12)
    assert int(clear.sum()) > 4000
    assert bool((idx == want_i)[clear].all())
    # the distance is the one to the index returned
    back = (q - t[idx.long()]).norm(dim=1)
    assert _close(dist, back)


def test_metrics_match_reference(pkg, eval_fix):
    import eval_scene
    E = pkg.evaluation
    targets, queries = eval_scene.nn_scene()
    got = [E.accuracy(targets, queries), E.completion(targets, queries), E.completion_ratio(targets, queries)]
    for name, g, w in zip(("accuracy", "completion", "completion_ratio"), got, eval_fix["nn.metrics"]):
        print(name, g, w)
        assert abs(g - w) <= 1e-12 * abs(w), name
    assert E.completion_ratio(targets, queries, dist_th=10.0) == 1.0
    assert E.completion_ratio(targets, queries, dist_th=0.0) == 0.0


def test_nn_edge_cases_against_brute_force(pkg, nn_run):
    import torch

    import eval_scene
    t, q, _, dist, idx = nn_run
    N = pkg.ops.NNGrid
    # one target
    d1, i1 = N(t[:1].contiguous()).query(q[:300].contiguous())
    bd, bi = _brute(q[:300], t[:1])
    assert _close(d1, bd) and bool((i1 == 0).all())
    # coplanar targets (one axis of zero extent), queries off the plane
    flat = t[t[:, 2] == 0.0].contiguous()
    assert flat.shape[0] > 300
    g = N(flat)
    assert g.dims[2] == 1
    d2, i2 = g.query(q[:512].contiguous())
    bd, bi = _brute(q[:512], flat)
    assert _close(d2, bd) and bool((i2 == bi).all())
    # 64 queries 10 m outside the box, on every side
    far = q[:64].clone()
    side = torch.arange(64, device=DEV) % 6
    room = _t(eval_scene.ROOM)
    far[torch.arange(64), side // 2] = torch.where(side % 2 == 0, -10.0, room[side // 2] + 10.0)
    d3, i3 = nn_run[2].query(far.contiguous())
    bd, bi = _brute(far, t)
    assert _close(d3, bd) and bool((i3 == bi).all()) and float(d3.min()) >= 10.0
    # duplicated targets: the lowest original index wins, whatever the order
    dup = torch.cat([t[:700], t[:700].flip(0), t[:700]], 0).contiguous()
    d4, i4 = N(dup).query(q[:700].contiguous())
    bd, bi = _brute(q[:700], dup)
    assert _close(d4, bd) and bool((i4 == bi).all()) and int(i4.max()) < 1400
    exact, ie = N(dup).query(dup[700:1400].contiguous())        # queries ON duplicated targets
    assert bool((exact == 0).all()) and bool((ie == torch.arange(699, -1, -1, device=DEV)).all())
    # a bounded query: misses are inf / -1, hits equal the unbounded query's
    d5, i5 = nn_run[2].query(q, 0.05)
    hit = dist <= 0.05
    assert 0.2 < float(hit.double().mean()) < 0.8
    assert bool((d5[hit] == dist[hit]).all()) and bool((i5[hit] == idx[hit]).all())
    assert bool(torch.isinf(d5[~hit]).all()) and bool((i5[~hit] == -1).all())
    with pytest.raises(ValueError):
        N(torch.full((4, 3), float("nan"), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        N(torch.zeros(0, 3, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------
# sampling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 11])
def test_sample_surface_matches_host_restatement(pkg, seed):
    import eval_scene as S
    assert seed in S.SAMPLE_SEEDS
    v, f = S.sample_mesh()
    pts, fid, cdf = pkg.ops.sample_surface(_t(v), _t(f), S.SAMPLE_COUNT, seed)
    cdf = cdf.cpu().numpy()
    assert abs(cdf[-1] - 59.0) <= 1e-12 and cdf[5] == cdf[4]
    want_p, want_f, _ = S.sample_surface_host(v, f, cdf, S.SAMPLE_COUNT, seed)
    pts, fid = pts.cpu().numpy(), fid.cpu().numpy()
    print(f"seed {seed}: max |points - host| {np.abs(pts - want_p).max():.3e}")
    assert np.array_equal(fid, want_f)
    assert np.abs(pts - want_p).max() <= 1e-12
    assert (fid != 5).all()                                    # the zero-area face
    # every point lies on its face: barycentric coordinates in [0, 1], plane residual
    a, b, c = v[f[fid, 0]], v[f[fid, 1]], v[f[fid, 2]]
    e1, e2, w = b - a, c - a, pts - a
    n = np.cross(e1, e2)
    assert np.abs((w * n).sum(1) / np.linalg.norm(n, axis=1)).max() <= 1e-12
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    det = d11 * d22 - d12 * d12
    s = (d22 * (w * e1).sum(1) - d12 * (w * e2).sum(1)) / det
    t = (d11 * (w * e2).sum(1) - d12 * (w * e1).sum(1)) / det
    assert s.min() >= -1e-12 and t.min() >= -1e-12 and (s + t).max() <= 1 + 1e-12
    # per-face counts within 5 sigma of the area shares
    share = np.diff(np.concatenate([[0.0], cdf])) / cdf[-1]
    cnt = np.bincount(fid, minlength=f.shape[0])
    sig = np.sqrt(S.SAMPLE_COUNT * share * (1 - share))
    assert (np.abs(cnt - S.SAMPLE_COUNT * share) <= 5 * sig).all()


def test_sample_surface_public_interface(pkg):
    import torch

    import eval_scene as S
    v, f = S.sample_mesh()
    pts, fid = pkg.evaluation.sample_surface(v, f, 1000, 4)
    again, _ = pkg.evaluation.sample_surface(v, f, 1000, 4)
    other, _ = pkg.evaluation.sample_surface(v, f, 1000, 5)
    assert pts.is_cuda and pts.dtype == torch.float64 and pts.shape == (1000, 3) and fid.dtype == torch.int32
    assert torch.equal(pts, again) and not torch.equal(pts, other)
    with pytest.raises(ValueError):                            # no area to sample
        pkg.evaluation.sample_surface(v, np.array([[0, 1, 1]], dtype=np.int32), 10, 0)


# ------------------------------------------------------------------------------------------------
# cull
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_poses", [1, 9])
def test_frustum_seen_matches_recorded_formulae(pkg, eval_fix, n_poses):
    import eval_scene as S
    v, poses = S.cull_scene()
    got = pkg.evaluation.seen_vertices(v, poses[:n_poses], **S.CAM).cpu().numpy()
    ref = eval_fix[f"cull.seen{n_poses}"].astype(bool)
    cmp = eval_fix[f"cull.margin{n_poses}"] >= S.CULL_MARGIN
    left_out = 1.0 - cmp.mean()
    bad = got != ref
    print(f"{n_poses} poses: seen {int(got.sum())}, left out {left_out:.4%}, mismatches {int(bad.sum())} "
          f"(compared {int((bad & cmp).sum())})")
    assert left_out <= S.CULL_MAX_LEFT_OUT
    assert got.dtype == bool and got.shape == ref.shape
    assert not (bad & cmp).any()


def test_cull_mesh_keeps_faces_with_a_seen_vertex(pkg):
    import eval_scene as S
    v, poses = S.cull_scene()
    rng = np.random.default_rng(4)
    near = np.argsort(v[:, 0], kind="stable")                  # faces of neighbours: many all-seen, many all-unseen
    faces = np.stack([near[:-2], near[1:-1], near[2:]], 1)[rng.permutation(v.shape[0] - 2)[:3001]].astype(np.int32)
    mesh = {"vertices": v, "faces": faces, "colors": None}
    out = pkg.evaluation.cull_mesh(mesh, poses, **S.CAM)
    seen = pkg.evaluation.seen_vertices(v, poses, **S.CAM).cpu().numpy()
    want = faces[seen[faces].any(1)]
    assert 0 < want.shape[0] < faces.shape[0]
    assert out["faces"].dtype == np.int32 and np.array_equal(out["faces"], want)
    assert out["vertices"] is v and mesh["faces"] is faces     # vertices kept, the input left alone
    none = pkg.evaluation.cull_mesh(mesh, poses[:0], **S.CAM)   # no camera sees anything
    assert none["faces"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------
# ICP
# ------------------------------------------------------------------------------------------------
def test_kabsch_sums_match_torch(pkg):
    import torch

    import eval_scene as S
    src, dst, _ = S.icp_scene()
    a, b = _t(src), _t(dst)
    _, idx = pkg.ops.NNGrid(b).query(a, 0.1)
    got = pkg.ops.kabsch_sums(a, idx, b)
    ok = idx >= 0
    assert 100 < int(ok.sum()) < a.shape[0]                    # some pairs are beyond the threshold
    pa, pb = a[ok], b[idx[ok].long()]
    want = torch.cat([ok.sum().double().reshape(1), pa.sum(0), pb.sum(0), (pa[:, :, None] * pb[:, None, :]).sum(0)
                      .reshape(-1), ((pa - pb) ** 2).sum().reshape(1)]).cpu().numpy()
    rel = np.abs(got - want) / np.abs(want)
    print("kabsch sums: max rel", rel.max())
    assert got.shape == (17,) and got[0] == want[0] and rel.max() <= 1e-12
    assert np.array_equal(got, pkg.ops.kabsch_sums(a, idx, b))
    # a count that is no multiple of the workgroup's 1024 points, and fewer points than one wave
    for n in (1, 63, 1025):
        g = pkg.ops.kabsch_sums(a[:n].contiguous(), idx[:n].contiguous(), b)
        k = ok[:n]
        assert g[0] == int(k.sum())
        if g[0]:
            w = a[:n][k].sum(0).cpu().numpy()
            assert np.abs(g[1:4] - w).max() <= 1e-12 * np.abs(w).max()


def _kabsch_partials(src, idx, targets):
    """The workgroup partials [workgroups, 17] in k_kabsch_sums' order: thread t of workgroup w takes points
    w · 1024 + k · 256 + t for k = 0..3, forms the 17 values as the kernel writes them (e2 summed over r = 0..2
    from 0 before it is added), and the workgroup's sums are csrc/nslam_reduce.h's.  A skipped point adds +0."""
    import ordered_sum_ref as osr
    n = src.shape[0]
    wgs = -(-n // 1024)
    ok = np.zeros(wgs * 1024, bool)
    ok[:n] = idx >= 0
    a, b = np.zeros((wgs * 1024, 3)), np.zeros((wgs * 1024, 3))
    a[:n][ok[:n]] = src[ok[:n]]
    b[:n][ok[:n]] = targets[idx[ok[:n]]]
    vals = np.zeros((17, wgs * 1024))
    vals[0] = ok
    e2 = np.zeros(wgs * 1024)
    for r in range(3):
        vals[1 + r], vals[4 + r] = a[:, r], b[:, r]
        for c in range(3):
            vals[7 + 3 * r + c] = a[:, r] * b[:, c]
        d = a[:, r] - b[:, r]
        e2 = e2 + d * d
    vals[16] = e2
    per_thread = osr.thread_sum(vals.reshape(17, wgs, 4, 256).transpose(2, 0, 1, 3))   # [17, wgs, 256]
    return osr.group_sum(per_thread).T


@pytest.mark.parametrize("n", [1, 63, 1025, 65 * 1024 + 1])
def test_kabsch_sums_bits_are_the_ordered_sum(pkg, n):
    """Bit for bit, the host's chain over the workgroup partials included."""
    import ordered_sum_ref as osr
    rng = np.random.default_rng([9, n])
    src, targets = rng.standard_normal((n, 3)), rng.standard_normal((500, 3))
    idx = rng.integers(0, 500, n).astype(np.int32)
    idx[rng.random(n) < 0.2] = -1
    if n == 1:
        idx[0] = 3
    got = pkg.ops.kabsch_sums(_t(src), _t(idx), _t(targets))
    want = osr.ordered_sum(_kabsch_partials(src, idx, targets))
    assert want[0] == (idx >= 0).sum() > 0
    assert np.array_equal(osr.bits(got), osr.bits(want)), got - want


def test_icp_recovers_the_transform(pkg):
    import eval_scene as S
    src, dst, want = S.icp_scene()
    got = pkg.evaluation.icp_align(src, dst)
    err_r, err_t = np.abs(got[:3, :3] - want[:3, :3]).max(), np.abs(got[:3, 3] - want[:3, 3]).max()
    print(f"icp: max |R - R0| {err_r:.3e}, max |t - t0| {err_t:.3e}")
    assert got.shape == (4, 4) and got.dtype == np.float64 and got[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert err_r <= 1e-9 and err_t <= 1e-9
    assert np.array_equal(got, pkg.evaluation.icp_align(src, dst))   # bit-identical run to run
    moved = pkg.ops.transform_points(_t(src), got).cpu().numpy()
    assert np.abs(moved - dst).max() <= 1e-8
    assert np.array_equal(pkg.evaluation.icp_align(src, dst, max_iteration=0), np.eye(4))


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_calc_3d_metric_end_to_end(pkg, eval_fix, tmp_path, capsys):
    import eval_scene as S
    (gv, gf), (rv, rf) = S.e2e_meshes()
    pkg.mesher.write_ply(str(tmp_path / "gt.ply"), gv, gf)
    pkg.mesher.write_ply(str(tmp_path / "rec.ply"), rv, rf)
    out = pkg.evaluation.calc_3d_metric(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), align=False,
                                        n_points=S.E2E_POINTS, seed=S.E2E_SEED)
    printed = capsys.readouterr().out
    assert list(out) == ["accuracy_cm", "completion_cm", "completion_ratio_pct"]
    for k, w in zip(out, eval_fix["e2e.metrics"]):
        print(k, out[k], w)
        assert abs(out[k] - w) <= 1e-9 * abs(w), k
    assert out["completion_cm"] > out["accuracy_cm"] and out["completion_ratio_pct"] < 100.0
    lines = printed.splitlines()
    assert lines[0].startswith("accuracy:  ") and lines[1].startswith("completion:  ")
    assert lines[2].startswith("completion ratio:  ")
    # with the alignment: the 1 cm shift is mostly undone (the missing wall keeps ICP from the exact answer)
    al = pkg.evaluation.calc_3d_metric(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), align=True,
                                       n_points=S.E2E_POINTS, seed=S.E2E_SEED)
    assert al["accuracy_cm"] < out["accuracy_cm"]
