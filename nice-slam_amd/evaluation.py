"""Evaluation of a run's output with the reference's tools' call surface (src/tools/cull_mesh.py,
src/tools/eval_recon.py, src/tools/eval_ate.py), on the HIP kernels of csrc/nslam_eval.hip.

cull_mesh = vertices against every camera's frustum (nslam_frustum_seen) → faces with a seen vertex
(nslam_mesh_face_cull).  calc_3d_metric = optional point-to-point ICP of the reconstruction's vertices onto the
ground truth's (nslam_nn_query, nslam_kabsch_sums, a 3x3 SVD on the host) → area-weighted surface samples of both
meshes (nslam_face_areas, nslam_sample_surface) → accuracy, completion and completion ratio from exact float64
nearest neighbours (nslam_nn_build / nslam_nn_query).  Torch does allocation, sort, cumsum, searchsorted and
boolean indexing only; trimesh and open3d are not imported, scipy only by oriented_bounds.  evaluate_ate is n x 3
work and runs on the host in float64.  calc_depth_l1 (the reference's calc_2d_metric) = views drawn inside the
ground truth's shrunk oriented box and rejected when they see an unseen point (nslam_views_see_any) → both meshes
rendered from each (nslam_raster_depth, csrc/nslam_raster.hip) → the mean absolute depth difference
(nslam_depth_l1).

Deviations from the reference, all stated in DESIGN.md §7b:
  * the samples come from the package's counter-based stream, not numpy's global RNG (same distribution);
  * icp_align follows open3d's documented point-to-point loop; open3d is absent, so the match with its
    implementation is unpinned;
  * calc_depth_l1 renders with the package's rasteriser (pixel-centre rays, inclusive edges) in place of an
    open3d OpenGL window, draws its views from the counter-based stream, takes the near plane as a parameter and
    restates trimesh's oriented bounds (scipy's ConvexHull, imported lazily); open3d and trimesh are absent, so
    the match with them is unpinned;
  * the trajectory plot is not built.

render_metrics / eval_rendering (the reference has no such tool): PSNR, SSIM, MS-SSIM and rendered-depth
L1 of Renderer.render_img against the frames a run was trained on, on csrc/nslam_metrics.hip (nslam_image_errors,
nslam_ssim).  LPIPS is not computed (it needs network weights the package does not ship).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import mesher, ops

DEVICE = "cuda:0"

# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(data, path):
    if data[:4] != b"ply\n" and data[:5] != b"ply\r\n":
        raise ValueError(f"{path}: not a PLY file")
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if end < 0 or nl < 0:
        raise ValueError(f"{path}: the PLY header does not end")
    fmt, elements = None, []
    for ln in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append({"name": w[1], "count": int(w[2]), "props": []})
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"{path}: a property before any element")
            try:
                if w[1] == "list":
                    elements[-1]["props"].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
                else:
                    elements[-1]["props"].append((w[2], _PLY_TYPES[w[1]], None))
            except (KeyError, IndexError):
                raise ValueError(f"{path}: unknown property line {ln!r}") from None
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: format {fmt!r} is not read (ascii and binary_little_endian are)")
    return fmt, elements, nl + 1


def _split_faces(rows, path):
    """Index lists of 3 or 4 → int32 [F,3]; quads are split 0 1 2 / 0 2 3, in place of the quad."""
    out = []
    for r in rows:
        if len(r) == 3:
            out.append(r)
        elif len(r) == 4:
            out.append((r[0], r[1], r[2]))
            out.append((r[0], r[2], r[3]))
        else:
            raise ValueError(f"{path}: a face with {len(r)} indices (3 or 4 are read)")
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def _faces_fixed(idx, path):
    """idx [F,k] with k = 3 or 4 (every face the same size) → [F',3]."""
    if idx.shape[1] == 3:
        return idx.astype(np.int64)
    if idx.shape[1] == 4:
        return np.stack([idx[:, [0, 1, 2]], idx[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int64)
    raise ValueError(f"{path}: faces with {idx.shape[1]} indices (3 or 4 are read)")


def load_mesh(path):
    """A PLY triangle or quad mesh → dict(vertices float64 [V,3], faces int32 [F,3], colors uint8 [V,3|4] or None).

    Reads ascii and binary_little_endian files with any scalar vertex properties (x, y, z and red, green, blue
    [, alpha] are kept; normals and the rest are skipped) and faces `list uchar|uint8 int|uint vertex_indices`
    (or vertex_index) of 3 or 4 indices; quads are split 0 1 2 / 0 2 3.  A file shorter than its header says,
    or with an index past the vertices, raises ValueError."""
    with open(path, "rb") as fh:
        data = fh.read()
    fmt, elements, pos = _ply_header(data, path)
    names = [e["name"] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: no vertex element")
    tokens, tpos = (data[pos:].split(), 0) if fmt == "ascii" else (None, 0)
    verts = cols = faces = None
    for e in elements:
        n, props = e["count"], e["props"]
        scalar = all(p[2] is None for p in props)
        if e["name"] == "vertex":
            pn = [p[0] for p in props]
            if not scalar or not all(k in pn for k in "xyz"):
                raise ValueError(f"{path}: the vertex element needs scalar x, y, z")
            if fmt == "ascii":
                need = n * len(props)
                if tpos + need > len(tokens):
                    raise ValueError(f"{path}: truncated (vertex data)")
                try:
                    tab = np.array(tokens[tpos:tpos + need], dtype=np.float64).reshape(n, len(props))
                except ValueError:
                    raise ValueError(f"{path}: a vertex value is not a number") from None
                tpos += need
                col = {k: tab[:, i] for i, k in enumerate(pn)}
            else:
                dt = np.dtype([(f"{k}_{i}", "<" + t) for i, (k, t, _) in enumerate(props)])
                if pos + n * dt.itemsize > len(data):
                    raise ValueError(f"{path}: truncated (vertex data)")
                rec = np.frombuffer(data, dtype=dt, count=n, offset=pos)
                pos += n * dt.itemsize
                col = {k: rec[f"{k}_{i}"] for i, k in enumerate(pn)}
            verts = np.stack([col["x"], col["y"], col["z"]], 1).astype(np.float64)
            if all(k in col for k in ("red", "green", "blue")):
                keys = ["red", "green", "blue"] + (["alpha"] if "alpha" in col else [])
                cols = np.stack([col[k] for k in keys], 1).astype(np.uint8)
        elif e["name"] == "face":
            li = [i for i, p in enumerate(props) if p[2] is not None]
            if len(li) != 1 or props[li[0]][0] not in ("vertex_indices", "vertex_index"):
                raise ValueError(f"{path}: the face element needs one list property vertex_indices")
            li = li[0]
            if fmt == "ascii":
                rows = []
                try:
                    for _ in range(n):
                        row = None
                        for i, p in enumerate(props):
                            if i == li:
                                k = int(tokens[tpos])
                                row = tuple(int(t) for t in tokens[tpos + 1:tpos + 1 + k])
                                if len(row) != k:
                                    raise IndexError
                                tpos += 1 + k
                            else:
                                tpos += 1
                        rows.append(row)
                    if tpos > len(tokens):
                        raise IndexError
                except (IndexError, ValueError):
                    raise ValueError(f"{path}: truncated or malformed (face data)") from None
                faces = _split_faces(rows, path)
            else:
                ct, it = np.dtype("<" + props[li][1]), np.dtype("<" + props[li][2])
                if ct.kind == "f" or it.kind == "f":
                    raise ValueError(f"{path}: a face list of floats")
                if n == 0:
                    faces = np.zeros((0, 3), np.int64)
                    continue
                if pos + ct.itemsize > len(data):
                    raise ValueError(f"{path}: truncated (face data)")
                k0 = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                fields = []
                for i, p in enumerate(props):
                    fields += [(f"n_{i}", ct), (f"i_{i}", it, (k0,))] if i == li else [(f"s_{i}", "<" + p[1])]
                dt = np.dtype(fields)
                rec = None
                if pos + n * dt.itemsize <= len(data):
                    rec = np.frombuffer(data, dtype=dt, count=n, offset=pos)
                    if not (rec[f"n_{li}"] == k0).all():
                        rec = None
                if rec is not None:  # every face has k0 indices: one structured read
                    pos += n * dt.itemsize
                    faces = _faces_fixed(rec[f"i_{li}"].reshape(n, k0), path)
                else:                # mixed sizes: face by face
                    rows = []
                    for _ in range(n):
                        row = None
                        for i, p in enumerate(props):
                            if i == li:
                                if pos + ct.itemsize > len(data):
                                    raise ValueError(f"{path}: truncated (face data)")
                                k = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                                pos += ct.itemsize
                                if pos + k * it.itemsize > len(data):
                                    raise ValueError(f"{path}: truncated (face data)")
                                row = tuple(int(v) for v in np.frombuffer(data, dtype=it, count=k, offset=pos))
                                pos += k * it.itemsize
                            else:
                                pos += np.dtype(p[1]).itemsize
                        rows.append(row)
                    if pos > len(data):
                        raise ValueError(f"{path}: truncated (face data)")
                    faces = _split_faces(rows, path)
        else:  # an element this reader has no use for: skipped when its size is known
            if not scalar:
                raise ValueError(f"{path}: element {e['name']!r} has list properties; it cannot be skipped")
            if fmt == "ascii":
                tpos += n * len(props)
                if tpos > len(tokens):
                    raise ValueError(f"{path}: truncated ({e['name']} data)")
            else:
                pos += n * sum(np.dtype(p[1]).itemsize for p in props)
                if pos > len(data):
                    raise ValueError(f"{path}: truncated ({e['name']} data)")
    if faces is None:
        faces = np.zeros((0, 3), np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= verts.shape[0]):
        raise ValueError(f"{path}: a face indexes past the {verts.shape[0]} vertices")
    return {"vertices": verts, "faces": faces.astype(np.int32), "colors": cols}


def load_poses(path):
    """cull_mesh.py:9-19: one 4x4 camera-to-world matrix per line (16 numbers), the y and z columns of its
    rotation negated, cast to float32 → numpy float32 [N,4,4]."""
    poses = []
    with open(path, "r") as f:
        lines = f.readlines()
    for line in lines:
        if not line.strip():
            continue
        c2w = np.array(list(map(float, line.split()))).reshape(4, 4)
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        poses.append(c2w.astype(np.float32))
    return np.stack(poses, 0) if poses else np.zeros((0, 4, 4), np.float32)


def _dev64(x, device=None):
    """Array or tensor → contiguous float64 tensor on the HIP device."""
    if isinstance(x, torch.Tensor):
        dev = x.device if x.is_cuda and device is None else (device or DEVICE)
        return x.detach().to(device=dev, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(device or DEVICE)


def _faces32(faces, device):
    if isinstance(faces, torch.Tensor):
        return faces.detach().to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(faces, dtype=np.int32))).to(device)


# ------------------------------------------------------------------------------------------------
# cull_mesh
# ------------------------------------------------------------------------------------------------
def seen_vertices(vertices, poses, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5, device=None):
    """bool [V] on the device: the vertex lies in some camera's viewing frustum (cull_mesh.py:47-71).
    poses: float32 camera-to-world matrices [N,4,4] as load_poses returns them; inverted here on the host in
    float32, as the reference does."""
    v = _dev64(vertices, device)
    poses = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, dtype=np.float32)
    poses = poses.reshape(-1, 4, 4)
    w2c = np.stack([np.linalg.inv(p).astype(np.float32) for p in poses], 0) if len(poses) else \
        np.zeros((0, 4, 4), np.float32)
    return ops.frustum_seen(v, torch.from_numpy(w2c).to(v.device).contiguous(), H, W, fx, fy, cx, cy)


def cull_mesh(mesh, poses, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5, device=None):
    """cull_mesh.py: drop the faces whose three vertices are all outside every camera's frustum.  mesh: the dict
    load_mesh returns; the result is such a dict with the vertex array (and colours) unchanged, as trimesh's
    update_faces leaves them."""
    seen = seen_vertices(mesh["vertices"], poses, H, W, fx, fy, cx, cy, device)
    faces = _faces32(mesh["faces"], seen.device)
    keep = ops.mesh_face_cull(faces, ~seen)
    out = dict(mesh)
    out["faces"] = faces[keep].cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------------
# 3D reconstruction metrics
# ------------------------------------------------------------------------------------------------
def sample_surface(vertices, faces, count, seed, device=None):
    """trimesh.sample.sample_surface on the device → (points float64 [count,3], face_id int32 [count])."""
    v = _dev64(vertices, device)
    pts, fid, _ = ops.sample_surface(v, _faces32(faces, v.device), count, seed)
    return pts, fid


def nn_distance(query, target, max_dist=None, device=None):
    """Exact nearest neighbour of every query among the targets → (dist float64 [N], idx int32 [N]) on the
    device; beyond max_dist: inf and -1.  `target` may be an ops.NNGrid built earlier."""
    if isinstance(target, ops.NNGrid):
        grid = target
        q = _dev64(query, grid.sorted.device)
    else:
        t = _dev64(target, device)
        grid = ops.NNGrid(t)
        q = _dev64(query, t.device)
    return grid.query(q, max_dist)


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    d, _ = nn_distance(gt_points, rec_points)
    return float((d < dist_th).to(torch.float64).mean())


def accuracy(gt_points, rec_points):
    d, _ = nn_distance(rec_points, gt_points)
    return float(d.mean())


def completion(gt_points, rec_points):
    d, _ = nn_distance(gt_points, rec_points)
    return float(d.mean())


def _kabsch(s):
    """The rigid update (4x4, float64 numpy) that moves the a's onto the b's, from nslam_kabsch_sums' totals."""
    n = s[0]
    sa, sb, sab = s[1:4], s[4:7], s[7:16].reshape(3, 3)
    mu_a, mu_b = sa / n, sb / n
    m = sab - np.outer(sa, sb) / n                      # Σ (a - μa)(b - μb)ᵀ
    u, _, vh = torch.linalg.svd(torch.from_numpy(m))
    u, vh = u.numpy(), vh.numpy()
    d = np.eye(3)
    if np.linalg.det(vh.T @ u.T) < 0:
        d[2, 2] = -1.0
    r = vh.T @ d @ u.T
    t = np.eye(4)
    t[:3, :3] = r
    t[:3, 3] = mu_b - r @ mu_a
    return t


def icp_align(src_vertices, dst_vertices, threshold=0.1, max_iteration=30, relative_fitness=1e-6,
              relative_rmse=1e-6, device=None):
    """Point-to-point ICP of src onto dst from the identity (get_align_transformation, eval_recon.py:45-59:
    open3d's registration_icp with its default criteria) → 4x4 float64 numpy matrix.

    The loop is open3d's as documented: correspondences = nearest target within `threshold` of the transformed
    source, fitness = matched share, inlier RMSE; stop when both change by less than their criterion; else the
    Kabsch update of the matched pairs.  The target grid is built once; every iteration reads 17 sums back."""
    dst = _dev64(dst_vertices, device)
    src = _dev64(src_vertices, dst.device)
    grid = ops.NNGrid(dst)
    trans = np.eye(4)
    n = src.shape[0]

    def register(cur):
        _, idx = grid.query(cur, threshold)
        s = ops.kabsch_sums(cur, idx, dst)
        fit = s[0] / n if n else 0.0
        rmse = float(np.sqrt(s[16] / s[0])) if s[0] > 0 else 0.0
        return s, fit, rmse

    cur = src
    s, fit, rmse = register(cur)
    for _ in range(int(max_iteration)):
        if s[0] < 3:  # no update can be formed
            break
        trans = _kabsch(s) @ trans
        cur = ops.transform_points(src, trans)
        s_new, fit_new, rmse_new = register(cur)
        done = abs(fit - fit_new) < relative_fitness and abs(rmse - rmse_new) < relative_rmse
        s, fit, rmse = s_new, fit_new, rmse_new
        if done:
            break
    return trans


def calc_3d_metric(rec_meshfile, gt_meshfile, align=True, n_points=200000, seed=0, device=None):
    """eval_recon.py:91-117 → {accuracy_cm, completion_cm, completion_ratio_pct}, printed as the reference
    prints them.  The reconstruction is sampled with `seed`, the ground truth with `seed + 1`."""
    rec, gt = load_mesh(rec_meshfile), load_mesh(gt_meshfile)
    rec_v, gt_v = _dev64(rec["vertices"], device), _dev64(gt["vertices"], device)
    if align:
        rec_v = ops.transform_points(rec_v, icp_align(rec_v, gt_v))
    rec_pc, _ = sample_surface(rec_v, rec["faces"], n_points, seed)
    gt_pc, _ = sample_surface(gt_v, gt["faces"], n_points, seed + 1)
    gt_grid, rec_grid = ops.NNGrid(gt_pc), ops.NNGrid(rec_pc)
    d_acc, _ = gt_grid.query(rec_pc)
    d_comp, _ = rec_grid.query(gt_pc)
    out = {"accuracy_cm": float(d_acc.mean()) * 100, "completion_cm": float(d_comp.mean()) * 100,
           "completion_ratio_pct": float((d_comp < 0.05).to(torch.float64).mean()) * 100}
    print('accuracy: ', out["accuracy_cm"])
    print('completion: ', out["completion_cm"])
    print('completion ratio: ', out["completion_ratio_pct"])
    return out


def calc_2d_metric(*args, **kwargs):
    raise NotImplementedError("calc_2d_metric is not an entry point of this package: the 2D depth-L1 metric is "
                              "calc_depth_l1 (seeded views, the near plane as a parameter; DESIGN §7b)")


# ------------------------------------------------------------------------------------------------
# 2D metric: depth L1 (eval_recon.py:120-210)
# ------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
VIEW_BATCH_BYTES = 256 << 20     # two float32 image batches (ground truth, reconstruction) stay under this


def _mix64(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def _uniforms(seed, first, count, k):
    """Uniform k of the draws first..first+count-1 in [0,1): the counter-based stream of nslam_sample_surface,
    (mix64(seed ^ mix64(i * 0x9e3779b97f4a7c15 + k)) >> 11) * 2^-53, on the host."""
    with np.errstate(over="ignore"):
        i = np.arange(first, first + count, dtype=np.uint64)
        bits = _mix64(np.uint64(int(seed) & _M64) ^ _mix64(i * np.uint64(0x9e3779b97f4a7c15) + np.uint64(k)))
    return (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _hull_2d(p):
    """Indices of the convex hull of 2D points, counter-clockwise (Andrew's monotone chain)."""
    order = np.lexsort((p[:, 1], p[:, 0]))
    def half(idx):
        h = []
        for i in idx:
            while len(h) >= 2:
                a, b = p[h[-2]], p[h[-1]]
                if (b[0] - a[0]) * (p[i][1] - a[1]) - (b[1] - a[1]) * (p[i][0] - a[0]) > 0.0:
                    break
                h.pop()
            h.append(i)
        return h
    lo, hi = half(order), half(order[::-1])
    return np.array(lo[:-1] + hi[:-1], dtype=np.int64)


def _min_rectangle(p):
    """The minimum-area rectangle round 2D points → (area, angle of its first axis, lo [2], hi [2] along its
    axes): one candidate per edge of the convex hull."""
    h = p[_hull_2d(p)] if len(p) > 2 else p
    edges = np.roll(h, -1, 0) - h
    norm = np.linalg.norm(edges, axis=1)
    edges = edges[norm > 0.0] / norm[norm > 0.0][:, None]
    if len(edges) == 0:
        edges = np.array([[1.0, 0.0]])
    best = None
    for e in edges:
        x = h @ e
        y = h @ np.array([-e[1], e[0]])
        area = (x.max() - x.min()) * (y.max() - y.min())
        if best is None or area < best[0]:
            best = (area, e, np.array([x.min(), y.min()]), np.array([x.max(), y.max()]))
    return best


def oriented_bounds(vertices):
    """The minimum-volume oriented box of a point set (trimesh.bounds.oriented_bounds) → (to_origin float64
    [4,4], extents float64 [3]): to_origin moves the points into the box -extents/2 .. extents/2, extents ascending,
    the rotation right-handed.  Host, float64: one candidate per face normal of the convex hull (its height along
    the normal times the minimum-area rectangle in the face's plane).  trimesh is absent: ties between candidates
    and the signs of the axes are this function's own."""
    try:
        from scipy.spatial import ConvexHull
    except ImportError as e:
        raise ImportError("evaluation.oriented_bounds needs scipy (scipy.spatial.ConvexHull); install it, or pass "
                          "calc_depth_l1(..., cam_box=(extents, transform))") from e
    v = np.asarray(vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else vertices,
                   dtype=np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    hull = ConvexHull(v)
    hv = v[hull.vertices]
    normals = hull.equations[:, :3]
    # one candidate per distinct direction (a normal and its negation give the same box)
    keys = np.round(normals * np.where(normals[:, [np.argmax(np.abs(normals).sum(0) > 0)]] < 0, -1.0, 1.0), 9)
    _, first = np.unique(keys, axis=0, return_index=True)
    best = None
    for n in normals[np.sort(first)]:
        n = n / np.linalg.norm(n)
        a = np.eye(3)[np.argmin(np.abs(n))]
        u = np.cross(n, a)
        u /= np.linalg.norm(u)
        w = np.cross(n, u)
        area, e, lo2, hi2 = _min_rectangle(np.stack([hv @ u, hv @ w], 1))
        z = hv @ n
        vol = area * (z.max() - z.min())
        if best is None or vol < best[0]:
            ax0 = e[0] * u + e[1] * w
            ax1 = -e[1] * u + e[0] * w
            best = (vol, np.stack([ax0, ax1, n]), np.array([lo2[0], lo2[1], z.min()]),
                    np.array([hi2[0], hi2[1], z.max()]))
    _, rot, lo, hi = best
    ext = hi - lo
    order = np.argsort(ext, kind="stable")
    rot, lo, hi, ext = rot[order], lo[order], hi[order], ext[order]
    if np.linalg.det(rot) < 0.0:      # keep it a rotation: turn the last axis round
        rot[2] = -rot[2]
        lo[2], hi[2] = -hi[2], -lo[2]
    to_origin = np.eye(4)
    to_origin[:3, :3] = rot
    to_origin[:3, 3] = -(lo + hi) / 2.0
    return to_origin, ext


def get_cam_position(gt_vertices):
    """eval_recon.py:120-128 → (extents [3], transform [4,4]): the box the cameras are drawn from, the oriented
    bounds shrunk to (0.3, 0.7, 0.7) of their extents, moved back into the world and lifted 0.4 along world z."""
    to_origin, extents = oriented_bounds(gt_vertices)
    extents = extents * np.array([0.3, 0.7, 0.7])
    transform = np.linalg.inv(to_origin)
    transform[2, 3] += 0.4
    return extents, transform


def _viewmatrix(z, up, pos):
    """eval_recon.py:15-21, for a batch: [n,3,4] = (x, y, z, position) columns."""
    vec2 = z / np.linalg.norm(z, axis=1, keepdims=True)
    vec0 = np.cross(np.broadcast_to(up, vec2.shape), vec2)
    vec0 /= np.linalg.norm(vec0, axis=1, keepdims=True)
    vec1 = np.cross(vec2, vec0)
    vec1 /= np.linalg.norm(vec1, axis=1, keepdims=True)
    return np.stack([vec0, vec1, vec2, pos], 2)


def _check_proj_w2c(c2w):
    """check_proj's matrices (eval_recon.py:67-72): y and z columns negated, float64 inverse, float32 cast."""
    m = c2w.copy()
    m[:, :3, 1] *= -1.0
    m[:, :3, 2] *= -1.0
    return np.linalg.inv(m).astype(np.float32) if len(m) else np.zeros((0, 4, 4), np.float32)


def sample_views(n, extents, transform, unseen_pc, seed, H=500, W=500, fx=300., fy=300., cx=249.5, cy=249.5,
                 batch=None, device=None):
    """The views of calc_2d_metric's loop (eval_recon.py:159-178) → float64 numpy [n,4,4] camera-to-world.

    Candidate i draws six uniforms from the counter-based stream (seed, i, k): its origin is uniform in the box
    ((u - 1/2) * extents, then `transform`: trimesh.sample.volume_rectangular), its target has each coordinate
    uniform in +-10000 rounded to two decimals, its pose is viewmatrix(target - origin, (0, 0, -1), origin).  A
    candidate whose image holds a point of unseen_pc (check_proj) is rejected; the result is the first n accepted
    candidates in candidate order, so it depends on the seed and not on `batch` (candidates tested per launch).
    After 64 n candidates without n accepted: RuntimeError (the reference would loop for ever)."""
    n = int(n)
    extents = np.asarray(extents, dtype=np.float64).reshape(3)
    transform = np.asarray(transform, dtype=np.float64).reshape(4, 4)
    pc = None
    if unseen_pc is not None and len(unseen_pc):
        pc = _dev64(unseen_pc, device).reshape(-1, 3).contiguous()
    batch = max(1, int(batch) if batch else max(64, 2 * n))
    up = np.array([0.0, 0.0, -1.0])
    kept, have, first, limit = [], 0, 0, 64 * n
    while have < n:
        if first >= limit:
            raise RuntimeError(f"sample_views: {limit} candidates gave only {have} of {n} views that see no unseen "
                               "point; the camera box or the unseen cloud does not fit this mesh")
        m = min(batch, limit - first)
        u = np.stack([_uniforms(seed, first, m, k) for k in range(6)], 1)
        origin = ((u[:, :3] - 0.5) * extents) @ transform[:3, :3].T + transform[:3, 3]
        target = np.round(u[:, 3:] * 20000.0 - 10000.0, 2)
        c2w = np.tile(np.eye(4), (m, 1, 1))
        c2w[:, :3, :] = _viewmatrix(target - origin, up, origin)
        if pc is None:
            ok = np.ones(m, dtype=bool)
        else:
            w2c = torch.from_numpy(_check_proj_w2c(c2w)).to(pc.device).contiguous()
            ok = ~ops.views_see_any(pc, w2c, H, W, fx, fy, cx, cy).cpu().numpy()
        kept.append(c2w[ok][:n - have])
        have += len(kept[-1])
        first += m
    return np.concatenate(kept, 0) if kept else np.zeros((0, 4, 4))


def render_depth(vertices, faces, c2w=None, *, w2c=None, H=500, W=500, fx=300., fy=300., cx=249.5, cy=249.5,
                 z_near=0.01, z_far=20., small_max_pixels=None, device=None):
    """Depth images of a mesh (nslam_raster_depth) → float32 [B,H,W] on the device: the camera-space z of the
    nearest triangle at every pixel centre, 0 for background — what open3d's capture_depth_float_buffer(True)
    returns with mesh_show_back_face.  Give the cameras as c2w (camera-to-world; inverted here in float64, as
    eval_recon.py:181 does) or as w2c = param.extrinsic; [B,4,4], the camera looks along +z with y down."""
    if (c2w is None) == (w2c is None):
        raise ValueError("render_depth: give c2w or w2c (one of them)")
    v = _dev64(vertices, device)
    f = _faces32(faces, v.device)
    if w2c is None:
        c2w = np.asarray(c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float64)
        c2w = c2w.reshape(-1, 4, 4)
        w2c = np.linalg.inv(c2w) if len(c2w) else c2w
    m = _dev64(w2c, v.device)
    m = m.reshape(-1, *m.shape[-2:])
    return ops.render_depth(v, f, m, H, W, fx, fy, cx, cy, z_near, z_far, small_max_pixels)


def _near_plane(vertices):
    """0.01 x the largest extent of the mesh's axis-aligned box: where open3d's view control is understood to put
    the near plane of a camera inside the scene (unpinned: open3d is absent)."""
    if vertices.shape[0] == 0:
        return 0.01
    ext = (vertices.max(0).values - vertices.min(0).values).max()
    return 0.01 * float(ext)


def calc_depth_l1(rec_meshfile, gt_meshfile, align=True, n_imgs=1000, seed=0, *, unseen_pc=None, cam_box=None,
                  H=500, W=500, focal=300., z_near=None, z_far=20., device=None):
    """eval_recon.py:131-210 (calc_2d_metric) → {"depth_l1_cm", "errors" float64 [n_imgs] (metres), "views" float64
    [n_imgs,4,4] camera-to-world}, printed as the reference prints it.

    n_imgs views are drawn inside the ground truth's shrunk oriented box (sample_views, `seed`), both meshes are
    rendered from each (render_depth) and the mean |depth difference| over all pixels (background counts) is
    averaged.  unseen_pc: the points no view may see, [N,3]; None loads the reference's sidecar
    gt_meshfile.replace('.ply', '_pc_unseen.npy'); an empty array turns the rejection off.  cam_box = (extents,
    transform) skips the oriented bounds (no scipy needed).  z_near=None: 0.01 x the largest extent of each
    mesh's own axis-aligned box.  Deviations from the reference: DESIGN §7b."""
    if unseen_pc is None:
        side = gt_meshfile.replace('.ply', '_pc_unseen.npy')
        try:
            unseen_pc = np.load(side)
        except FileNotFoundError:
            raise FileNotFoundError(f"calc_depth_l1: the unseen-point file {side} is missing; pass unseen_pc= "
                                    "(an empty [0,3] array turns the view rejection off)") from None
    unseen_pc = np.asarray(unseen_pc, dtype=np.float64).reshape(-1, 3)
    rec, gt = load_mesh(rec_meshfile), load_mesh(gt_meshfile)
    rec_v, gt_v = _dev64(rec["vertices"], device), _dev64(gt["vertices"], device)
    if not rec_v.is_cuda:
        raise RuntimeError("calc_depth_l1: nice-slam_amd kernels run on the HIP device only; got a CPU device")
    rec_f, gt_f = _faces32(rec["faces"], rec_v.device), _faces32(gt["faces"], gt_v.device)
    if align:
        rec_v = ops.transform_points(rec_v, icp_align(rec_v, gt_v))
    extents, transform = cam_box if cam_box is not None else get_cam_position(gt["vertices"])
    H, W = int(H), int(W)
    fx = fy = float(focal)
    cx, cy = H / 2.0 - 0.5, W / 2.0 - 0.5      # as the reference writes them
    views = sample_views(n_imgs, extents, transform, unseen_pc, seed, H, W, fx, fy, cx, cy, device=gt_v.device)
    zn_gt = _near_plane(gt_v) if z_near is None else float(z_near)
    zn_rec = _near_plane(rec_v) if z_near is None else float(z_near)
    w2c = torch.from_numpy(np.linalg.inv(views)[:, :3, :].copy() if len(views) else np.zeros((0, 3, 4))) \
        .to(gt_v.device).contiguous()
    per = max(1, VIEW_BATCH_BYTES // (2 * 4 * H * W))
    ws = torch.empty(ops.RASTER_WS_BYTES, dtype=torch.uint8, device=gt_v.device)
    errors = []
    for v0 in range(0, len(views), per):
        m = w2c[v0:v0 + per]
        d_gt = ops.render_depth(gt_v, gt_f, m, H, W, fx, fy, cx, cy, zn_gt, z_far, ws=ws)
        d_rec = ops.render_depth(rec_v, rec_f, m, H, W, fx, fy, cx, cy, zn_rec, z_far, ws=ws)
        errors.append(ops.depth_l1(d_gt, d_rec))
    errors = torch.cat(errors).cpu().numpy() if errors else np.zeros(0)
    out = {"depth_l1_cm": float(errors.mean() * 100) if len(errors) else float("nan"), "errors": errors,
           "views": views}
    print('Depth L1: ', out["depth_l1_cm"])
    return out


# ------------------------------------------------------------------------------------------------
# ATE (host, float64)
# ------------------------------------------------------------------------------------------------
def convert_poses(c2w_list, N, scale, gt=True):
    """eval_ate.py:239-256 → (translations [M,3] = c2w[:3,3] / scale of frames 0..N, mask bool [N+1]).
    With gt, poses holding NaN or inf are masked out.  The input is not modified (the reference divides in
    place), and only the translation is kept: evaluate_ate reads nothing else of the reference's 7-vector."""
    poses = []
    mask = torch.ones(N + 1).bool()
    for idx in range(0, N + 1):
        c2w = torch.as_tensor(c2w_list[idx])
        if gt and (torch.isinf(c2w).any() or torch.isnan(c2w).any()):
            mask[idx] = 0
            continue
        poses.append(c2w[:3, 3] / scale)
    poses = torch.stack(poses) if poses else torch.zeros(0, 3)
    return poses, mask


def align_horn(model, data):
    """eval_ate.py:44-78: the closed-form (Horn) rigid alignment of model [3,n] onto data [3,n] →
    (rot [3,3], trans [3,1], trans_error [n])."""
    model, data = np.asarray(model, dtype=np.float64), np.asarray(data, dtype=np.float64)
    mm, dm = model.mean(1, keepdims=True), data.mean(1, keepdims=True)
    mz, dz = model - mm, data - dm
    u, _, vh = np.linalg.svd((mz @ dz.T).transpose())   # Σ outer(model_c, data_c) over the frames, transposed
    s = np.identity(3)
    if np.linalg.det(u) * np.linalg.det(vh) < 0:
        s[2, 2] = -1
    rot = u @ s @ vh
    trans = dm - rot @ mm
    err = rot @ model + trans - data
    return rot, trans, np.sqrt(np.sum(np.multiply(err, err), 0))


def evaluate_ate(poses_gt, poses_est):
    """eval_ate.py:113-236 for two trajectories with the same frames ([n, >=3], the translation first) → the
    reference's result dict (ATE after Horn alignment of the estimate onto the ground truth, metres)."""
    def xyz(p):
        p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        return np.asarray(p, dtype=np.float64).reshape(p.shape[0], -1)[:, :3].T
    first, second = xyz(poses_gt), xyz(poses_est)
    if first.shape != second.shape:
        raise ValueError("evaluate_ate: the trajectories differ in length")
    if first.shape[1] < 2:
        raise ValueError("evaluate_ate: fewer than two pose pairs to compare")
    _, _, e = align_horn(second, first)
    return {
        "compared_pose_pairs": len(e),
        "absolute_translational_error.rmse": np.sqrt(np.dot(e, e) / len(e)),
        "absolute_translational_error.mean": np.mean(e),
        "absolute_translational_error.median": np.median(e),
        "absolute_translational_error.std": np.std(e),
        "absolute_translational_error.min": np.min(e),
        "absolute_translational_error.max": np.max(e),
    }


def evaluate_ate_checkpoint(ckpt, scale):
    """The ATE dict of a checkpoint dict (datasets.load_checkpoint): frames 0..ckpt['idx'], invalid ground-truth
    poses masked out of both trajectories (eval_ate.py:286-301)."""
    n = int(ckpt["idx"])
    poses_gt, mask = convert_poses(ckpt["gt_c2w_list"], n, scale)
    poses_est, _ = convert_poses(ckpt["estimate_c2w_list"], n, scale, gt=False)
    return evaluate_ate(poses_gt, poses_est[mask])


# ------------------------------------------------------------------------------------------------
# rendering quality
# ------------------------------------------------------------------------------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
RENDER_METRICS = ("psnr", "ssim", "ms_ssim", "depth_l1")


def _as_image(a, device, name, dims):
    a = torch.as_tensor(a)
    if a.dim() != dims:
        raise ValueError(f"render_metrics: {name} must have {dims} dimensions, got {list(a.shape)}")
    return a.to(device=device, dtype=torch.float32).contiguous()[None]


def _render_sums(color, gt_color, depth, gt_depth, mask, device):
    """The device half of render_metrics → (errors float64 [4], SSIM / CS means float64 [levels,C,2]); no host
    synchronisation.  The means have five levels when both sides exceed 160, else one."""
    if mask not in ops.metrics.MASK_MODES:
        raise ValueError(f"render_metrics: mask must be 'depth' or 'none', got {mask!r}")
    if device is None:
        device = color.device if isinstance(color, torch.Tensor) and color.is_cuda else DEVICE
    color, gt_color = _as_image(color, device, "color", 3), _as_image(gt_color, device, "gt_color", 3)
    depth, gt_depth = _as_image(depth, device, "depth", 2), _as_image(gt_depth, device, "gt_depth", 2)
    errors = ops.image_errors(color, gt_color, depth, gt_depth, mask=mask, clamp=True)[0]
    levels = ops.MS_SSIM_LEVELS if min(color.shape[1:3]) >= ops.MS_SSIM_MIN_SIDE else 1
    means = ops.ssim(color.clamp(0.0, 1.0), gt_color, data_range=1.0, levels=levels)[0]
    return errors, means


def _render_values(errors, means):
    """The host half: errors [4] and means [levels][C][2] (nested lists of floats) → the metrics dict."""
    sq, n_color, ad, n_depth = errors
    if n_color == 0:
        psnr = float("nan")
    else:
        mse = sq / n_color
        psnr = float("inf") if mse == 0 else -10.0 * math.log10(mse)
    ssim = math.fsum(c[0] for c in means[0]) / len(means[0])
    ms = None
    if len(means) == len(MS_SSIM_WEIGHTS):
        per_channel = []
        for ch in range(len(means[0])):
            v = [max(means[l][ch][1], 0.0) for l in range(len(means) - 1)] + [max(means[-1][ch][0], 0.0)]
            per_channel.append(math.prod(x ** w for x, w in zip(v, MS_SSIM_WEIGHTS)))
        ms = math.fsum(per_channel) / len(per_channel)
    return {"psnr": psnr, "ssim": ssim, "ms_ssim": ms,
            "depth_l1": ad / n_depth if n_depth > 0 else float("nan"), "valid_depth_pixels": int(n_depth)}


def render_metrics(color, gt_color, depth, gt_depth, mask="depth", device=None):
    """Rendering quality of one frame → {"psnr", "ssim", "ms_ssim", "depth_l1", "valid_depth_pixels"}.

    color, gt_color [H,W,C] (C = 1 or 3, data range 1; the rendered colour is clamped to [0,1]), depth, gt_depth
    [H,W]; tensors or arrays of any float type (converted to float32 on `device`).  mask "depth" counts only pixels
    with gt_depth > 0 for the PSNR, "none" every pixel; the depth error always counts gt_depth > 0 alone.
      psnr      -10 log10(mse); inf at mse 0, nan when no value counts
      ssim      the mean over channels of the SSIM map's mean (11-tap Gaussian window, sigma 1.5)
      ms_ssim   the mean over channels of the five-level product, cs and ssim clamped at 0; None when a side is
                <= 160 (the fifth level would not hold a window)
      depth_l1  the mean |depth - gt_depth| in the depth's own unit; nan without a valid pixel"""
    errors, means = _render_sums(color, gt_color, depth, gt_depth, mask, device)
    return _render_values(errors.tolist(), means.tolist())


def last_checkpoint(output):
    """The path of the last checkpoint under output/ckpts (eval_ate.py:283-286's rule: sorted names)."""
    ckptsdir = os.path.join(output, "ckpts")
    ckpts = sorted(f for f in os.listdir(ckptsdir) if "tar" in f) if os.path.isdir(ckptsdir) else []
    if not ckpts:
        raise FileNotFoundError(f"no checkpoint under {ckptsdir}")
    return os.path.join(ckptsdir, ckpts[-1])


def eval_rendering(cfg, args, ckpt_path=None, every=5, mask="depth", device=DEVICE, on_frame=None):
    """Rendering quality of a finished run over the frames it was trained on → dict.

    The run's last checkpoint (ckpt_path, else the last one under the output folder: args.output, else
    cfg['data']['output']) gives the grids, the decoders and the estimated poses; every `every`-th frame up to
    the checkpoint's idx is rendered at its estimated pose (Renderer.render_img, stage "color", the frame's depth
    guiding the samples) and compared with the frame (render_metrics).  args: nice, output, input_folder, as
    run.py's.  on_frame(idx, color, gt_color) receives the device images of every evaluated frame (the tool's
    --save_images).  The per-frame sums stay on the device until the loop ends: one download.

    Result: "frames" (indices), per-frame lists under "psnr", "ssim", "ms_ssim", "depth_l1" (a frame without a value
    holds None), their means over the frames that have one under "mean", "frames_without_depth" and
    "frames_without_color" (counts), "checkpoint", "every", "mask"."""
    from . import datasets, slam
    from .renderer import Renderer
    every = int(every)
    if every < 1:
        raise ValueError("eval_rendering: every must be at least 1")
    output = cfg["data"]["output"] if getattr(args, "output", None) is None else args.output
    path = last_checkpoint(output) if ckpt_path is None else ckpt_path
    ck = datasets.load_checkpoint(path, device=device)
    nice = bool(args.nice)
    bound = slam.load_bound(cfg)
    decoders = slam.build_decoders(cfg, bound, device, nice=nice)
    decoders.load_state_dict(ck["decoder_state_dict"])
    H, W, fx, fy, cx, cy = slam.update_cam(cfg)
    from types import SimpleNamespace
    renderer = Renderer(cfg, args, SimpleNamespace(nice=nice, bound=bound, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy))
    reader = datasets.get_dataset(cfg, args, cfg["scale"], device=device, color_dtype=torch.float32)
    est = ck["estimate_c2w_list"]
    frames = [i for i in range(0, min(int(ck["idx"]), len(reader) - 1) + 1, every)]
    sums, means = [], []
    for i in frames:
        _, gt_color, gt_depth, _ = reader[i]
        depth, _, color = renderer.render_img(ck["c"], decoders, est[i].to(device), device, stage="color",
                                              gt_depth=gt_depth)
        e, m = _render_sums(color, gt_color, depth, gt_depth, mask, device)
        sums.append(e)
        means.append(m)
        if on_frame is not None:
            on_frame(i, color, gt_color)
    out = {k: [] for k in RENDER_METRICS}
    if frames:
        sums, means = torch.stack(sums).tolist(), torch.stack(means).tolist()  # the one download
        for e, m in zip(sums, means):
            v = _render_values(e, m)
            for k in RENDER_METRICS:
                out[k].append(None if v[k] is None or math.isnan(v[k]) else v[k])

    def mean(vals):
        have = [v for v in vals if v is not None]
        return math.fsum(have) / len(have) if have else None
    out["mean"] = {k: mean(out[k]) for k in RENDER_METRICS}
    out["frames"] = frames
    out["frames_without_depth"] = sum(v is None for v in out["depth_l1"])
    out["frames_without_color"] = sum(v is None for v in out["psnr"])
    out.update(checkpoint=path, every=every, mask=mask)
    return out


write_ply = mesher.write_ply
