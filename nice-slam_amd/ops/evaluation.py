"""Evaluation, csrc/nslam_eval.hip: frustum tests, surface samples, nearest neighbours, ICP sums, depth L1."""
import ctypes

import torch

from .._lib import check, lib, ptr, stream_ptr
from ._check import _want, _want_mesh
from .raster import RASTER_MAX_VIEWS


def frustum_seen(vertices, w2c, H, W, fx, fy, cx, cy):
    """nslam_frustum_seen → bool [N]: the vertex projects into the image of any camera.

    vertices float64 [N,3]; w2c float32 [K,4,4] (inverted on the host by the caller)."""
    _want(vertices, "vertices", torch.float64, (None, 3))
    k = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float32, (k, 4, 4))
    n, dev = vertices.shape[0], vertices.device
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib().nslam_frustum_seen(ptr(vertices), n, ptr(w2c), k, int(H), int(W), float(fx), float(fy), float(cx),
                                  float(cy), ptr(out), stream_ptr(dev))
    check(rc, "nslam_frustum_seen")
    return out.bool()


def face_areas(vertices, faces):
    """nslam_face_areas → float64 [F]."""
    nv, nf = _want_mesh(vertices, faces, "face_areas")
    area = torch.empty(nf, dtype=torch.float64, device=vertices.device)
    rc = lib().nslam_face_areas(ptr(vertices), nv, ptr(faces), nf, ptr(area), stream_ptr(vertices.device))
    check(rc, "nslam_face_areas")
    return area


def sample_surface(vertices, faces, count, seed, cdf=None):
    """nslam_sample_surface → (points float64 [count,3], face_id int32 [count], cdf float64 [F]).

    Area-weighted samples from the counter-based stream (seed, sample, k); cdf = cumsum(face areas) unless given."""
    nv, nf = _want_mesh(vertices, faces, "sample_surface")
    dev = vertices.device
    count = int(count)
    if count < 0:
        raise ValueError("sample_surface: count must not be negative")
    if nf == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    if cdf is None:
        cdf = torch.cumsum(face_areas(vertices, faces), 0)
    _want(cdf, "cdf", torch.float64, (nf,))
    total = float(cdf[-1])
    if not (total > 0.0 and total < float("inf")):
        raise ValueError(f"sample_surface: the mesh's area is {total}")
    points = torch.empty(count, 3, dtype=torch.float64, device=dev)
    face_id = torch.empty(count, dtype=torch.int32, device=dev)
    rc = lib().nslam_sample_surface(ptr(vertices), nv, ptr(faces), ptr(cdf), nf, count,
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(points), ptr(face_id), stream_ptr(dev))
    check(rc, "nslam_sample_surface")
    return points, face_id, cdf


NN_MAX_CELLS = 1 << 24
NN_PER_CELL = 2.0  # targets aimed at per occupied cell


def nn_cell_grid(lo, hi, m):
    """Cell edge and cell counts (host) of the grid over the box lo..hi for m targets, taken as samples of a
    surface: about NN_PER_CELL targets per occupied cell on the box's own surface area; an axis of zero extent
    gets one cell, every axis at least one, at most NN_MAX_CELLS in all."""
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0])
    if area > 0.0:
        cell = (NN_PER_CELL * area / m) ** 0.5
    elif max(ext) > 0.0:
        cell = NN_PER_CELL * max(ext) / m
    else:
        cell = 1.0
    cell = max(cell, max(ext) * 2.0 ** -20, 2.0 ** -1000)
    while True:
        dims = [int(e / cell) + 1 for e in ext]
        if dims[0] * dims[1] * dims[2] <= NN_MAX_CELLS:
            return cell, dims
        cell *= 1.25


class NNGrid:
    """The targets of nn_query sorted into a uniform cell grid (nslam_nn_build): built once per target set."""

    def __init__(self, targets):
        _want(targets, "targets", torch.float64, (None, 3))
        m, dev = targets.shape[0], targets.device
        if m == 0:
            raise ValueError("NNGrid: no targets")
        lo_t, hi_t = targets.min(0).values, targets.max(0).values
        box = torch.stack([lo_t, hi_t]).cpu().tolist()
        if not all(abs(v) < float("inf") for row in box for v in row):  # NaN fails the comparison too
            raise ValueError("NNGrid: a target is not finite")
        self.cell, dims = nn_cell_grid(box[0], box[1], m)
        self.lo = (ctypes.c_double * 3)(*box[0])
        self.dims = (ctypes.c_int32 * 3)(*dims)
        self.cells = dims[0] * dims[1] * dims[2]
        keys = torch.empty(m, dtype=torch.int32, device=dev)
        rc = lib().nslam_nn_build(ptr(targets), m, self.lo, self.cell, self.dims, ptr(keys), stream_ptr(dev))
        check(rc, "nslam_nn_build")
        skeys, order = torch.sort(keys, stable=True)
        self.orig = order.to(torch.int32).contiguous()
        self.sorted = targets[order].contiguous()
        self.start = torch.searchsorted(skeys, torch.arange(self.cells + 1, dtype=torch.int32, device=dev)) \
            .to(torch.int32).contiguous()
        self.targets, self.m = targets, m

    def query(self, queries, max_dist=None):
        """nslam_nn_query → (dist float64 [N], idx int32 [N] into the original targets; inf / -1 past max_dist)."""
        _want(queries, "queries", torch.float64, (None, 3))
        n, dev = queries.shape[0], queries.device
        if n and not bool(torch.isfinite(queries).all()):
            raise ValueError("nn_query: a query is not finite")
        md = -1.0 if max_dist is None else float(max_dist)
        if max_dist is not None and not md >= 0.0:
            raise ValueError("nn_query: max_dist must be >= 0")
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        rc = lib().nslam_nn_query(ptr(queries), n, ptr(self.sorted), ptr(self.orig), self.m, ptr(self.start),
                                  self.start.shape[0], self.lo, self.cell, self.dims, md, ptr(dist), ptr(idx),
                                  stream_ptr(dev))
        check(rc, "nslam_nn_query")
        return dist, idx


def transform_points(points, matrix):
    """nslam_transform_points → float64 [N,3]: R p + t for the host 4x4 (or 3x4) `matrix`."""
    _want(points, "points", torch.float64, (None, 3))
    flat = [float(matrix[r][c]) for r in range(3) for c in range(4)]
    out = torch.empty_like(points)
    rc = lib().nslam_transform_points(ptr(points), points.shape[0], (ctypes.c_double * 12)(*flat), ptr(out),
                                      stream_ptr(points.device))
    check(rc, "nslam_transform_points")
    return out


def kabsch_sums(src, idx, targets):
    """nslam_kabsch_sums → numpy float64 [17]: count, Σa, Σb, Σabᵀ, Σ|a-b|² over the pairs
    (src[i], targets[idx[i]]) with idx[i] >= 0.  The workgroup partials are read back (ICP's one small copy per
    iteration) and added in index order on the host, so the sums are the same on every run."""
    _want(src, "src", torch.float64, (None, 3))
    n, dev = src.shape[0], src.device
    _want(idx, "idx", torch.int32, (n,))
    _want(targets, "targets", torch.float64, (None, 3))
    wgs = lib().nslam_kabsch_partials(n)
    partials = torch.empty(max(wgs, 1), 17, dtype=torch.float64, device=dev)
    if wgs == 0:
        return partials.zero_()[0].cpu().numpy()
    rc = lib().nslam_kabsch_sums(ptr(src), ptr(idx), n, ptr(targets), targets.shape[0], ptr(partials), wgs,
                                 stream_ptr(dev))
    check(rc, "nslam_kabsch_sums")
    return partials.cpu().numpy().cumsum(0)[-1]  # numpy's cumsum is one sequential chain per column


def views_see_any(points, w2c, H, W, fx, fy, cx, cy):
    """nslam_views_see_any → bool [B]: the view's image holds some point of the cloud (frustum_seen's test).

    points float64 [N,3]; w2c float32 [B,4,4] (inverted on the host by the caller)."""
    _want(points, "points", torch.float64, (None, 3))
    b = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float32, (b, 4, 4))
    n, dev = points.shape[0], points.device
    out = torch.zeros(b, dtype=torch.uint8, device=dev)
    for v0 in range(0, b, RASTER_MAX_VIEWS):
        v1 = min(b, v0 + RASTER_MAX_VIEWS)
        rc = lib().nslam_views_see_any(ptr(points), n, ptr(w2c[v0:v1]), v1 - v0, int(H), int(W), float(fx), float(fy),
                                       float(cx), float(cy), ptr(out[v0:v1]), stream_ptr(dev))
        check(rc, "nslam_views_see_any")
    return out.bool()


def depth_l1(a, b):
    """nslam_depth_l1 → float64 [B]: the mean over a view's pixels of |a - b| (float32 [B,H,W] each)."""
    _want(a, "a", torch.float32, (None, None, None))
    _want(b, "b", torch.float32, tuple(a.shape))
    nb, npix = int(a.shape[0]), int(a.shape[1]) * int(a.shape[2])
    if nb and npix == 0:
        raise ValueError("depth_l1: the images have no pixels")
    out = torch.empty(nb, dtype=torch.float64, device=a.device)
    rc = lib().nslam_depth_l1(ptr(a), ptr(b), nb, npix, ptr(out), stream_ptr(a.device))
    check(rc, "nslam_depth_l1")
    return out
