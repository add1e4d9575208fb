"""Mesh extraction, csrc/nslam_mesh.hip: seen masks, marching cubes, the hull test, culling and components."""
import ctypes

import torch

from .._lib import check, lib, ptr, stream_ptr
from ._check import _face_range, _mc_offsets, _want, _want_mesh


def point_masks(points, w2c, depth, H, W, fx, fy, cx, cy, depth_test, use_all_frames, points_batch_size):
    """nslam_point_masks → (seen, forecast, unseen) bool [N] on the device.

    points float32 [N,3]; w2c float32 [K,4,4]; depth float32 [K,H,W] (None with use_all_frames)."""
    _want(points, "points", torch.float32, (None, 3))
    n, dev = points.shape[0], points.device
    k = int(w2c.shape[0])
    _want(w2c, "w2c", torch.float32, (k, 4, 4))
    if not use_all_frames:
        if depth is None:
            raise ValueError("point_masks: depth images are needed unless use_all_frames")
        _want(depth, "depth", torch.float32, (k, H, W))
    else:
        depth = None
    if int(points_batch_size) <= 0:
        raise ValueError("point_masks: points_batch_size must be positive")
    out = torch.empty(3, n, dtype=torch.uint8, device=dev)
    wsb = lib().nslam_point_masks_workspace_size(n, k, int(points_batch_size))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    rc = lib().nslam_point_masks(ptr(points), n, ptr(w2c), k, ptr(depth), int(H), int(W), float(fx), float(fy),
                                 float(cx), float(cy), int(bool(depth_test)), int(bool(use_all_frames)),
                                 int(points_batch_size), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), wsb,
                                 stream_ptr(dev))
    check(rc, "nslam_point_masks")
    return out[0].bool(), out[1].bool(), out[2].bool()


def marching_cubes(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """Indexed iso-surface of a float32 volume [nx,ny,nz] → (verts float64 [V,3], faces int32 [F,3]).

    One vertex per lattice edge with (a < level) != (b < level), at origin + (index + t)·spacing; vertices in
    owner-edge order, faces in cell order, normals toward decreasing values (nslam_mc_count / nslam_mc_emit).
    A value at the level is not below it.  Every loop of a cell is fanned from its valid apex with the lowest
    edge id (csrc/nslam_mc_fan.h, shared with tsdf_marching_cubes): no directed edge occurs twice, also across
    cell faces with four crossings, and the negated volume at the negated level gives every face reversed.  A
    volume with a dimension of 1 holds no cell and gives the empty mesh (0 x 3 and 0 x 3)."""
    _want(volume, "volume", torch.float32, (None, None, None))
    nx, ny, nz = (int(v) for v in volume.shape)
    dev = volume.device
    n = nx * ny * nz
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("marching_cubes: origin and spacing have three entries")
    wsb = lib().nslam_mc_workspace_size(nx, ny, nz)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib().nslam_mc_count(ptr(volume), nx, ny, nz, float(level), ptr(ws), wsb, stream_ptr(dev))
    check(rc, "nslam_mc_count")
    voff, foff, n_verts, n_faces = _mc_offsets(ws[:3 * n], ws[3 * n:])
    verts = torch.empty(n_verts, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    if voff is None:
        return verts, faces
    o = (ctypes.c_double * 3)(*[float(v) for v in origin])
    sp = (ctypes.c_double * 3)(*[float(v) for v in spacing])
    rc = lib().nslam_mc_emit(ptr(volume), nx, ny, nz, float(level), o, sp, ptr(voff), ptr(foff), n_verts, n_faces,
                             ptr(verts), ptr(faces), stream_ptr(dev))
    check(rc, "nslam_mc_emit")
    return verts, faces


def points_in_hull(points, planes):
    """nslam_points_in_hull → bool [N]: planes[k]·(p, 1) <= 0 for all k.  points float32/float64 [N,3]."""
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points: expected float32 or float64, got {points.dtype}")
    _want(points, "points", points.dtype, (None, 3))
    _want(planes, "planes", torch.float64, (None, 4))
    n, dev = points.shape[0], points.device
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib().nslam_points_in_hull(ptr(points), int(points.dtype == torch.float64), n, ptr(planes),
                                    int(planes.shape[0]), ptr(out), stream_ptr(dev))
    check(rc, "nslam_points_in_hull")
    return out.bool()


def mesh_face_cull(faces, vertex_mask):
    """nslam_mesh_face_cull → bool [F]: False for faces whose three vertices are all masked."""
    _want(faces, "faces", torch.int32, (None, 3))
    vm = vertex_mask.to(torch.uint8) if vertex_mask.dtype == torch.bool else vertex_mask
    _want(vm, "vertex_mask", torch.uint8, (None,))
    nf, nv = faces.shape[0], vm.shape[0]
    _face_range(faces, nv, "mesh_face_cull", "the vertex mask")
    keep = torch.empty(nf, dtype=torch.uint8, device=faces.device)
    rc = lib().nslam_mesh_face_cull(ptr(faces), nf, ptr(vm), nv, ptr(keep), stream_ptr(faces.device))
    check(rc, "nslam_mesh_face_cull")
    return keep.bool()


def mesh_components(verts, faces):
    """nslam_mesh_components → (label int32 [V], area float64 [V]); area[l] is the area of component l."""
    nv, nf = _want_mesh(verts, faces, "mesh_components", "verts")
    dev = verts.device
    label = torch.empty(nv, dtype=torch.int32, device=dev)
    area = torch.empty(nv, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = lib().nslam_mesh_components(ptr(verts), nv, ptr(faces), nf, ptr(label), ptr(area), ptr(flag), stream_ptr(dev))
    check(rc, "nslam_mesh_components")
    return label, area


def mesh_keep_components(verts, faces, largest, area_threshold=0.0):
    """trimesh's split + the reference's choice (Mesher.py:498-510): the largest component (largest=True) or
    every component with area > area_threshold, compacted → (verts, faces, vertex ids kept int64)."""
    label, area = mesh_components(verts, faces)
    nv, nf, dev = verts.shape[0], faces.shape[0], verts.device
    if nf == 0:
        return verts[:0], faces[:0], torch.zeros(0, dtype=torch.int64, device=dev)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    used = torch.zeros(nv, dtype=torch.uint8, device=dev)
    big = torch.argmax(area).reshape(1).contiguous() if largest else None
    rc = lib().nslam_mesh_select(ptr(faces), nf, ptr(label), ptr(area), ptr(big), float(area_threshold), ptr(keep),
                                 ptr(used), stream_ptr(dev))
    check(rc, "nslam_mesh_select")
    new_id = (torch.cumsum(used, 0, dtype=torch.int32) - used).contiguous()
    kept_faces = faces[keep.bool()].contiguous()
    out = torch.empty_like(kept_faces)
    rc = lib().nslam_mesh_remap(ptr(kept_faces), kept_faces.shape[0], ptr(new_id), ptr(out), stream_ptr(dev))
    check(rc, "nslam_mesh_remap")
    ids = torch.nonzero(used).reshape(-1)
    return verts[ids], out, ids
