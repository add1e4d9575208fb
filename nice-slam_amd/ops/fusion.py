"""The block volume of tsdf.TSDFVolume on the device: TSDF fusion (csrc/nslam_tsdf.hip) and the depth odometry that
ray-casts it (csrc/nslam_odometry.hip)."""
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._check import _i3, _mc_offsets, _pose16, _want, _want_pool, _want_volume


def _tsdf_frames(depth, c2w, H, W):
    _want(depth, "depth", torch.float32, (None, int(H), int(W)))
    k = int(depth.shape[0])
    _want(c2w, "c2w", torch.float64, (k, 4, 4))
    return k


def tsdf_block_range(depth, c2w, H, W, fx, fy, cx, cy, stride, depth_trunc, voxel, trunc):
    """nslam_tsdf_block_range → (bounds int32 [6]: min x, y, z, max x, y, z; n_valid int64 [1]), on the device.

    depth float32 [K,H,W]; c2w float64 [K,4,4] (+z forward)."""
    k = _tsdf_frames(depth, c2w, H, W)
    dev = depth.device
    bounds = torch.empty(6, dtype=torch.int32, device=dev)
    n_valid = torch.empty(1, dtype=torch.int64, device=dev)
    rc = lib().nslam_tsdf_block_range(ptr(depth), ptr(c2w), k, int(H), int(W), float(fx), float(fy), float(cx),
                                      float(cy), int(stride), float(depth_trunc), float(voxel), float(trunc),
                                      ptr(bounds), ptr(n_valid), stream_ptr(dev))
    check(rc, "nslam_tsdf_block_range")
    return bounds, n_valid


def tsdf_touch(depth, c2w, H, W, fx, fy, cx, cy, stride, depth_trunc, voxel, trunc, block_lo, block_hi):
    """nslam_tsdf_touch → (mask int32 [cells]: bit f = frame f's samples reach the block, in table order;
    n_outside int64 [1]), on the device.  At most 32 frames."""
    k = _tsdf_frames(depth, c2w, H, W)
    dev = depth.device
    lo, hi = _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi")
    cells = max(0, hi[0] - lo[0]) * max(0, hi[1] - lo[1]) * max(0, hi[2] - lo[2])
    if not 0 < cells <= 1 << 27:
        raise ValueError(f"tsdf_touch: the block table [{list(lo)}, {list(hi)}) must hold 1 to 2^27 cells")
    mask = torch.empty(cells, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    rc = lib().nslam_tsdf_touch(ptr(depth), ptr(c2w), k, int(H), int(W), float(fx), float(fy), float(cx), float(cy),
                                int(stride), float(depth_trunc), float(voxel), float(trunc), lo, hi, ptr(mask),
                                ptr(n_out), stream_ptr(dev))
    check(rc, "nslam_tsdf_touch")
    return mask, n_out


def tsdf_integrate(depth, color, w2c, H, W, fx, fy, cx, cy, depth_trunc, voxel, trunc, block_lo, block_hi, list_key,
                   list_id, list_mask, n_pool, tsdf, weight, color_pool):
    """nslam_tsdf_integrate, in place on tsdf / weight [cap,4096] and color_pool [3,cap,4096] (or None).

    depth float32 [K,H,W]; color uint8 [K,H,W,3] or None; w2c float32 [K,4,4]; list_* int32 [n_list]."""
    _want(depth, "depth", torch.float32, (None, int(H), int(W)))
    k = int(depth.shape[0])
    _want(w2c, "w2c", torch.float32, (k, 4, 4))
    n_list = int(list_key.shape[0])
    for name, t in (("list_key", list_key), ("list_id", list_id), ("list_mask", list_mask)):
        _want(t, name, torch.int32, (n_list,))
    cap, n_pool = _want_pool("tsdf_integrate", tsdf, weight, color_pool, n_pool)
    if color_pool is not None:
        if color is None:
            raise ValueError("tsdf_integrate: a volume with colour needs colour images")
        _want(color, "color", torch.uint8, (k, int(H), int(W), 3))
    else:
        color = None
    dev = depth.device
    rc = lib().nslam_tsdf_integrate(ptr(depth), ptr(color), ptr(w2c), k, int(H), int(W), float(fx), float(fy),
                                    float(cx), float(cy), float(depth_trunc), float(voxel), float(trunc),
                                    _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi"), ptr(list_key),
                                    ptr(list_id), ptr(list_mask), n_list, n_pool, ptr(tsdf), ptr(weight),
                                    ptr(color_pool), cap * 4096, stream_ptr(dev))
    check(rc, "nslam_tsdf_integrate")


def tsdf_marching_cubes(tsdf, weight, color_pool, pool_key, n_pool, table, block_lo, block_hi, voxel):
    """nslam_tsdf_mc_count / nslam_tsdf_mc_emit over the first n_pool blocks → (verts float64 [V,3], faces int32
    [F,3], colors uint8 [V,3] or None), vertices in pool / owner-edge order, faces in pool / cell order."""
    cap, n_pool, lo, hi, _ = _want_volume("tsdf_marching_cubes", tsdf, weight, color_pool, pool_key, n_pool, table,
                                          block_lo, block_hi)
    dev = tsdf.device
    n = n_pool * 4096
    verts = torch.empty(0, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    colors = None if color_pool is None else torch.empty(0, 3, dtype=torch.uint8, device=dev)
    if n == 0:
        return verts, faces, colors
    flags = torch.empty(3 * n, dtype=torch.uint8, device=dev)
    ntri = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib().nslam_tsdf_mc_count(ptr(tsdf), ptr(weight), ptr(pool_key), n_pool, ptr(table), lo, hi, ptr(flags),
                                   ptr(ntri), stream_ptr(dev))
    check(rc, "nslam_tsdf_mc_count")
    voff, foff, n_verts, n_faces = _mc_offsets(flags, ntri)
    if voff is None:
        return verts, faces, colors
    verts = torch.empty(n_verts, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    if color_pool is not None:
        colors = torch.empty(n_verts, 3, dtype=torch.uint8, device=dev)
    rc = lib().nslam_tsdf_mc_emit(ptr(tsdf), ptr(weight), ptr(color_pool), cap * 4096, ptr(pool_key), n_pool,
                                  ptr(table), lo, hi, float(voxel), ptr(flags), ptr(ntri), ptr(voff), ptr(foff),
                                  n_verts, n_faces, ptr(verts), ptr(colors), ptr(faces), stream_ptr(dev))
    check(rc, "nslam_tsdf_mc_emit")
    return verts, faces, colors


def depth_maps(depth, fx, fy, cx, cy, depth_trunc, max_jump):
    """nslam_depth_maps → (vertex, normal) float32 [H,W,3] in the camera frame (+z forward), NaN where invalid.

    depth float32 [H,W]."""
    _want(depth, "depth", torch.float32, (None, None))
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if H < 1 or W < 1:
        raise ValueError("depth_maps: an empty image")
    dev = depth.device
    vertex = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    rc = lib().nslam_depth_maps(ptr(depth), H, W, float(fx), float(fy), float(cx), float(cy), float(depth_trunc),
                                float(max_jump), ptr(vertex), ptr(normal), stream_ptr(dev))
    check(rc, "nslam_depth_maps")
    return vertex, normal


def tsdf_raycast(table, pool_key, tsdf, weight, n_pool, block_lo, block_hi, voxel, trunc, c2w, H, W, fx, fy, cx, cy,
                 near, far):
    """nslam_tsdf_raycast over the first n_pool blocks → (vertex, normal) float32 [H,W,3] in the world frame, NaN
    where a ray hits nothing.  c2w: a 4x4 pose (+z forward), read on the host."""
    _, n_pool, lo, hi, _ = _want_volume("tsdf_raycast", tsdf, weight, None, pool_key, n_pool, table, block_lo, block_hi)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("tsdf_raycast: an empty image")
    dev = table.device
    vertex = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    rc = lib().nslam_tsdf_raycast(ptr(table), ptr(pool_key), ptr(tsdf), ptr(weight), n_pool, lo, hi, float(voxel),
                                  float(trunc), _pose16(c2w, "c2w"), H, W, float(fx), float(fy), float(cx), float(cy),
                                  float(near), float(far), ptr(vertex), ptr(normal), stream_ptr(dev))
    check(rc, "nslam_tsdf_raycast")
    return vertex, normal


def icp_sums(src_vertex, src_normal, T, model_vertex, model_normal, w2c, fx, fy, cx, cy, stride, dist_th, cos_th,
             return_mask=False):
    """nslam_icp_sums → float64 [29] on the device: the upper triangle of sum J J^T (21), sum J r (6), sum r^2 and
    the inlier count of the projective point-to-plane association (with return_mask also uint8 [Hs,Ws]: the
    accepted source pixels).

    src_* float32 [Hs,Ws,3] (camera frame); model_* float32 [Hm,Wm,3] (world frame, seen by the camera whose
    world-to-camera matrix is w2c); T, w2c: 4x4 poses read on the host."""
    _want(src_vertex, "src_vertex", torch.float32, (None, None, 3))
    Hs, Ws = int(src_vertex.shape[0]), int(src_vertex.shape[1])
    _want(src_normal, "src_normal", torch.float32, (Hs, Ws, 3))
    _want(model_vertex, "model_vertex", torch.float32, (None, None, 3))
    Hm, Wm = int(model_vertex.shape[0]), int(model_vertex.shape[1])
    _want(model_normal, "model_normal", torch.float32, (Hm, Wm, 3))
    if min(Hs, Ws, Hm, Wm) < 1 or int(stride) < 1:
        raise ValueError("icp_sums: non-empty maps and stride >= 1 expected")
    dev = src_vertex.device
    groups = int(lib().nslam_icp_partials(Hs, Ws, int(stride)))
    partial = torch.empty(groups, 29, dtype=torch.float64, device=dev)
    out = torch.empty(29, dtype=torch.float64, device=dev)
    mask = torch.empty(Hs, Ws, dtype=torch.uint8, device=dev) if return_mask else None
    rc = lib().nslam_icp_sums(ptr(src_vertex), ptr(src_normal), Hs, Ws, int(stride), _pose16(T, "T"),
                              ptr(model_vertex), ptr(model_normal), Hm, Wm, _pose16(w2c, "w2c"), float(fx), float(fy),
                              float(cx), float(cy), float(dist_th), float(cos_th), ptr(partial), groups, ptr(out),
                              ptr(mask), stream_ptr(dev))
    check(rc, "nslam_icp_sums")
    return (out, mask) if return_mask else out


def gray_pyramid(rgb, levels):
    """nslam_gray_pyramid → a list of `levels` float32 [h_l, w_l] views of one buffer, h_l = ceil(H / 2^l): level 0
    is the grey image in [0, 1], every further level the 3 x 3 binomial of the one below at every second pixel.

    rgb uint8 [H,W,3]; levels 1 to 8."""
    _want(rgb, "rgb", torch.uint8, (None, None, 3))
    H, W, levels = int(rgb.shape[0]), int(rgb.shape[1]), int(levels)
    if H < 1 or W < 1:
        raise ValueError("gray_pyramid: an empty image")
    if not 1 <= levels <= 8:
        raise ValueError("gray_pyramid: 1 to 8 levels expected")
    dev = rgb.device
    out = torch.empty(int(lib().nslam_gray_pyramid_size(H, W, levels)), dtype=torch.float32, device=dev)
    rc = lib().nslam_gray_pyramid(ptr(rgb), H, W, levels, ptr(out), stream_ptr(dev))
    check(rc, "nslam_gray_pyramid")
    views, at, h, w = [], 0, H, W
    for _ in range(levels):
        views.append(out[at:at + h * w].view(h, w))
        at, h, w = at + h * w, (h + 1) // 2, (w + 1) // 2
    return views


def photo_sums(src_vertex, src_gray, ref_gray, level, ref_vertex, T, w2c, fx, fy, cx, cy, depth_th, photo_th,
               return_mask=False):
    """nslam_photo_sums → float64 [29] on the device, laid out as icp_sums': the upper triangle of sum J J^T (21),
    sum J r (6), sum r^2 and the count of the photometric residual r = I_ref(projection) - I_src (with return_mask
    also uint8 [Hs,Ws]: the accepted source pixels).

    src_vertex float32 [Hs,Ws,3] (source camera frame); src_gray / ref_gray: level `level` of the two frames'
    gray_pyramid, float32 [ceil(Hs / 2^level), ceil(Ws / 2^level)] and likewise for the reference; ref_vertex
    float32 [Hr,Wr,3]: the reference frame's own vertex map in its camera frame; T (source camera to world) and
    w2c (of the reference camera): 4x4 poses read on the host."""
    level = int(level)
    if not 0 <= level <= 7:
        raise ValueError("photo_sums: level 0 to 7 expected")
    _want(src_vertex, "src_vertex", torch.float32, (None, None, 3))
    Hs, Ws = int(src_vertex.shape[0]), int(src_vertex.shape[1])
    _want(ref_vertex, "ref_vertex", torch.float32, (None, None, 3))
    Hr, Wr = int(ref_vertex.shape[0]), int(ref_vertex.shape[1])
    if min(Hs, Ws, Hr, Wr) < 1:
        raise ValueError("photo_sums: non-empty maps expected")
    S = 1 << level
    sh, sw, rh, rw = -(-Hs // S), -(-Ws // S), -(-Hr // S), -(-Wr // S)
    _want(src_gray, "src_gray", torch.float32, (sh, sw))
    _want(ref_gray, "ref_gray", torch.float32, (rh, rw))
    dev = src_vertex.device
    groups = int(lib().nslam_icp_partials(Hs, Ws, S))
    partial = torch.empty(groups, 29, dtype=torch.float64, device=dev)
    out = torch.empty(29, dtype=torch.float64, device=dev)
    mask = torch.empty(Hs, Ws, dtype=torch.uint8, device=dev) if return_mask else None
    rc = lib().nslam_photo_sums(ptr(src_vertex), Hs, Ws, ptr(src_gray), sh, sw, ptr(ref_gray), rh, rw, level,
                                ptr(ref_vertex), Hr, Wr, _pose16(T, "T"), _pose16(w2c, "w2c"), float(fx), float(fy),
                                float(cx), float(cy), float(depth_th), float(photo_th), ptr(partial), groups,
                                ptr(out), ptr(mask), stream_ptr(dev))
    check(rc, "nslam_photo_sums")
    return (out, mask) if return_mask else out
