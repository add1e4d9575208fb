"""The mesh rasteriser and scene renderer of csrc/nslam_raster.hip."""
import ctypes

import torch

# the header's pass flags and cull modes are _lib's (re-exported here: ops.RASTER_*, ops.SCENE_*, ops.CULL_MODES)
from .._lib import (CULL_MODES, RASTER_ALL, RASTER_BIG, RASTER_CLEAR, RASTER_RESOLVE, RASTER_SMALL,  # noqa: F401
                    SCENE_ALL, SCENE_POINTS, check, lib, ptr, stream_ptr)
from ._check import _on_device, _want, _want_mesh


RASTER_SMALL_MAX_PIXELS = 64     # a larger pixel box goes to the list pass (how it was chosen)
RASTER_WS_BYTES = 64 << 20       # the list's byte budget: 8 M items of 8 bytes
RASTER_MAX_VIEWS = 65535         # views per launch (one grid row each)


def raster_workspace(capacity, device):
    """A workspace for render_depth whose list of large items holds `capacity` entries (uint8 tensor)."""
    return torch.empty(lib().nslam_raster_workspace_size(int(capacity)), dtype=torch.uint8, device=device)


def _views(w2c):
    """The cameras of a call as device float64 [B,3,4] (from [B,3,4] or [B,4,4]) → (w2c, B)."""
    _on_device(w2c, "w2c")
    if w2c.dim() == 3 and tuple(w2c.shape[1:]) == (4, 4):
        w2c = w2c[:, :3, :].contiguous()
    return _want(w2c, "w2c", torch.float64, (int(w2c.shape[0]), 3, 4)), int(w2c.shape[0])


def render_depth(vertices, faces, w2c, H, W, fx, fy, cx, cy, z_near, z_far, small_max_pixels=None, ws=None,
                 passes=RASTER_ALL, out=None):
    """nslam_raster_depth → float32 [B,H,W]: the camera-space z of the nearest triangle along the ray through every
    pixel centre, 0 where nothing is hit.

    vertices float64 [V,3]; faces int32 [F,3]; w2c float64 [B,3,4] or [B,4,4] (the camera looks along +z, x right,
    y down).  small_max_pixels: the largest pixel box a (face, view) thread tests itself (None: the default);
    ws: a raster_workspace (None: one of RASTER_WS_BYTES).  The image does not depend on either.  passes / out:
    run single passes on an image kept between calls (tools/eval_bench.py's per-stage timing)."""
    nv, nf = _want_mesh(vertices, faces, "render_depth")
    dev = vertices.device
    w2c, b = _views(w2c)
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or not float(fx) > 0 or not float(fy) > 0:
        raise ValueError("render_depth: H, W, fx and fy must be positive")
    if not (0.0 <= float(z_near) < float(z_far)):
        raise ValueError(f"render_depth: need 0 <= z_near < z_far, got {z_near}, {z_far}")
    small = RASTER_SMALL_MAX_PIXELS if small_max_pixels is None else int(small_max_pixels)
    if small < 0:
        raise ValueError("render_depth: small_max_pixels must not be negative")
    if out is None:
        out = torch.empty(b, H, W, dtype=torch.float32, device=dev)
        if nf == 0:
            out.zero_()
    _want(out, "out", torch.float32, (b, H, W))
    if b == 0 or nf == 0:
        return out
    if ws is None:
        ws = torch.empty(RASTER_WS_BYTES, dtype=torch.uint8, device=dev)
    _want(ws, "ws", torch.uint8, (None,))
    for v0 in range(0, b, RASTER_MAX_VIEWS):
        v1 = min(b, v0 + RASTER_MAX_VIEWS)
        rc = lib().nslam_raster_depth(ptr(vertices), nv, ptr(faces), nf, ptr(w2c[v0:v1]), v1 - v0, H, W, float(fx),
                                      float(fy), float(cx), float(cy), float(z_near), float(z_far), small,
                                      int(passes), ptr(out[v0:v1]), ptr(ws), ws.numel(), stream_ptr(dev))
        check(rc, "nslam_raster_depth")
    return out


def raster_list_length(ws):
    """The number of items the last SMALL pass appended to (or, past the capacity, drew instead of) the list."""
    return int(ws[:8].view(torch.int64)[0])


SCENE_MAX_POINT_SIZE = 64


def scene_workspace(capacity, n_views, H, W, device):
    """A workspace for render_scene: a list of `capacity` large items and the keys of n_views images (uint8 tensor)."""
    n = lib().nslam_scene_workspace_size(int(capacity), int(n_views), int(H), int(W))
    return torch.empty(n, dtype=torch.uint8, device=device)


def _rgb3(c, name):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise ValueError(f"render_scene: {name} must be three values in 0..255")
    return (ctypes.c_uint8 * 3)(*c)


def render_scene(vertices, faces, vertex_colors, normals, points, point_colors, w2c, H, W, fx, fy, cx, cy, z_near,
                 z_far, point_size=4, cull="none", background=(255, 255, 255), grey=(178, 178, 178), ambient=0.3,
                 small_max_pixels=None, ws=None, passes=SCENE_ALL, out=None, want_depth=True, want_ids=True):
    """nslam_scene_render → (colour uint8 [B,H,W,3], depth float32 [B,H,W] or None, ids int32 [B,H,W] or None): a
    mesh with vertex colours under a head light and depth-tested point sprites, from render_depth's cameras.

    vertices float64 [V,3], faces int32 [F,3], vertex_colors uint8 [V,3] or None (every vertex `grey`), normals
    float32 or float64 [V,3] (unit; not read when F == 0, then all four may be None); points float64 [P,3] and
    point_colors uint8 [P,3] (both None: no points); w2c float64 [B,3,4] or [B,4,4].  ids: a face index, -2 - the
    point's index, -1 for background.  cull: "none" | "back" | "front".  small_max_pixels / ws (a scene_workspace
    for the views of one call; None: a list of RASTER_WS_BYTES): the images do not depend on either.  passes /
    out (the three images of an earlier call): single passes on a workspace kept between calls
    (tools/replay_bench.py's per-stage timing)."""
    w2c, b = _views(w2c)
    dev = w2c.device
    nv = nf = 0
    if faces is not None and faces.shape[0] > 0:
        nv, nf = _want_mesh(vertices, faces, "render_scene")
        if vertex_colors is not None:
            _want(vertex_colors, "vertex_colors", torch.uint8, (nv, 3))
        if not isinstance(normals, torch.Tensor) or normals.dtype not in (torch.float32, torch.float64):
            raise TypeError("normals: expected a float32 or float64 tensor")
        _want(normals, "normals", normals.dtype, (nv, 3))
    else:
        vertices = faces = vertex_colors = normals = None
    n_pts = 0
    if points is not None and points.shape[0] > 0:
        _want(points, "points", torch.float64, (None, 3))
        n_pts = int(points.shape[0])
        _want(point_colors, "point_colors", torch.uint8, (n_pts, 3))
    else:
        points = point_colors = None
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or not float(fx) > 0 or not float(fy) > 0:
        raise ValueError("render_scene: H, W, fx and fy must be positive")
    if not (0.0 <= float(z_near) < float(z_far)):
        raise ValueError(f"render_scene: need 0 <= z_near < z_far, got {z_near}, {z_far}")
    if cull not in CULL_MODES:
        raise ValueError(f"render_scene: cull must be one of {sorted(CULL_MODES)}, got {cull!r}")
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError("render_scene: ambient must lie in [0, 1]")
    if not 0.0 < float(point_size) <= SCENE_MAX_POINT_SIZE:
        raise ValueError(f"render_scene: point_size must lie in (0, {SCENE_MAX_POINT_SIZE}]")
    small = RASTER_SMALL_MAX_PIXELS if small_max_pixels is None else int(small_max_pixels)
    if small < 0:
        raise ValueError("render_scene: small_max_pixels must not be negative")
    bg, gr = _rgb3(background, "background"), _rgb3(grey, "grey")
    if out is None:
        out = (torch.empty(b, H, W, 3, dtype=torch.uint8, device=dev),
               torch.empty(b, H, W, dtype=torch.float32, device=dev) if want_depth else None,
               torch.empty(b, H, W, dtype=torch.int32, device=dev) if want_ids else None)
    color, depth, ids = out
    _want(color, "out[0]", torch.uint8, (b, H, W, 3))
    if depth is not None:
        _want(depth, "out[1]", torch.float32, (b, H, W))
    if ids is not None:
        _want(ids, "out[2]", torch.int32, (b, H, W))
    if b == 0:
        return color, depth, ids
    per = min(b, RASTER_MAX_VIEWS)
    if ws is None:
        ws = torch.empty(RASTER_WS_BYTES + 8 * per * H * W, dtype=torch.uint8, device=dev)
    _want(ws, "ws", torch.uint8, (None,))
    for v0 in range(0, b, RASTER_MAX_VIEWS):
        v1 = min(b, v0 + RASTER_MAX_VIEWS)
        rc = lib().nslam_scene_render(
            ptr(vertices), nv, ptr(faces), nf, ptr(vertex_colors), ptr(normals),
            int(normals is not None and normals.dtype == torch.float64), gr, ptr(points), ptr(point_colors), n_pts,
            float(point_size), ptr(w2c[v0:v1]), v1 - v0, H, W, float(fx), float(fy), float(cx), float(cy),
            float(z_near), float(z_far), CULL_MODES[cull], bg, float(ambient), small, int(passes), ptr(color[v0:v1]),
            ptr(None if depth is None else depth[v0:v1]), ptr(None if ids is None else ids[v0:v1]), ptr(ws),
            ws.numel(), stream_ptr(dev))
        check(rc, "nslam_scene_render")
    return color, depth, ids
