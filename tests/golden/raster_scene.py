"""The depth rasteriser's test scene and its numpy oracle (tests/test_gpu_raster.py): a room with one wall open, a
latitude / longitude sphere and a box, six views that reach every path of nslam_raster_depth, and a float64
brute-force ray caster evaluated with two edge tolerances.  Plain numpy.
"""
from __future__ import annotations

import numpy as np

import eval_scene

CAM = dict(H=48, W=64, fx=40.0, fy=40.0, cx=31.5, cy=23.5)
Z_NEAR, Z_FAR = 0.1, 3.0
SPHERE_C, SPHERE_R = np.array([2.6, 1.7, 0.9]), 0.6
BOX_LO, BOX_HI = np.array([0.5, 0.4, 0.0]), np.array([1.3, 1.1, 0.8])
EDGE_TOL = 1e-6          # barycentric band round an edge inside which a pixel may go either way
DECIDED_TOL = 1e-9       # lo and hi agree to this: the pixel is decided
MAX_UNDECIDED = 0.01

# position, direction, up
VIEWS = (
    ((1.0, 1.5, 1.2), (1.0, 0.1, -0.05), (0.0, 0.0, -1.0)),     # out of the open wall: background
    ((2.0, 0.05, 1.0), (1.0, 0.02, 0.1), (0.0, 0.0, -1.0)),     # 5 cm from a wall, along it: the near plane cuts it
    ((3.5, 2.5, 2.0), (-1.0, -0.7, -0.6), (0.0, 0.0, -1.0)),    # z_far clips
    ((2.6, 1.7, 2.2), (0.03, 0.02, -1.0), (0.0, 1.0, 0.0)),     # down on the sphere
    ((0.3, 0.3, 0.3), (0.2, 0.1, -1.0), (0.0, 0.0, -1.0)),      # two floor triangles fill the image
    ((1.2, 2.4, 1.4), (-0.3, -1.0, -0.5), (0.0, 0.0, -1.0)),
)


def sphere_mesh(center=SPHERE_C, radius=SPHERE_R, n_lat=6, n_lon=10):
    """Two poles and n_lat - 1 rings of n_lon vertices → (vertices [2 + (n_lat-1) n_lon, 3], faces int32)."""
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * np.pi * j / n_lon
            v.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    v.append([0.0, 0.0, -1.0])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = []
    for j in range(n_lon):
        f.append([0, ring(1, j), ring(1, j + 1)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    last = len(v) - 1
    for j in range(n_lon):
        f.append([last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    return np.asarray(v) * radius + np.asarray(center), np.array(f, dtype=np.int32)


def scene(box_shift=(0.0, 0.0, 0.0)):
    """(vertices float64 [68,3], faces int32 [122,3]): the room 0..(4,3,2.5) without its x = 4 wall, the sphere
    and the box (moved by box_shift)."""
    rv, rf = eval_scene.box_mesh(skip_wall=1)
    sv, sf = sphere_mesh()
    bv, bf = eval_scene.box_mesh(BOX_LO, BOX_HI)
    bv = bv + np.asarray(box_shift, dtype=np.float64)
    v = np.concatenate([rv, sv, bv], 0)
    f = np.concatenate([rf, sf + len(rv), bf + len(rv) + len(sv)], 0).astype(np.int32)
    return v, f


def degenerate_scene():
    """The scene plus a vertex of NaN, a face that uses it, a face with two equal corners and a face of three
    collinear vertices, put in the middle of the face list: it must render as scene() does."""
    v, f = scene()
    n = len(v)
    # n: a NaN vertex; n + 1: the midpoint of the room's edge from corner 0 (0,0,0) to corner 1 (4,0,0)
    v = np.concatenate([v, [[np.nan, 1.0, 1.0], [2.0, 0.0, 0.0]]], 0)
    bad = np.array([[0, 3, n], [8, 9, 9], [0, 2, 2], [0, n + 1, 1]], dtype=np.int32)
    return v, np.concatenate([f[:40], bad, f[40:]], 0)


def look(pos, direction, up):
    """The reference's viewmatrix (eval_recon.py:15-21) as a 4x4 camera-to-world: z = direction, x = up x z,
    y = z x x (the camera looks along +z, y is down)."""
    z = np.asarray(direction, dtype=np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    y /= np.linalg.norm(y)
    m = np.eye(4)
    m[:3, :4] = np.stack([x, y, z, np.asarray(pos, dtype=np.float64)], 1)
    return m


def views():
    """float64 [6,4,4] camera-to-world."""
    return np.stack([look(*v) for v in VIEWS], 0)


def cast(vertices, faces, c2w, tol, H=CAM["H"], W=CAM["W"], fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"],
         z_near=Z_NEAR, z_far=Z_FAR):
    """Brute force in world space, float64 (Moller-Trumbore): for the ray of every pixel centre, camera-space
    direction ((u - cx) / fx, (v - cy) / fy, 1), the smallest z in (z_near, z_far] among the triangles hit with
    all three barycentrics >= tol; 0 where there is none → [H,W].  The ray parameter is the camera-space z,
    because the direction has z = 1 in the camera and the pose is rigid."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = b - a, c - a
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], -1).reshape(-1, 3)
    d = d_cam @ c2w[:3, :3].T                                   # [P,3]
    o = c2w[:3, 3]
    with np.errstate(all="ignore"):
        p = np.cross(d[:, None, :], e2[None, :, :])              # [P,F,3]
        det = (e1[None] * p).sum(-1)
        tv = (o - a)[None]                                       # [1,F,3]
        bu = (tv * p).sum(-1) / det
        q = np.cross(tv, e1[None])                               # [1,F,3]
        bv = (d[:, None, :] * q).sum(-1) / det
        t = (e2[None] * q).sum(-1) / det
        bw = 1.0 - bu - bv
        ok = (det != 0.0) & (bu >= tol) & (bv >= tol) & (bw >= tol) & (t > z_near) & (t <= z_far)
    t = np.where(ok, t, np.inf).min(1)
    return np.where(np.isfinite(t), t, 0.0).reshape(H, W)


def oracle(vertices, faces, c2w, **kw):
    """(lo, hi, decided) [H,W]: the caster with tolerance +EDGE_TOL and -EDGE_TOL, and where they agree."""
    lo = cast(vertices, faces, c2w, EDGE_TOL, **kw)
    hi = cast(vertices, faces, c2w, -EDGE_TOL, **kw)
    return lo, hi, np.abs(lo - hi) <= DECIDED_TOL


def ulp_diff(got32, want32):
    """|a - b| in float32 units in the last place, for arrays of non-negative finite float32."""
    return np.abs(got32.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))


def check_image(got32, lo, hi, decided):
    """The test's rule → (undecided count, worst ulp distance on decided pixels, undecided pixels matching
    neither caster): decided pixels within 2 float32 ulps of the oracle, undecided ones equal to lo or hi."""
    got32 = np.ascontiguousarray(got32, dtype=np.float32)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    worst = int(ulp_diff(got32, lo32)[decided].max()) if decided.any() else 0
    und = ~decided
    neither = int((und & (ulp_diff(got32, lo32) > 2) & (ulp_diff(got32, hi32) > 2)).sum())
    return int(und.sum()), worst, neither
