"""The scene renderer's test scenes and its numpy twins (tests/test_replay_cpu.py, tests/test_gpu_replay.py): an
id-returning brute-force ray caster (the sibling of raster_scene.cast), the head-light shading rule, the point
sprites with their tie rule against faces, and two meshes with seeded colours and a point set.  Plain numpy
float64; tests/golden/raster_scene.py and eval_scene.py are imported as they are.
"""
from __future__ import annotations

import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import eval_scene  # noqa: E402
import raster_scene as R  # noqa: E402

CAM, Z_NEAR, Z_FAR = R.CAM, R.Z_NEAR, R.Z_FAR
EDGE_TOL, DECIDED_TOL = R.EDGE_TOL, R.DECIDED_TOL
SEPARATION = 1e-6            # the second-nearest hit must be farther than the nearest by more than this times z
Z_BAND = 1e-9                # a face's z is trusted to this relative error when it is compared with a point's
MAX_UNDECIDED = 0.02
AMBIENT = 0.3
BACKGROUND, GREY = (255, 255, 255), (178, 178, 178)
BOX_SHIFT = (0.0, 0.0, 0.05)                                   # lifts the box off the coplanar floor
SPHERE2_C, SPHERE2_R = np.array([1.2, 2.2, 0.6]), 0.4
# straight down on the box's top from 1.25 above it: every pixel of the top has the camera z of its vertices, so a
# point AT a vertex ties with the face in float32 (1.25 is far from a float32 rounding boundary)
TIE_VIEW = ((0.9, 0.75, 2.1), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
TIE_POINT = np.array([1.3, 0.4, 0.85])                          # the top's corner off its diagonal
ACTOR_POSE_T, ACTOR_SCALE = np.array([1.8, 1.2, 1.0]), 0.3
POINT_BIT = 0x80000000


def views():
    """float64 [7,4,4] camera-to-world: raster_scene's six and the tie view."""
    return np.concatenate([R.views(), R.look(*TIE_VIEW)[None]], 0)


def vertex_normals(v, f):
    """Mesher.vertex_normals in numpy: area-weighted face normals summed per vertex, normalised; (0, 0, 1) for none."""
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.maximum(ln, 1e-300), np.array([0.0, 0.0, 1.0]))


def meshes():
    """{name: (vertices, faces, colours uint8 [V,3], normals float64 [V,3])}: raster_scene's scene with the box
    lifted (122 faces), and the same plus a 12 x 16 sphere (474 faces: more than one 256-thread block)."""
    v1, f1 = R.scene(box_shift=BOX_SHIFT)
    sv, sf = R.sphere_mesh(SPHERE2_C, SPHERE2_R, n_lat=12, n_lon=16)
    v2 = np.concatenate([v1, sv], 0)
    f2 = np.concatenate([f1, sf + len(v1)], 0).astype(np.int32)
    out = {}
    for name, (v, f), seed in (("scene", (v1, f1), 21), ("two_spheres", (v2, f2), 22)):
        col = np.random.default_rng(seed).integers(0, 256, (len(v), 3)).astype(np.uint8)
        out[name] = (v, f, col, vertex_normals(v, f))
    return out


def actor_points(scale=ACTOR_SCALE):
    """replay.camera_actor's 1200 points, restated (viz.py:14-42)."""
    cp = scale * np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5],
                           [0.5, 1, 1.5], [0, 1.2, 1.5]], dtype=np.float64)
    lines = [[1, 2], [2, 3], [3, 4], [4, 1], [1, 3], [2, 4], [1, 0], [0, 2], [3, 0], [0, 4], [5, 7], [7, 6]]
    t = np.linspace(0.0, 1.0, 100)
    return np.concatenate([cp[a][None] * (1.0 - t)[:, None] + cp[b][None] * t[:, None] for a, b in lines])


def point_set():
    """(positions float64 [1211,3], colours uint8): the actor inside the room, a trajectory that leaves the room
    through the y = 0 wall (its last points lie behind that wall), the tie point and one NaN point."""
    rot = R.look((0, 0, 0), (0.4, -1.0, 0.1), (0.0, 0.0, -1.0))[:3, :3]
    actor = actor_points() @ rot.T + ACTOR_POSE_T
    traj = ACTOR_POSE_T + np.linspace(0.0, 1.0, 9)[:, None] * (np.array([2.4, -0.4, 1.0]) - ACTOR_POSE_T)
    p = np.concatenate([actor, traj, TIE_POINT[None], [[np.nan, 1.0, 1.0]]], 0)
    col = np.random.default_rng(23).integers(0, 256, (len(p), 3)).astype(np.uint8)
    return p, col


def w2c_of(c2w):
    """The world-to-camera [3,4] the device is given for a camera-to-world matrix."""
    return np.ascontiguousarray(np.linalg.inv(c2w)[:3, :])


# ------------------------------------------------------------------------------------------------
# faces
# ------------------------------------------------------------------------------------------------
def cast_ids(vertices, faces, c2w, tol, cull="none", H=CAM["H"], W=CAM["W"], fx=CAM["fx"], fy=CAM["fy"],
             cx=CAM["cx"], cy=CAM["cy"], z_near=Z_NEAR, z_far=Z_FAR):
    """raster_scene.cast with ids → (id int64 [H,W] (-1: none), z [H,W] (inf: none), barycentrics [H,W,3] of the
    face's vertices a, b, c, z of the second-nearest accepted hit [H,W]).  Ties go to the lowest face index.
    cull: by the sign of d . ((b - a) x (c - a)) = -det: "back" drops the positive ones, "front" the negative."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = b - a, c - a
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], -1).reshape(-1, 3)
    d = d_cam @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(all="ignore"):
        p = np.cross(d[:, None, :], e2[None, :, :])
        det = (e1[None] * p).sum(-1)
        tv = (o - a)[None]
        bu = (tv * p).sum(-1) / det
        q = np.cross(tv, e1[None])
        bv = (d[:, None, :] * q).sum(-1) / det
        t = (e2[None] * q).sum(-1) / det
        bw = 1.0 - bu - bv
        ok = (det != 0.0) & (bu >= tol) & (bv >= tol) & (bw >= tol) & (t > z_near) & (t <= z_far)
        if cull == "back":
            ok &= det > 0.0
        elif cull == "front":
            ok &= det < 0.0
    t = np.where(ok, t, np.inf)
    order = np.argsort(t, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(t))
    first = order[:, 0]
    z, z2 = t[rows, first], t[rows, order[:, 1]]
    fid = np.where(np.isfinite(z), first, -1)
    bary = np.stack([bw[rows, first], bu[rows, first], bv[rows, first]], -1)
    return fid.reshape(H, W), z.reshape(H, W), bary.reshape(H, W, 3), z2.reshape(H, W)


def face_oracle(vertices, faces, c2w, cull="none", **kw):
    """The caster with +EDGE_TOL (lo) and -EDGE_TOL (hi) → dict(lo, hi = (id, z, bary, z2), decided bool [H,W]):
    decided when both give the same id and z to DECIDED_TOL and the second-nearest accepted hit is farther than
    the nearest by more than SEPARATION * z (which leaves out coplanar and shared-edge ties)."""
    lo = cast_ids(vertices, faces, c2w, EDGE_TOL, cull, **kw)
    hi = cast_ids(vertices, faces, c2w, -EDGE_TOL, cull, **kw)
    both_none = (lo[0] < 0) & (hi[0] < 0)
    with np.errstate(invalid="ignore"):
        same = (lo[0] == hi[0]) & (np.abs(lo[1] - hi[1]) <= DECIDED_TOL)
        apart = (hi[3] - hi[1] > SEPARATION * hi[1]) & (lo[3] - lo[1] > SEPARATION * lo[1])
    return dict(lo=lo, hi=hi, decided=both_none | (same & apart))


def shade(vertices, faces, colours, normals, c2w, fid, bary, ambient=AMBIENT, grey=GREY, fx=CAM["fx"], fy=CAM["fy"],
          cx=CAM["cx"], cy=CAM["cy"]):
    """The head-light rule → float64 [H,W,3] before rounding is applied, rounded half up to uint8: the colours and
    normals of the face's vertices interpolated with the barycentrics, times ambient + (1 - ambient) |n . d| with
    both unit vectors in the world frame; a zero-length normal shades as 1.  Pixels of no face are left 0."""
    H, W = fid.shape
    f = faces[np.maximum(fid, 0)]                                            # [H,W,3]
    col = (np.full((len(vertices), 3), grey, dtype=np.float64) if colours is None else colours.astype(np.float64))
    c = (col[f] * bary[..., None]).sum(2)
    n = (normals[f] * bary[..., None]).sum(2)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], -1) @ c2w[:3, :3].T
    nn, dd = (n * n).sum(-1), (d * d).sum(-1)
    with np.errstate(all="ignore"):
        cosv = np.where(nn > 0, np.abs((n * d).sum(-1)) / (np.sqrt(nn) * np.sqrt(dd)), 1.0)
    cosv = np.minimum(cosv, 1.0)
    out = np.floor(c * (ambient + (1.0 - ambient) * cosv)[..., None] + 0.5)
    out = np.clip(np.nan_to_num(out, nan=0.0), 0, 255).astype(np.uint8)
    out[fid < 0] = 0
    return out


# ------------------------------------------------------------------------------------------------
# points
# ------------------------------------------------------------------------------------------------
def sprites(points, w2c, size, H=CAM["H"], W=CAM["W"], fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"],
            z_near=Z_NEAR, z_far=Z_FAR):
    """The point pass, operation for operation → (z32 float32 [H,W] (inf: none), index int64 [H,W] (-1: none),
    boxes [(x0, x1, y0, y1, clipped)] per drawn point): a finite point with camera z in (z_near, z_far] covers the
    pixel centres px - s/2 <= x < px + s/2 (and y), clipped to the image, at float32(z); the smallest
    (z32, index) wins a pixel."""
    m = np.asarray(w2c, dtype=np.float64)
    z32 = np.full((H, W), np.inf, dtype=np.float32)
    idx = np.full((H, W), -1, dtype=np.int64)
    boxes = {}
    half = size * 0.5
    for i, p in enumerate(np.asarray(points, dtype=np.float64)):
        if not np.isfinite(p).all():
            continue
        c = [((m[r, 0] * p[0] + m[r, 1] * p[1]) + m[r, 2] * p[2]) + m[r, 3] for r in range(3)]
        if not np.isfinite(c).all() or not c[2] > z_near or not c[2] <= z_far:
            continue
        px, py = fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        ux0, ux1 = np.ceil(px - half), np.ceil(px + half) - 1.0
        uy0, uy1 = np.ceil(py - half), np.ceil(py + half) - 1.0
        x0, x1, y0, y1 = max(ux0, 0.0), min(ux1, W - 1.0), max(uy0, 0.0), min(uy1, H - 1.0)
        if not (x0 <= x1 and y0 <= y1):
            continue
        x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
        boxes[i] = (x0, x1, y0, y1, (ux0, ux1, uy0, uy1) != (x0, x1, y0, y1))
        z = np.float32(c[2])
        zs, ids = z32[y0:y1 + 1, x0:x1 + 1], idx[y0:y1 + 1, x0:x1 + 1]
        win = (z < zs) | ((z == zs) & (ids < 0))                            # equal z: the earlier (lower) index stays
        zs[win], ids[win] = z, i
    return z32, idx, boxes


def compose(face, pz32, pidx):
    """One caster's faces (id, z, ...) against the sprites by the key rule → (ids int64 [H,W] in the device's
    encoding, z float64 [H,W] (0: background), point_wins, tie, robust): the smaller (float32 z, id) wins and a
    face's id is below every point's.  robust: the outcome is the same for the face's z times 1 -+ Z_BAND."""
    fid, fz = face[0], face[1]
    has_f, has_p = fid >= 0, pidx >= 0

    def p_wins(scale):
        with np.errstate(all="ignore"):
            f32 = np.where(has_f, fz * scale, np.inf).astype(np.float32)
        return has_p & (~has_f | (pz32 < f32)), has_p & has_f & (pz32 == f32)

    pw, tie = p_wins(1.0)
    (pw_a, tie_a), (pw_b, tie_b) = p_wins(1.0 - Z_BAND), p_wins(1.0 + Z_BAND)
    robust = (pw == pw_a) & (pw == pw_b) & (tie == tie_a) & (tie == tie_b)
    ids = np.where(pw, -2 - pidx, np.where(has_f, fid, -1))
    z = np.where(pw, pz32.astype(np.float64), np.where(has_f, fz, 0.0))
    z = np.where(np.isfinite(z), z, 0.0)
    return ids, z, pw, tie, robust


def expected(mesh, c2w, points=None, point_colours=None, size=4, cull="none", background=BACKGROUND, fo=None):
    """Everything the device should give for one view → dict(ids_lo, ids_hi, z_lo, z_hi, colour uint8 [H,W,3],
    decided, point_wins, point_loses, tie, boxes, point_at, fo).  mesh: (vertices, faces, colours, normals) or
    None; fo: the mesh's face_oracle for this view and cull mode when it is already known."""
    H, W = CAM["H"], CAM["W"]
    if fo is not None:
        pass
    elif mesh is not None and len(mesh[1]):
        fo = face_oracle(mesh[0], mesh[1], c2w, cull)
    else:
        none = (np.full((H, W), -1), np.full((H, W), np.inf), np.zeros((H, W, 3)), np.full((H, W), np.inf))
        fo = dict(lo=none, hi=none, decided=np.ones((H, W), bool))
    if points is not None and len(points):
        pz32, pidx, boxes = sprites(points, w2c_of(c2w), size)
    else:
        pz32, pidx, boxes = np.full((H, W), np.inf, np.float32), np.full((H, W), -1), {}
    ids_lo, z_lo, pw, tie, robust = compose(fo["lo"], pz32, pidx)
    ids_hi, z_hi, _, _, robust_hi = compose(fo["hi"], pz32, pidx)
    decided = fo["decided"] & robust & robust_hi
    colour = np.empty((H, W, 3), dtype=np.uint8)
    colour[:] = np.array(background, dtype=np.uint8)
    if mesh is not None and len(mesh[1]):
        sh = shade(mesh[0], mesh[1], mesh[2], mesh[3], c2w, fo["lo"][0], fo["lo"][2])
        face_px = ids_lo >= 0
        colour[face_px] = sh[face_px]
    if pw.any():
        colour[pw] = point_colours[pidx[pw]]
    return dict(ids_lo=ids_lo, ids_hi=ids_hi, z_lo=z_lo, z_hi=z_hi, colour=colour, decided=decided, point_wins=pw,
                point_loses=(pidx >= 0) & ~pw & ~tie, tie=tie, boxes=boxes, point_at=pidx, fo=fo)


# ------------------------------------------------------------------------------------------------
# the culling scene
# ------------------------------------------------------------------------------------------------
def outward_box():
    """(vertices, faces, colours, normals): raster_scene's box with every face wound so that its right-hand normal
    points out of it, over a floor quad whose normal points up; seen from CULL_VIEW every nearest hit is a front."""
    bv, bf = eval_scene.box_mesh(R.BOX_LO + np.array(BOX_SHIFT), R.BOX_HI + np.array(BOX_SHIFT))
    centre = bv.mean(0)
    n = np.cross(bv[bf[:, 1]] - bv[bf[:, 0]], bv[bf[:, 2]] - bv[bf[:, 0]])
    inward = (n * (bv[bf].mean(1) - centre)).sum(1) < 0
    bf = np.where(inward[:, None], bf[:, ::-1], bf)
    fv = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [3.0, 2.5, 0.0], [0.0, 2.5, 0.0]])
    ff = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32) + len(bv)
    v = np.concatenate([bv, fv], 0)
    f = np.concatenate([bf, ff], 0).astype(np.int32)
    col = np.random.default_rng(24).integers(0, 256, (len(v), 3)).astype(np.uint8)
    return v, f, col, vertex_normals(v, f)


CULL_VIEW = ((2.2, 2.3, 1.6), (-1.0, -1.1, -0.6), (0.0, 0.0, -1.0))
