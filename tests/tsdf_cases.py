"""Scenes and numpy twins of the TSDF volume (nice-slam_amd/tsdf.py, csrc/nslam_tsdf.hip), shared by
tests/test_tsdf_cpu.py and tests/test_gpu_tsdf.py.  Everything is procedural: nothing is stored.

The contract is the one in include/nslam.h.  It is written twice here: `fuse(..., dtype=np.float64)` (fuse_ref)
carries every quantity in float64, `fuse(..., dtype=np.float32)` (fuse_f32) rounds every operation of the
integration to float32 in the stated order (numpy's elementwise float32 operations are single IEEE
operations: no contraction).  The sample passes (block range, touch) are float64 in the contract, so both twins
share them.  `extract_ref` is marching cubes over given pool arrays in the kernels' output order.

Poses are camera-to-world matrices in the volume's convention (+z forward, y down).  The world origin lies
inside both scenes, so block indices are negative on every axis.
"""
from __future__ import annotations

import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np

from conftest import GOLDEN, REPO

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mesh_scene  # noqa: E402

CAM = mesh_scene.CAM                  # 24 x 32, fx = fy = 15
L = 0.04
TRUNC = 0.12
B = 16.0 * L                          # 0.64 m blocks
STRIDE = 4
DEPTH_TRUNC = 1000.0
PIXEL_MARGIN = 2.5e-4                 # covers 1e-4 px around a pixel edge and around the border tests at 1e-4
SDF_MARGIN = 1e-6
FACE_MARGIN = 1e-9


def _mc_rows():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(REPO, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_table()[0]


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def _pose(R, t):
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = t
    return m


def _pixel_dirs(H, W):
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([(ii - CAM["cx"]) / CAM["fx"], (jj - CAM["cy"]) / CAM["fy"], np.ones_like(ii)], -1)


def _frame(depth, c2w, seed):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=depth.shape + (3,), dtype=np.uint8)
    return SimpleNamespace(depth=np.ascontiguousarray(depth, dtype=np.float32), color=color,
                           c2w=np.asarray(c2w, dtype=np.float64))


WALL_DEPTH = np.float32(1.5)
WALL_ROLL = 0.37
# the camera looks along world +x, rolled about its axis; the wall is the plane x = WALL_X.  A projective TSDF
# scales the distance by the ray length of the pixel a voxel falls into, which differs between the two ends of
# an edge: the interpolated crossing leaves the plane by a b |m0 - m1| / (a m0 + b m1) for ends at distances a
# and b.  The wall is therefore put a = 1.5e-4 behind a plane of voxel centres: with |m0 - m1| / m <= 0.05
# between neighbouring pixels of this camera the crossings stay within 1e-5 of it.
WALL_X = 0.5 * L + 1.5e-4


def wall_scene():
    """One frame: a fronto-parallel wall 1.5 in front of a camera that is rotated (its axis along world +x,
    rolled by 0.37) and translated; the wall cuts the block face x = 0.  → ([frame], plane (n, c): n . p = c)"""
    c, s = np.cos(WALL_ROLL), np.sin(WALL_ROLL)
    R = np.array([[0.0, 0.0, 1.0], [c, -s, 0.0], [s, c, 0.0]])
    t = np.array([WALL_X - float(WALL_DEPTH), 0.13, -0.21])
    depth = np.full((CAM["H"], CAM["W"]), WALL_DEPTH, dtype=np.float32)
    return [_frame(depth, _pose(R, t), 100)], (np.array([1.0, 0.0, 0.0]), t[0] + float(WALL_DEPTH))


CORNER = np.array([-1.0, -0.8, -0.7])          # the room corner: the planes x = -1, y = -0.8, z = -0.7
SPHERE = (np.array([-0.3, -0.2, -0.1]), 0.35)


def _cast(c2w, H, W):
    """z-depth [H,W] float64 of the corner's three planes and the sphere; 0 where a ray hits nothing."""
    d = _pixel_dirs(H, W) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    best = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for ax in range(3):
            tt = (CORNER[ax] - o[ax]) / d[..., ax]
            hit = o + tt[..., None] * d
            ok = (tt > 0) & (hit >= CORNER - 1e-9).all(-1)
            best = np.where(ok & (tt < best), tt, best)
        ctr, r = SPHERE
        oc = o - ctr
        a, b, c = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - r * r
        disc = b * b - 4.0 * a * c
        ts = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / (2.0 * a)
        best = np.where((disc >= 0) & (ts > 0) & (ts < best), ts, best)
    return np.where(np.isfinite(best), best, 0.0)   # the ray direction has z = 1: t is the z-depth


def corner_pose(k):
    """Pose k of the corner scene: cameras in the room looking at the corner, each from its own place."""
    eye = np.array([1.15 + 0.07 * k, 0.85 - 0.05 * (k % 3), 0.95 + 0.04 * ((k * 5) % 7)])
    target = np.array([-0.45 + 0.06 * (k % 4), -0.35 + 0.05 * (k % 5), -0.3 - 0.04 * (k % 3)])
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], 1)
    roll = 0.05 * k
    cr, sr = np.cos(roll), np.sin(roll)
    R = R @ np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    return _pose(R, eye)


def close_frame():
    """A camera 0.25 in front of the wall x = -1, looking at it: the blocks its samples touch reach behind it."""
    R = np.array([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])   # columns: right -y, down +z, forward -x
    c2w = _pose(R, np.array([-0.75, 0.3, 0.2]))
    return _frame(_cast(c2w, CAM["H"], CAM["W"]).astype(np.float32), c2w, 300)


def corner_frames(n=3, H=None, W=None, holes=True):
    """n frames of the room corner with the sphere (H x W crops of the camera's image, same intrinsics).  With
    `holes`, frame k gets a zero, a NaN and a depth above DEPTH_TRUNC, at strided pixels and between them."""
    H, W = H or CAM["H"], W or CAM["W"]
    out = []
    for k in range(n):
        c2w = corner_pose(k)
        depth = _cast(c2w, H, W).astype(np.float32)
        if holes:
            depth[4, 8 + 4 * (k % 3)] = 0.0
            depth[8, 12] = np.nan
            depth[12, 4 * (k % 5)] = 2000.0
            depth[5, 9] = np.nan
            depth[13, 18 + (k % 4)] = 0.0
            depth[10, 21] = 2000.0
        out.append(_frame(depth, c2w, 200 + k))
    return out


# ------------------------------------------------------------------------------------------------
# passes A and B in float64 (shared by both twins)
# ------------------------------------------------------------------------------------------------
def frame_samples(fr, stride=STRIDE, depth_trunc=DEPTH_TRUNC, trunc=TRUNC, block=B):
    """The valid strided samples of a frame → dict(lo, hi int64 [n,3]: floor((p -+ trunc) / B); face_dist [n]:
    the smallest distance of p -+ trunc to a block face, in world units)."""
    H, W = fr.depth.shape
    v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    d32 = fr.depth[v, u]
    with np.errstate(invalid="ignore"):
        ok = (d32 > 0) & (d32 <= np.float32(depth_trunc))
    u, v, d = u[ok].astype(np.float64), v[ok].astype(np.float64), d32[ok].astype(np.float64)
    x = ((u - CAM["cx"]) * d) / CAM["fx"]
    y = ((v - CAM["cy"]) * d) / CAM["fy"]
    m = fr.c2w
    p = np.stack([((m[c, 0] * x + m[c, 1] * y) + m[c, 2] * d) + m[c, 3] for c in range(3)], 1)
    qlo, qhi = (p - trunc) / block, (p + trunc) / block
    lo, hi = np.floor(qlo).astype(np.int64), np.floor(qhi).astype(np.int64)
    face = np.minimum(np.abs(qlo - np.rint(qlo)), np.abs(qhi - np.rint(qhi))).min(1) * block
    return {"lo": lo, "hi": hi, "face_dist": face, "p": p}


def block_range(frames, **kw):
    """(lo [3], hi [3] exclusive, n_valid) over the frames; (None, None, 0) without a valid sample."""
    s = [frame_samples(fr, **kw) for fr in frames]
    n = sum(x["lo"].shape[0] for x in s)
    if n == 0:
        return None, None, 0
    lo = np.concatenate([x["lo"] for x in s]).min(0)
    hi = np.concatenate([x["hi"] for x in s]).max(0) + 1
    return [int(v) for v in lo], [int(v) for v in hi], n


def touch(frames, lo, hi, **kw):
    """One touch call over <= 32 frames → (mask int64 [cells] in table order, n_outside, margin mask: the
    bits set by samples within FACE_MARGIN of a block face)."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    dims = hi - lo
    mask = np.zeros(int(dims.prod()), dtype=np.int64)
    near = np.zeros_like(mask)
    n_out = 0
    for f, fr in enumerate(frames):
        s = frame_samples(fr, **kw)
        for a, b, fd in zip(s["lo"], s["hi"], s["face_dist"]):
            out = False
            for bx in range(a[0], b[0] + 1):
                for by in range(a[1], b[1] + 1):
                    for bz in range(a[2], b[2] + 1):
                        i = np.array([bx, by, bz]) - lo
                        if (i < 0).any() or (i >= dims).any():
                            out = True
                            continue
                        key = (i[0] * dims[1] + i[1]) * dims[2] + i[2]
                        mask[key] |= 1 << f
                        if fd < FACE_MARGIN:
                            near[key] |= 1 << f
            n_out += int(out)
    return mask, n_out, near


# ------------------------------------------------------------------------------------------------
# pass C twice: dtype float64 (fuse_ref) and float32 in the stated operation order (fuse_f32)
# ------------------------------------------------------------------------------------------------
def _integrate_block(st, pid, coord, fr, w2c32, dtype, color, voxel=L, trunc=TRUNC):
    """One frame into one block; returns (updated bool [4096], margin bool [4096]); st['behind'] and
    st['off_image'] (when present) count the voxels behind the camera and in front of it but outside the image."""
    T = dtype
    H, W = fr.depth.shape
    loc = np.arange(16)
    gx, gy, gz = np.meshgrid(coord[0] * 16 + loc, coord[1] * 16 + loc, coord[2] * 16 + loc, indexing="ij")
    centre = [((g.reshape(-1).astype(np.float64) + 0.5) * voxel).astype(np.float32).astype(T) for g in (gx, gy, gz)]
    M = w2c32.astype(T)
    fx, fy, cx, cy = (T(np.float32(CAM[k])) for k in ("fx", "fy", "cx", "cy"))
    half, one, tr = T(np.float32(0.5)), T(1.0), T(np.float32(trunc))
    e4 = T(np.float32(1e-4))
    cam = [((M[r, 0] * centre[0] + M[r, 1] * centre[1]) + M[r, 2] * centre[2]) + M[r, 3] for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        front = cam[2] > 0
        z = np.where(front, cam[2], one)
        uf = ((cam[0] * fx) / z + cx) + half
        vf = ((cam[1] * fy) / z + cy) + half
        Wf, Hf = T(np.float32(W)) - e4, T(np.float32(H)) - e4
        inside = front & (uf >= e4) & (uf < Wf) & (vf >= e4) & (vf < Hf)
        u = np.where(inside, uf, one).astype(np.int64)
        v = np.where(inside, vf, one).astype(np.int64)
        d32 = fr.depth[v, u]
        valid = inside & (d32 > 0) & (d32 <= np.float32(DEPTH_TRUNC))
        d = np.where(valid, d32, np.float32(1.0)).astype(T)
        xn = (u.astype(np.float32).astype(T) - cx) / fx
        yn = (v.astype(np.float32).astype(T) - cy) / fy
        m = np.sqrt((xn * xn + yn * yn) + one)
        sdf = (d - z) * m
        upd = valid & (sdf > -tr)
        t = np.minimum(one, sdf * (one / tr))
        w = st["weight"][pid]
        w1 = w + one
        st["tsdf"][pid] = np.where(upd, (st["tsdf"][pid] * w + t) / w1, st["tsdf"][pid])
        if color:
            for c in range(3):
                px = fr.color[v, u, c].astype(np.float32).astype(T)
                st["color"][c][pid] = np.where(upd, (st["color"][c][pid] * w + px) / w1, st["color"][c][pid])
        st["weight"][pid] = np.where(upd, w1, w)
        # decisions a float32 rounding could flip (judged on this twin's own values)
        near = front & (np.abs(cam[2]) < 1e-6)
        pix = (np.abs(uf - np.rint(uf)) < PIXEL_MARGIN) | (np.abs(vf - np.rint(vf)) < PIXEL_MARGIN)
        near |= front & pix & (uf > -1) & (uf < W + 1) & (vf > -1) & (vf < H + 1)
        near |= valid & (np.abs(sdf + tr) < SDF_MARGIN)
        near |= np.abs(cam[2]) < 1e-6
    if "behind" in st:
        st["behind"] += int((~front).sum())
        st["off_image"] += int((front & ~inside).sum())
    return upd, near


def fuse(frames, lo, hi, dtype=np.float64, calls=None, color=True, voxel=L, trunc=TRUNC):
    """The volume after integrate calls over `frames` (calls: lists of frame indices, default: 32 at a time).
    → SimpleNamespace(coords int64 [n,3] in pool order, keys [n], table int32 [cells], tsdf / weight [n,4096],
    color [3,n,4096] (or None), n_outside per call, new_blocks per call, margin bool [n,4096]: voxels with a
    decision too close to call, updates: voxel-frame pairs updated, margin_pairs: those too close to call,
    touched: {(pool id, frame index)}, behind / off_image: voxel-frame pairs behind the camera / in front of it
    but outside the image)."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    dims = hi - lo
    if calls is None:
        calls = [list(range(s, min(len(frames), s + 32))) for s in range(0, len(frames), 32)]
    table = np.full(int(dims.prod()), -1, dtype=np.int32)
    st = {"tsdf": [], "weight": [], "color": [[], [], []], "behind": 0, "off_image": 0}
    kw = dict(trunc=trunc, block=16.0 * voxel)
    keys, margin, touched = [], [], set()
    n_outside, new_blocks, updates, margin_pairs = [], [], 0, 0
    for call in calls:
        assert 0 < len(call) <= 32
        mask, n_out, near_face = touch([frames[i] for i in call], lo, hi, **kw)
        n_outside.append(n_out)
        hit = np.flatnonzero(mask)
        fresh = [k for k in hit if table[k] < 0]
        new_blocks.append(len(fresh))
        for k in fresh:
            table[k] = len(keys)
            keys.append(int(k))
            st["tsdf"].append(np.zeros(4096, dtype))
            st["weight"].append(np.zeros(4096, dtype))
            for c in range(3):
                st["color"][c].append(np.zeros(4096, dtype))
            margin.append(np.zeros(4096, bool))
        for k in hit:
            pid = int(table[k])
            coord = np.array([k // (dims[1] * dims[2]), (k // dims[2]) % dims[1], k % dims[2]]) + lo
            for bit, fi in enumerate(call):
                if not (mask[k] >> bit) & 1:
                    continue
                fr = frames[fi]
                w2c32 = np.linalg.inv(fr.c2w).astype(np.float32)
                upd, near = _integrate_block(st, pid, coord, fr, w2c32, dtype, color, voxel, trunc)
                if (near_face[k] >> bit) & 1:
                    near = np.ones(4096, bool)
                touched.add((pid, fi))
                updates += int(upd.sum())
                margin_pairs += int(near.sum())
                margin[pid] |= near
    n = len(keys)
    k = np.array(keys, dtype=np.int64)
    coords = np.stack([k // (dims[1] * dims[2]), (k // dims[2]) % dims[1], k % dims[2]], 1) + lo if n else \
        np.zeros((0, 3), np.int64)
    arr = (lambda x: np.stack(x, 0) if n else np.zeros((0, 4096), dtype))
    return SimpleNamespace(lo=lo, hi=hi, coords=coords, keys=k, table=table, tsdf=arr(st["tsdf"]),
                           weight=arr(st["weight"]),
                           color=np.stack([arr(c) for c in st["color"]], 0) if color else None,
                           n_outside=n_outside, new_blocks=new_blocks, margin=arr(margin).astype(bool),
                           updates=updates, margin_pairs=margin_pairs, touched=touched, behind=st["behind"],
                           off_image=st["off_image"])


def would_update(vol, frames, pid, fi):
    """Would frame fi change block pid of `vol`, had it touched it?"""
    fr = frames[fi]
    st = {"tsdf": [np.zeros(4096)], "weight": [np.zeros(4096)], "color": [[np.zeros(4096)] for _ in range(3)]}
    upd, _ = _integrate_block(st, 0, vol.coords[pid], fr, np.linalg.inv(fr.c2w).astype(np.float32), np.float64, True)
    return bool(upd.any())


def touched_by_0_only(vol, frames):
    """Pool ids of the blocks that only frame 0 touched although frame 1 sees them."""
    others = range(1, len(frames))
    return [pid for pid in range(vol.coords.shape[0])
            if (pid, 0) in vol.touched and not any((pid, f) in vol.touched for f in others)
            and would_update(vol, frames, pid, 1)]


def fuse_ref(frames, lo, hi, **kw):
    return fuse(frames, lo, hi, dtype=np.float64, **kw)


def fuse_f32(frames, lo, hi, **kw):
    return fuse(frames, lo, hi, dtype=np.float32, **kw)


# ------------------------------------------------------------------------------------------------
# pass D
# ------------------------------------------------------------------------------------------------
def edge_faces(e):
    """The two faces (axis, side) of the cell that edge e = axis * 4 + (a + 2 b) lies in."""
    ax, a, b = e >> 2, e & 1, (e >> 1) & 1
    o1, o2 = [x for x in range(3) if x != ax]
    return {(o1, a), (o2, b)}


def row_loops(row):
    """The loops behind a row of the case table, which holds a fan per loop from the loop's first vertex."""
    loops = []
    for t in row:
        if loops and loops[-1][0] == t[0] and loops[-1][-1] == t[1]:
            loops[-1].append(t[2])
        else:
            loops.append(list(t))
    return loops


def refan(row):
    """The row's loops fanned from a vertex whose diagonals all cross the cell's interior (no diagonal shares a
    face of the cell with its apex); of those vertices, the one with the lowest edge id, a choice that does not
    depend on the direction in which the loop is listed: same loops, same count, same winding."""
    tris = []
    for loop in row_loops(row):
        n = len(loop)
        apex = min((c for c in range(n)
                    if not any(edge_faces(loop[c]) & edge_faces(loop[(c + d) % n]) for d in range(2, n - 1))),
                   key=lambda c: loop[c])
        tris += [(loop[apex], loop[(apex + i) % n], loop[(apex + i + 1) % n]) for i in range(1, n - 1)]
    return tris


def extract_ref(tsdf, weight, color, keys, lo, hi, voxel=L):
    """Marching cubes of pool arrays (tsdf, weight float32 [n,4096], color float32 [3,n,4096] or None, keys [n]:
    the blocks' table cells) → dict(vertices float64 [V,3], faces int32 [F,3], colors uint8 [V,3] or None,
    cells: the valid cells' low corners as global voxel indices [C,3], cases [C]), in the kernels' order:
    vertices by (pool voxel, axis), faces by pool voxel of the cell's low corner, the table's loops fanned by
    `refan` with the winding flipped."""
    rows = _mc_rows()
    lo, hi = np.asarray(lo), np.asarray(hi)
    dims = hi - lo
    n = len(keys)
    shape = tuple(int(d) * 16 for d in dims)
    f_d = np.zeros(shape, np.float32)
    w_d = np.zeros(shape, np.float32)
    pidx = np.full(shape, -1, np.int64)
    c_d = np.zeros((3,) + shape, np.float32) if color is not None else None
    for i, k in enumerate(np.asarray(keys, dtype=np.int64)):
        b = np.array([k // (dims[1] * dims[2]), (k // dims[2]) % dims[1], k % dims[2]]) * 16
        sl = tuple(slice(int(v), int(v) + 16) for v in b)
        f_d[sl] = np.asarray(tsdf[i], np.float32).reshape(16, 16, 16)
        w_d[sl] = np.asarray(weight[i], np.float32).reshape(16, 16, 16)
        pidx[sl] = i * 4096 + np.arange(4096).reshape(16, 16, 16)
        if c_d is not None:
            for c in range(3):
                c_d[c][sl] = np.asarray(color[c][i], np.float32).reshape(16, 16, 16)
    ok = (w_d > 0) & (pidx >= 0)
    below = f_d < 0
    nx, ny, nz = shape
    valid = np.ones((nx - 1, ny - 1, nz - 1), bool)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        sl = (slice(dx, nx - 1 + dx), slice(dy, ny - 1 + dy), slice(dz, nz - 1 + dz))
        valid &= ok[sl]
        case |= below[sl].astype(np.int64) << k
    # an owned edge has a vertex when it crosses and one of the (up to four) cells around it is valid
    vpad = np.zeros((nx + 1, ny + 1, nz + 1), bool)     # vpad[i + 1] = valid[i]
    vpad[1:nx, 1:ny, 1:nz] = valid
    vert_id = np.full(shape + (3,), -1, np.int64)
    recs = []
    for ax in range(3):
        o1, o2 = [a for a in range(3) if a != ax]
        around = np.zeros(shape, bool)
        for a in (0, 1):
            for b in (0, 1):
                sl = [slice(1, nx + 1), slice(1, ny + 1), slice(1, nz + 1)]
                sl[o1] = slice(1 - a, shape[o1] + 1 - a)
                sl[o2] = slice(1 - b, shape[o2] + 1 - b)
                around |= vpad[tuple(sl)]
        nb = np.roll(below, -1, axis=ax)
        cross = (below != nb) & around
        idx = np.argwhere(cross)
        for g in idx:
            recs.append((int(pidx[tuple(g)]), ax, tuple(int(v) for v in g)))
    recs.sort()
    verts = np.zeros((len(recs), 3))
    cols = np.zeros((len(recs), 3), np.uint8) if c_d is not None else None
    for i, (_, ax, g) in enumerate(recs):
        h = list(g)
        h[ax] += 1
        h = tuple(h)
        f0, f1 = f_d[g], f_d[h]
        t = np.float32(f0) / (np.float32(f0) - np.float32(f1))
        gg = np.array(g, dtype=np.float64) + lo * 16
        pos = gg + 0.5
        pos[ax] = pos[ax] + float(t)
        verts[i] = pos * voxel
        vert_id[g + (ax,)] = i
        if c_d is not None:
            a0, a1 = np.abs(np.float32(f0)), np.abs(np.float32(f1))
            for c in range(3):
                cv = (a1 * c_d[c][g] + a0 * c_d[c][h]) / (a0 + a1)
                cols[i, c] = np.uint8(min(255.0, max(0.0, np.floor(np.float32(cv) + np.float32(0.5)))))
    cells = np.argwhere(valid)
    order = np.argsort(pidx[tuple(cells.T)], kind="stable") if len(cells) else np.zeros(0, np.int64)
    cells = cells[order]
    faces = []
    for g in cells:
        cs = int(case[tuple(g)])
        for tri in refan(rows[cs]):
            ids = []
            for e in tri:
                ax, ea, eb = e >> 2, e & 1, (e >> 1) & 1
                off = [0, 0, 0]
                o1, o2 = [a for a in range(3) if a != ax]
                off[o1], off[o2] = ea, eb
                ids.append(int(vert_id[tuple(g + np.array(off)) + (ax,)]))
            assert min(ids) >= 0
            faces.append([ids[0], ids[2], ids[1]])
    faces = np.array(faces, dtype=np.int32).reshape(-1, 3)
    return {"vertices": verts, "faces": faces, "colors": cols, "cells": cells + lo * 16,
            "cases": case[tuple(cells.T)] if len(cells) else np.zeros(0, np.int64)}


def face_normals(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return np.cross(b - a, c - a)
