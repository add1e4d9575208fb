"""The evaluation scenes shared by tests/golden/make_golden_eval.py (which records the reference's answers) and
tests/test_gpu_eval.py / tests/test_eval_cpu.py (which replay them): inputs rebuilt from seeds, and the numpy host
restatement of the package's surface sampler (nslam_sample_surface).  Plain numpy.
"""
from __future__ import annotations

import numpy as np

import scenes

ROOM = np.array([4.0, 3.0, 2.5])                     # the room: the box 0..ROOM
CAM = dict(H=48, W=64, fx=40.0, fy=40.0, cx=31.5, cy=23.5)
N_TARGETS, N_QUERIES = 4099, 4096
N_CULL, N_POSES = 4096, 9
CULL_MARGIN = 1e-3       # vertices closer than this to a decision threshold are not compared
CULL_MAX_LEFT_OUT = 0.01
SAMPLE_COUNT, SAMPLE_SEEDS = 5003, (3, 11)
E2E_POINTS, E2E_SEED = 20000, 0
ICP_ANGLE, ICP_SHIFT = np.deg2rad(2.0), np.array([0.02, -0.015, 0.01])

_MASK = (1 << 64) - 1


def wall_points(n, seed, room=ROOM):
    """n points uniform over the six walls of the box 0..room (area-weighted), float64 [n,3]."""
    rng = np.random.default_rng(seed)
    a = np.array([room[1] * room[2], room[1] * room[2], room[0] * room[2], room[0] * room[2],
                  room[0] * room[1], room[0] * room[1]])
    wall = rng.choice(6, size=n, p=a / a.sum())
    p = rng.random((n, 3)) * room
    ax = wall // 2
    p[np.arange(n), ax] = np.where(wall % 2 == 0, 0.0, room[ax])
    return p


def nn_scene():
    """(targets [4099,3], queries [4096,3]): wall points, the queries other wall points plus 1 cm noise."""
    t = wall_points(N_TARGETS, 1)
    q = wall_points(N_QUERIES, 2) + np.random.default_rng(3).normal(0.0, 0.01, (N_QUERIES, 3))
    return t, q


def box_mesh(lo=(0.0, 0.0, 0.0), hi=ROOM, skip_wall=None):
    """The box lo..hi as 8 vertices and 12 triangles (two per wall, wall w = 2 * axis + side); skip_wall leaves
    one wall's two triangles out.  (vertices float64 [8,3], faces int32 [F,3])."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])
    f = []
    for ax in range(3):
        b, c = [a for a in range(3) if a != ax]
        for side in range(2):
            if skip_wall == 2 * ax + side:
                continue
            k0 = side << ax
            q = [k0, k0 | (1 << b), k0 | (1 << b) | (1 << c), k0 | (1 << c)]
            f += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return v, np.array(f, dtype=np.int32)


def sample_mesh():
    """The sampling test's mesh: the room box plus one zero-area face (two of its corners coincide), put in
    the middle of the face list."""
    v, f = box_mesh()
    f = np.concatenate([f[:5], np.array([[0, 1, 1]], dtype=np.int32), f[5:]], 0)
    return v, f


def e2e_meshes():
    """(ground truth, reconstruction): the room box, and the same box shifted 1 cm along x and missing its
    +z wall."""
    gv, gf = box_mesh()
    rv, rf = box_mesh(skip_wall=5)
    return (gv, gf), (rv + np.array([0.01, 0.0, 0.0]), rf)


# ------------------------------------------------------------------------------------------------
# the sampler's host restatement
# ------------------------------------------------------------------------------------------------
def _mix64(x):
    x = np.asarray(x, dtype=np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def uniforms(seed, count, k):
    """Uniform k of samples 0..count-1 in [0,1): (mix64(seed ^ mix64(i * 0x9e3779b97f4a7c15 + k)) >> 11) * 2^-53."""
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64)
        bits = _mix64(np.uint64(int(seed) & _MASK) ^ _mix64(i * np.uint64(0x9e3779b97f4a7c15) + np.uint64(k)))
    return (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def face_cdf(vertices, faces):
    """cumsum of the triangle areas, float64 (the GPU test reads the device's own cdf back instead)."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))


def sample_surface_host(vertices, faces, cdf, count, seed):
    """nslam_sample_surface in numpy → (points float64 [count,3], face_id int32 [count], (u1, u2) after the
    reflection): the face is the first f with cdf[f] > u0 * cdf[-1], the barycentric pair is reflected when
    u1 + u2 > 1, the point is (v0 + u1 (v1 - v0)) + u2 (v2 - v0)."""
    v = np.asarray(vertices, dtype=np.float64)
    cdf = np.asarray(cdf, dtype=np.float64)
    u0, u1, u2 = (uniforms(seed, count, k) for k in range(3))
    fid = np.searchsorted(cdf, u0 * cdf[-1], side="right")
    flip = u1 + u2 > 1.0
    u1, u2 = np.where(flip, 1.0 - u1, u1), np.where(flip, 1.0 - u2, u2)
    t = np.asarray(faces)[fid]
    p, q, r = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    pts = (p + u1[:, None] * (q - p)) + u2[:, None] * (r - p)
    return pts, fid.astype(np.int32), (u1, u2)


# ------------------------------------------------------------------------------------------------
# cull, ICP, ATE scenes
# ------------------------------------------------------------------------------------------------
def cull_scene():
    """(vertices float64 [4096,3] in and around the room, poses float32 [9,4,4]): camera-to-world matrices as
    load_poses returns them (the camera looks down its -z axis)."""
    rng = np.random.default_rng(7)
    v = (rng.random((N_CULL, 3)) * 1.4 - 0.2) * ROOM
    ctr = ROOM / 2
    poses = [scenes.look_pose(ctr, 0.7 * k, 1.2 + 0.1 * (k % 4), (0.3 * ((k % 3) - 1), 0.2 * ((k % 2) - 0.5), 0.05 * k))
             for k in range(N_POSES)]
    return v, np.stack(poses, 0).astype(np.float32)


def icp_scene():
    """(source, target, T): target = 4096 wall points, source = them rotated by 2 degrees about z and shifted by
    (2, -1.5, 1) cm; T (4x4) moves the source back onto the target."""
    dst = wall_points(N_QUERIES, 2)
    c, s = np.cos(ICP_ANGLE), np.sin(ICP_ANGLE)
    r = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    src = dst @ r.T + ICP_SHIFT
    t = np.eye(4)
    t[:3, :3] = r.T
    t[:3, 3] = -r.T @ ICP_SHIFT
    return src, dst, t


def ate_scene(n=50, scale=1.0):
    """(gt c2w float32 [n,4,4], est c2w float32 [n,4,4]): a smooth 3-D curve, the estimate a rigid move of it
    plus 5 mm noise; ground-truth poses 7 and 31 hold NaN / inf.  Translations are multiplied by `scale`."""
    rng = np.random.default_rng(13)
    s = np.linspace(0.0, 1.0, n)
    xyz = np.stack([2.0 * np.cos(2.5 * s), 1.5 * np.sin(3.1 * s), 0.4 * s + 0.2 * np.sin(7.0 * s)], 1)
    gt = np.tile(np.eye(4), (n, 1, 1))
    est = np.tile(np.eye(4), (n, 1, 1))
    a = 0.3
    r = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    gt[:, :3, 3] = xyz * scale
    est[:, :3, 3] = (xyz @ r.T + np.array([0.5, -0.2, 0.1]) + rng.normal(0.0, 0.005, (n, 3))) * scale
    gt[7, 0, 3] = np.nan
    gt[31, 1, 1] = np.inf
    return gt.astype(np.float32), est.astype(np.float32)
