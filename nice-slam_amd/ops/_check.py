"""Argument checks and host-side argument conversions shared by the wrappers (no csrc unit of its own)."""
import ctypes

import torch


def _dims_match(shape, spec):
    """shape against spec, whose entries are a size, None (any size) or a container of the sizes allowed."""
    return len(shape) == len(spec) and all(
        s is None or (d in s if hasattr(s, "__contains__") else int(d) == int(s)) for d, s in zip(shape, spec))


def _on_device(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: nice-slam_amd kernels run on the HIP device only; got a CPU tensor")


def _want(t, name, dtype, shape=None):
    """Dtype / contiguity / shape check of a tensor whose pointer is handed to a kernel."""
    _on_device(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and not _dims_match(t.shape, shape):
        raise ValueError(f"{name}: expected shape {list(shape)}, got {list(t.shape)}")
    return t


def _expect(fn, specs, msg=None):
    """Every (tensor, dtype, shape) of specs is a contiguous tensor of exactly that dtype and shape (entries as
    in _dims_match), else ValueError (fn: the caller's name; msg: its own wording instead of the expected / got
    line)."""
    for t, dt, shp in specs:
        if t.dtype != dt or not t.is_contiguous() or (tuple(t.shape) != tuple(shp) and not _dims_match(t.shape, shp)):
            raise ValueError(f"{fn}: " + (msg or f"expected contiguous {dt} {shp}, got {t.dtype} {tuple(t.shape)}"))


def bound_list(b):
    b = b.detach().to("cpu", torch.float64)
    return [float(v) for v in b[:, 0]], [float(v) for v in b[:, 1]]


def _i3(v, name):
    if len(v) != 3:
        raise ValueError(f"{name}: three block indices expected")
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


def _pose16(m, name):
    """A 4x4 pose (tensor or array) as the HOST float64 [16] the odometry entry points read."""
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().tolist()
    flat = [float(x) for row in m for x in row]
    if len(flat) != 16:
        raise ValueError(f"{name}: a 4x4 matrix expected")
    return (ctypes.c_double * 16)(*flat)


def _face_range(faces, nv, what, past="the vertices"):
    """Every index of faces lies in [0, nv) (one host read of the extremes), else ValueError in what's name."""
    if faces.shape[0] and (nv == 0 or int(faces.max()) >= nv or int(faces.min()) < 0):
        raise ValueError(f"{what}: a face indexes past {past}")


def _want_mesh(vertices, faces, what, vname="vertices"):
    """vertices float64 [V,3] and faces int32 [F,3] indexing them → (V, F)."""
    _want(vertices, vname, torch.float64, (None, 3))
    _want(faces, "faces", torch.int32, (None, 3))
    _face_range(faces, vertices.shape[0], what)
    return vertices.shape[0], faces.shape[0]


def _want_pool(fn, tsdf, weight, color_pool, n_pool):
    """The block pool of a tsdf.TSDFVolume: tsdf / weight [cap,4096], color_pool [3,cap,4096] or None, of
    which the first n_pool blocks are in use → (cap, n_pool)."""
    cap, n_pool = int(tsdf.shape[0]), int(n_pool)
    if not 0 <= n_pool <= cap:
        raise ValueError(f"{fn}: n_pool exceeds the pool's capacity")
    _want(tsdf, "tsdf", torch.float32, (cap, 4096))
    _want(weight, "weight", torch.float32, (cap, 4096))
    if color_pool is not None:
        _want(color_pool, "color_pool", torch.float32, (3, cap, 4096))
    return cap, n_pool


def _want_volume(fn, tsdf, weight, color_pool, pool_key, n_pool, table, block_lo, block_hi):
    """The pool with its keys and the block table over [block_lo, block_hi) → (cap, n_pool, lo, hi, cells)."""
    cap, n_pool = _want_pool(fn, tsdf, weight, color_pool, n_pool)
    _want(pool_key, "pool_key", torch.int32, (None,))
    if int(pool_key.shape[0]) < n_pool:
        raise ValueError(f"{fn}: pool_key is shorter than the pool")
    lo, hi = _i3(block_lo, "block_lo"), _i3(block_hi, "block_hi")
    cells = max(0, hi[0] - lo[0]) * max(0, hi[1] - lo[1]) * max(0, hi[2] - lo[2])
    _want(table, "table", torch.int32, (cells,))
    return cap, n_pool, lo, hi, cells


def _mc_offsets(flags, ntri):
    """The host half of marching cubes: the count pass's per-edge flags and per-cell triangle counts (uint8) →
    (voff, foff, n_verts, n_faces), the exclusive int32 prefix sums the emit pass writes at and their totals
    (one host read); the offsets are None when the surface is empty."""
    vinc = torch.cumsum(flags, 0, dtype=torch.int32)
    finc = torch.cumsum(ntri, 0, dtype=torch.int32)
    n_verts, n_faces = int(vinc[-1]), int(finc[-1])
    if n_verts == 0 and n_faces == 0:
        return None, None, 0, 0
    return (vinc - flags).contiguous(), (finc - ntri).contiguous(), n_verts, n_faces
