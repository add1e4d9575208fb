"""Mesher with the reference's call surface (src/utils/Mesher.py), on the HIP kernels of csrc/nslam_mesh.hip.

get_mesh = lattice points (get_grid_uniform) → seen / forecast / unseen masks (nslam_point_masks) or the
convex-hull test (nslam_points_in_hull) → occupancy logits of the lattice (eval_points, the fused query
kernel) → marching cubes (nslam_mc_count / nslam_mc_emit) → face culling and connected components
(nslam_mesh_face_cull / nslam_mesh_components) → vertex colours (eval_points, colour stage) → a binary PLY
written here.  Torch does allocation, cumsum, boolean indexing and batching only; skimage, trimesh and open3d
are not imported.

Deviations from the reference, all stated in DESIGN.md §7a:
  * get_bound_from_frames has two methods, chosen by meshing.bound_from: 'points' (the default) back-projects
    the keyframe depths directly on the host; 'tsdf' fuses them into a TSDF volume on the device first, as the
    reference does with open3d (tsdf.TSDFVolume, a restatement: parity with open3d itself is unpinned, §7h).
    Either way the hull comes back as half-spaces [M,4] (float64) rather than a trimesh object;
  * the hull test is a half-space test, trimesh's `contains` a ray test;
  * trimesh's vertex merging on construction (process=True) is not reproduced: the mesh is already indexed;
  * 'render_ray_along_normal' (iMAP*'s colour mode, Mesher.py:526-553) is implemented for nice=False: the vertex
    normal is the normalised sum of the un-normalised cross products of the vertex's faces, which is believed to
    be open3d's compute_vertex_normals; the library is absent, so that match is unpinned.  With nice=True the
    mode still raises NotImplementedError.
Extensions: get_mesh(..., mesh_bound=planes) skips the hull construction (no scipy needed), and the last
extracted mesh stays on the object as `last_mesh`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


# ------------------------------------------------------------------------------------------------
# PLY (binary little-endian; the vertex / face layout trimesh's exporter writes)
# ------------------------------------------------------------------------------------------------
def write_ply(path, vertices, faces, vertex_colors=None):
    """vertices [V,3] (stored as float32), faces [F,3] (int32), vertex_colors uint8 [V,3] or [V,4] or None."""
    v = np.asarray(vertices)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("write_ply: vertices [V,3] and faces [F,3] expected")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}",
            "property float x", "property float y", "property float z"]
    if vertex_colors is not None:
        c = np.asarray(vertex_colors)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[0] != v.shape[0] or c.shape[1] not in (3, 4):
            raise ValueError("write_ply: vertex_colors must be uint8 [V,3] or [V,4]")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.zeros(v.shape[0], dtype=np.dtype(fields))
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if vertex_colors is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
        vrec["alpha"] = c[:, 3] if c.shape[1] == 4 else 255
    frec = np.zeros(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"] = 3
    frec["i"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """The files write_ply writes → dict(vertices float32 [V,3], faces int32 [F,3], colors uint8 [V,4] or None)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = nf = 0
    props = []
    for ln in lines[2:]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:1] == ["property"] and w[1] != "list" and nf == 0:
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
    names = [p[0] for p in props]
    if names[:3] != ["x", "y", "z"] or names[3:] not in ([], ["red", "green", "blue", "alpha"]):
        raise ValueError(f"{path}: unexpected vertex properties {names}")
    vdt = np.dtype(props)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    vrec = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    frec = np.frombuffer(data, dtype=fdt, count=nf, offset=end + nv * vdt.itemsize)
    if end + nv * vdt.itemsize + nf * fdt.itemsize != len(data) or (nf and not (frec["n"] == 3).all()):
        raise ValueError(f"{path}: size does not match its header")
    colors = None
    if len(names) == 7:
        colors = np.stack([vrec["red"], vrec["green"], vrec["blue"], vrec["alpha"]], 1)
    return {"vertices": np.stack([vrec["x"], vrec["y"], vrec["z"]], 1), "faces": np.array(frec["i"]),
            "colors": colors}


def box_planes(lo, hi):
    """Half-spaces [6,4] (float64, outward normals) of the axis-aligned box lo..hi."""
    rows = []
    for ax in range(3):
        n = [0.0, 0.0, 0.0]
        n[ax] = -1.0
        rows.append(n + [float(lo[ax])])
        n = [0.0, 0.0, 0.0]
        n[ax] = 1.0
        rows.append(n + [-float(hi[ax])])
    return np.array(rows, dtype=np.float64)


class Mesher(object):

    def __init__(self, cfg, args, slam, points_batch_size=500000, ray_batch_size=100000):
        self.points_batch_size = points_batch_size
        self.ray_batch_size = ray_batch_size
        self.renderer = slam.renderer
        self.coarse = cfg["coarse"]
        self.scale = cfg["scale"]
        self.occupancy = cfg["occupancy"]

        m = cfg["meshing"]
        self.resolution = m["resolution"]
        self.level_set = m["level_set"]
        self.clean_mesh_bound_scale = m["clean_mesh_bound_scale"]
        self.remove_small_geometry_threshold = m["remove_small_geometry_threshold"]
        self.color_mesh_extraction_method = m["color_mesh_extraction_method"]
        self.get_largest_components = m["get_largest_components"]
        self.depth_test = m["depth_test"]
        self.bound_from = m.get("bound_from", "points")  # get_bound_from_frames' default method

        self.bound = slam.bound
        self.nice = slam.nice
        self.verbose = slam.verbose

        self.marching_cubes_bound = torch.from_numpy(
            np.array(cfg["mapping"]["marching_cubes_bound"]) * self.scale)
        # the reference also constructs a dataset reader here (Mesher.py:48-49); get_mesh never reads it
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.last_mesh = None

    # -------------------------------------------------------------------------------------------
    def _w2c_and_depth(self, keyframe_dict, estimate_c2w_list, idx, device, use_all):
        """float32 [K,4,4] world-to-camera (np.linalg.inv in the pose's dtype, then float32: Mesher.py:90-92,
        128-130) and the stacked depths [K,H,W] (None with use_all)."""
        if use_all:
            poses = [estimate_c2w_list[i] for i in range(0, int(idx) + 1)]
        else:
            poses = [kf["est_c2w"] for kf in keyframe_dict]
        w2c = [np.linalg.inv(p.detach().cpu().numpy()).astype(np.float32) for p in poses]
        w2c = torch.from_numpy(np.stack(w2c, 0) if w2c else np.zeros((0, 4, 4), np.float32)).to(device)
        depth = None
        if not use_all:
            if keyframe_dict:
                depth = torch.stack([kf["depth"].to(device).float().reshape(self.H, self.W)
                                     for kf in keyframe_dict], 0).contiguous()
            else:
                depth = torch.zeros(0, self.H, self.W, device=device)
        return w2c.contiguous(), depth

    def point_masks_device(self, input_points, keyframe_dict, estimate_c2w_list, idx, device,
                           get_mask_use_all_frames=False):
        """point_masks with the three masks left on the device (bool [N])."""
        if not isinstance(input_points, torch.Tensor):
            input_points = torch.from_numpy(np.asarray(input_points))
        points = input_points.detach().to(device).float().contiguous()
        w2c, depth = self._w2c_and_depth(keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames)
        return ops.point_masks(points, w2c, depth, self.H, self.W, self.fx, self.fy, self.cx, self.cy,
                               self.depth_test, get_mask_use_all_frames, self.points_batch_size)

    def point_masks(self, input_points, keyframe_dict, estimate_c2w_list, idx, device,
                    get_mask_use_all_frames=False):
        """Mesher.point_masks (Mesher.py:53-212) → (seen, forecast, unseen) numpy bool [N].

        In depth_test mode the forecast mask depends on points_batch_size, as in the reference: the depth
        bound is the largest sample over the points of one batch (Mesher.py:166)."""
        s, f, u = self.point_masks_device(input_points, keyframe_dict, estimate_c2w_list, idx, device,
                                          get_mask_use_all_frames)
        return s.cpu().numpy(), f.cpu().numpy(), u.cpu().numpy()

    def get_bound_from_frames(self, keyframe_dict, scale=1, stride=8, method=None, device=None):
        """The convex hull that bounds the mesh, scaled about its centre by clean_mesh_bound_scale → half-spaces
        float64 [M,4] (numpy): a point p is inside when planes @ (p, 1) <= 0.

        method (default: cfg['meshing']['bound_from'], else 'points'):
          'points'  the hull of the keyframes' back-projected depths (every `stride`-th pixel, on the host) and
                    camera centres; `scale` is accepted for signature parity only;
          'tsdf'    the reference's construction (Mesher.py:214-279): the keyframes fused into a TSDF volume
                    with voxel 4 scale / 512 and truncation 0.04 scale on `device` (default: the depths' own
                    device when that is a HIP device, else cuda:0), the hull of the camera centres and the
                    vertices of the volume's mesh; `stride` is not used (the volume samples every 4th pixel).
                    The keyframes' poses are read, never edited."""
        if method is None:
            method = self.bound_from
        if method not in ("points", "tsdf"):
            raise ValueError(f"get_bound_from_frames: unknown method {method!r} (have 'points', 'tsdf')")
        try:
            from scipy.spatial import ConvexHull
        except ImportError as e:
            raise ImportError("Mesher.get_bound_from_frames needs scipy (scipy.spatial.ConvexHull); install "
                              "it, or pass get_mesh(..., mesh_bound=planes)") from e
        if method == "tsdf":
            pts = self._tsdf_hull_points(keyframe_dict, scale, device)
        else:
            pts = self._depth_hull_points(keyframe_dict, stride)
        hull = ConvexHull(pts)
        eq = np.array(hull.equations, dtype=np.float64)  # n . x + d <= 0 inside, |n| = 1
        centre = pts[hull.vertices].mean(0)
        s = float(self.clean_mesh_bound_scale)
        nc = eq[:, :3] @ centre
        eq[:, 3] = s * (nc + eq[:, 3]) - nc  # x' = centre + s (x - centre)
        return eq

    def _depth_hull_points(self, keyframe_dict, stride):
        H, W, fx, fy, cx, cy = self.H, self.W, self.fx, self.fy, self.cx, self.cy
        jj, ii = np.meshgrid(np.arange(0, H, stride, dtype=np.float64), np.arange(0, W, stride, dtype=np.float64),
                             indexing="ij")
        dirs = np.stack([(ii - cx) / fx, -(jj - cy) / fy, -np.ones_like(ii)], -1).reshape(-1, 3)
        pts = []
        for kf in keyframe_dict:
            c2w = kf["est_c2w"].detach().cpu().numpy().astype(np.float64)
            d = kf["depth"].detach().cpu().numpy().astype(np.float64).reshape(H, W)[::stride, ::stride].reshape(-1)
            ok = d > 0
            pts.append((dirs[ok] * d[ok, None]) @ c2w[:3, :3].T + c2w[:3, 3])
            pts.append(c2w[None, :3, 3])
        return np.concatenate(pts, 0)

    def fuse_keyframes(self, keyframe_dict, scale=1, device=None):
        """The keyframes' depths (and colours, when every keyframe has one) fused into a tsdf.TSDFVolume with
        the reference's voxel size 4 scale / 512 and truncation 0.04 scale; None when no depth sample is
        valid.  Poses are converted to the volume's +z-forward convention on copies."""
        from .tsdf import TSDFVolume, opengl_to_cv
        if device is None:
            d0 = keyframe_dict[0]["depth"].device
            device = d0 if d0.type == "cuda" else torch.device("cuda:0")
        H, W, fx, fy, cx, cy = self.H, self.W, self.fx, self.fy, self.cx, self.cy
        c2w = np.stack([opengl_to_cv(kf["est_c2w"]) for kf in keyframe_dict], 0)
        depth = torch.stack([kf["depth"].detach().to(device).float().reshape(H, W) for kf in keyframe_dict],
                            0).contiguous()
        color = None
        if all(kf.get("color") is not None for kf in keyframe_dict):
            color = torch.stack([(kf["color"].detach().to(device).float().reshape(H, W, 3) * 255).to(torch.uint8)
                                 for kf in keyframe_dict], 0).contiguous()
        voxel, trunc = 4.0 * scale / 512.0, 0.04 * scale
        lo, hi, n_valid = TSDFVolume.block_range(depth, c2w, H, W, fx, fy, cx, cy, voxel, trunc)
        if n_valid == 0:
            return None
        vol = TSDFVolume(voxel, trunc, lo, hi, device, color=color is not None)
        vol.integrate(depth, color, c2w, fx, fy, cx, cy)
        return vol

    def _tsdf_hull_points(self, keyframe_dict, scale, device):
        centres = np.stack([kf["est_c2w"].detach().cpu().numpy().astype(np.float64)[:3, 3]
                            for kf in keyframe_dict], 0)
        vol = self.fuse_keyframes(keyframe_dict, scale, device)
        if vol is None:
            return centres
        return np.concatenate([centres, vol.extract_mesh()["vertices"].cpu().numpy()], 0)

    def eval_points(self, p, decoders, c=None, stage="color", device="cuda:0"):
        """Mesher.eval_points (Mesher.py:281-319): raw [N,4] in batches; points outside the bound get logit 100."""
        if p.shape[0] == 0:
            return torch.zeros(0, 4, device=p.device)
        rets = [self.renderer.eval_points(pi, decoders, c, stage, device)
                for pi in torch.split(p, self.points_batch_size)]
        return torch.cat(rets, dim=0)

    @staticmethod
    def vertex_normals(vertices, faces):
        """Unit vertex normals [V,3] float64: the sum over a vertex's faces of (v1 - v0) x (v2 - v0), un-normalised
        (so weighted by area), then normalised; a vertex of no face (or of cancelling faces) gets (0, 0, 1)."""
        v = vertices.double()
        f = faces.long()
        fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
        n = torch.zeros_like(v)
        for k in range(3):
            n.index_add_(0, f[:, k], fn)
        ln = n.norm(dim=1, keepdim=True)
        up = torch.tensor([0.0, 0.0, 1.0], dtype=n.dtype, device=n.device).expand_as(n)
        return torch.where(ln > 0, n / ln.clamp_min(1e-300), up)

    def _colors_along_normal(self, vertices, faces, c, decoders, device, sign=-1.0, length=0.1):
        """Mesher.py:526-553: the colour rendered along each vertex normal, from v - 0.1 n with gt_depth 0.1."""
        normals = self.vertex_normals(vertices, faces)
        rays_d = normals.to(device)
        rays_o = (vertices.double() + sign * length * normals).to(device)
        gt = torch.full((vertices.shape[0],), length, device=device)
        cols = []
        for i in range(0, rays_d.shape[0], self.ray_batch_size):
            _, _, col = self.renderer.render_batch_ray(c, decoders, rays_d[i:i + self.ray_batch_size],
                                                       rays_o[i:i + self.ray_batch_size], device, stage="color",
                                                       gt_depth=gt[i:i + self.ray_batch_size])
            cols.append(col)
        return torch.cat(cols, 0) if cols else torch.zeros(0, 3, device=device)

    def get_grid_uniform(self, resolution):
        """Mesher.get_grid_uniform (Mesher.py:321-347): the lattice in np.meshgrid's default 'xy' order (y is
        the slowest axis of the flattened list) as float32 [R³,3], and the three float64 axes."""
        bound = self.marching_cubes_bound
        padding = 0.05
        x = np.linspace(bound[0][0] - padding, bound[0][1] + padding, resolution)
        y = np.linspace(bound[1][0] - padding, bound[1][1] + padding, resolution)
        z = np.linspace(bound[2][0] - padding, bound[2][1] + padding, resolution)
        xx, yy, zz = np.meshgrid(x, y, z)
        grid_points = torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float)
        return {"grid_points": grid_points, "xyz": [x, y, z]}

    # -------------------------------------------------------------------------------------------
    def _planes(self, mesh_bound, keyframe_dict, device):
        if mesh_bound is None:
            mesh_bound = self.get_bound_from_frames(keyframe_dict, self.scale, device=device)
        if not isinstance(mesh_bound, torch.Tensor):
            mesh_bound = torch.from_numpy(np.asarray(mesh_bound, dtype=np.float64))
        return mesh_bound.to(device=device, dtype=torch.float64).contiguous()

    def get_mesh(self, mesh_out_file, c, decoders, keyframe_dict, estimate_c2w_list, idx, device="cuda:0",
                 show_forecast=False, color=True, clean_mesh=True, get_mask_use_all_frames=False, mesh_bound=None):
        """Mesher.get_mesh (Mesher.py:349-575): extract the mesh and write it to mesh_out_file (binary PLY).

        mesh_bound (extension): half-spaces [M,4] used instead of get_bound_from_frames."""
        along_normal = self.color_mesh_extraction_method == "render_ray_along_normal"
        if color and along_normal and self.nice:
            raise NotImplementedError("'render_ray_along_normal' is iMAP*'s colour mode; the HIP path implements "
                                      "'direct_point_query'")
        if color and not along_normal and self.color_mesh_extraction_method != "direct_point_query":
            raise ValueError(f"unknown color_mesh_extraction_method {self.color_mesh_extraction_method!r}")
        with torch.no_grad():
            grid = self.get_grid_uniform(self.resolution)
            points = grid["grid_points"].to(device).contiguous()  # (the reference's list is a transposed view)
            masks = (keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames)
            planes = None

            if show_forecast:
                seen, forecast, unseen = self.point_masks_device(points, *masks)
                z = torch.zeros(points.shape[0], device=device)
                z[forecast] = self.eval_points(points[forecast], decoders, c, "coarse", device)[:, -1] + 0.2
                z[seen] = self.eval_points(points[seen], decoders, c, "fine", device)[:, -1]
                z[unseen] = -100
            else:
                planes = self._planes(mesh_bound, keyframe_dict, device)
                inside = ops.points_in_hull(points, planes)
                z = self.eval_points(points, decoders, c, "fine", device)[:, -1].float().clone()
                z[~inside] = 100

            x, y, zz = grid["xyz"]
            volume = z.float().reshape(y.shape[0], x.shape[0], zz.shape[0]).permute(1, 0, 2).contiguous()
            spacing = (x[2] - x[1], y[2] - y[1], zz[2] - zz[1])
            # skimage's vertices start at 0; the reference adds the lattice origin afterwards (Mesher.py:466)
            vertices, faces = ops.marching_cubes(volume, self.level_set, (x[0], y[0], zz[0]), spacing)
            if faces.shape[0] == 0:
                print("marching_cubes error. Possibly no surface extracted from the level set.")
                return

            if clean_mesh:
                if show_forecast:
                    planes = self._planes(mesh_bound, keyframe_dict, device)
                    vmask = ~ops.points_in_hull(vertices, planes)
                else:
                    vmask = ~self.point_masks_device(vertices, *masks)[0]
                faces = faces[ops.mesh_face_cull(faces, vmask)].contiguous()
                if faces.shape[0] == 0:
                    print("mesh cleaning removed every face; no mesh written.")
                    return
                thr = self.remove_small_geometry_threshold * self.scale * self.scale
                vertices, faces, _ = ops.mesh_keep_components(vertices, faces, bool(self.get_largest_components), thr)
                if faces.shape[0] == 0:
                    print("mesh cleaning removed every component; no mesh written.")
                    return

            vertex_colors = None
            forecast_v = None
            if color and along_normal and not show_forecast:
                rgb = self._colors_along_normal(vertices, faces, c, decoders, device)
                vertex_colors = (torch.clamp(rgb, 0, 1) * 255).to(torch.uint8)
            elif color:
                rgb = self.eval_points(vertices.float(), decoders, c, "color", device)[..., :3]
                vertex_colors = (torch.clamp(rgb, 0, 1) * 255).to(torch.uint8)
                if show_forecast:  # cyan for the forecast region
                    forecast_v = self.point_masks_device(vertices, *masks)[1]
                    vertex_colors[forecast_v] = torch.tensor([0, 255, 255], dtype=torch.uint8, device=device)

            out_vertices = vertices / self.scale
            self.last_mesh = {"lattice_vertices": vertices, "vertices": out_vertices, "faces": faces,
                              "vertex_colors": vertex_colors, "forecast": forecast_v}
            write_ply(mesh_out_file, out_vertices.cpu().numpy(), faces.cpu().numpy(),
                      None if vertex_colors is None else vertex_colors.cpu().numpy())
            if self.verbose:
                print("Saved mesh at", mesh_out_file)
