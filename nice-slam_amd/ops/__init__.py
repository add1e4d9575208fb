"""torch.autograd operators and launch wrappers over libnslam.so (HIP, gfx950): one module per csrc unit, every
public name re-exported here (callers write ops.<name>).  No CPU fallback.

  sampler     nslam_sampler.hip    sample_z, sample_importance
  query       nslam_query.hip      QueryMeta, fill_cfg, query_points, query_decoder, query_fwd_launch, DEC_*
  grid        nslam_grid.hip       channels_last, grid_sample, grid_sample_fwd, grid_sample_bwd
  composite   nslam_composite.hip  composite, composite_density, render_loss
  mapping     nslam_mapping.hip    gather_rays, PixelDraws, rows_pack, rows_unpack, FusedAdam
  camera      nslam_camera.hip     cam_pose*, cam_grad*, cam_vector_batch, loss_sum_best, CAM_GRAD_WS_DOUBLES
  image       nslam_image.hip      undistort_u8
  vis         nslam_vis.hip        vis_panels
  mesh        nslam_mesh.hip       point_masks, marching_cubes, points_in_hull, mesh_*
  evaluation  nslam_eval.hip       frustum_seen, views_see_any, depth_l1, face_areas, sample_surface, NNGrid,
                                   nn_cell_grid, transform_points, kabsch_sums
  raster      nslam_raster.hip     render_depth, render_scene, their workspaces, RASTER_* / SCENE_* / CULL_MODES
  imap        nslam_imap.hip       imap_params, imap_query, imap_query_rays, imap_struct, imap_query_struct
  fusion      nslam_tsdf.hip, nslam_odometry.hip (one block volume)  tsdf_*, depth_maps, icp_sums,
                                   gray_pyramid, photo_sums
  metrics     nslam_metrics.hip    image_errors, ssim, ssim_window, SSIM_* / MS_SSIM_* limits
  _check      the argument checks (_want, _expect) and host conversions (bound_list) they share

Two switches live here and are assigned from outside (ops.TIMER by the bench, ops.SPLIT_FWD by tests): the
submodules read them from this package at call time, through span() and in query_fwd_launch.
The two helpers of hipGraph capture live here too: capture() and GraphCache, the cache the Mapper and the
Tracker keep their graphs in.
"""
import contextlib
import gc

import torch


class KernelTimer:
    """Optional live timing of the C-ABI launches with HIP events on the launching stream.

    ops.TIMER = KernelTimer() turns it on (bench.py does, for the timed region only); each entry
    point records an event pair around its launches; summary() synchronises and averages.
    """

    def __init__(self):
        self.events = {}

    def span(self, name):
        return _Span(self, name)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, pairs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in pairs]
            out[name] = {"calls": len(ms), "avg_ms": sum(ms) / max(len(ms), 1), "total_ms": sum(ms)}
        return out


class _Span:
    def __init__(self, timer, name):
        self.timer, self.name = timer, name

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()
        return self

    def __exit__(self, *exc):
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.timer.events.setdefault(self.name, []).append((self.a, b))
        return False


TIMER = None
_NOSPAN = contextlib.nullcontext()


def span(name):
    return TIMER.span(name) if TIMER is not None else _NOSPAN


@contextlib.contextmanager
def capture(graph):
    """torch.cuda.graph(graph) with the garbage collector out of the way.  torch no longer collects before
    a capture, and an automatic collection inside one may free a dead cycle's device objects (an older
    graph, tensors of its pool) from the capturing thread, which the runtime does not allow while a stream
    captures: the process aborts.  So dead cycles are collected first and none is collected inside."""
    gc.collect()
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            yield
    finally:
        if enabled:
            gc.enable()


class GraphCache(dict):
    """The captured hipGraphs of one owner: plan record -> (graph, what its captured body returned).

    A key is a small frozen record (a namedtuple) whose first field `kind` names what was captured and whose
    other fields are every host value that capture baked into kernel arguments: learning rates, counts,
    image sizes, the draw seed.  The captured body takes the record and reads its host values from nowhere
    else, so a value cannot be baked unless it is in the key; a changed setting is a new key and a new graph,
    never a replay of the old value.  What an engine froze at its construction (sample counts, w_color, the
    tracker's edges) is not in the key: it belongs to the engine's identity, and whoever replaces an engine or
    a buffer that graphs hold by address drops them (drop()).

    graph(key, body, warm, rewind) is the one capture sequence:
      1. `rewind` tensors are cloned.  The draw counter is the usual one: the warm-up draws pixels too, and
         rewinding it makes a call draw the same pixels whether its graph was cached or just captured, and
         the same as the eager path.
      2. warm() runs eagerly.  It is the body with zero learning rates (the maps do not move), so that
         everything made lazily exists before the capture: streams, events, Adam state and tickets, draw
         counters, capacity buffers.  Made during a capture they would come from the graph's private pool
         with their initialisation baked into every replay.
      3. body() is captured under ops.capture (the garbage collector off: see there).  Capturing runs nothing.
      4. the `rewind` tensors are restored and (graph, body's return value) is stored.
    What the warm-up moved that is not a snapshot (the Adam moments it advanced, poses it rewrote) the caller
    resets when `captured` comes back true.

    A graph holds device memory by address, so whatever it reads or writes must outlive it.  Persistent buffers
    belong to the owner; a body returns what nobody else keeps.  The draw state is the case in point: an engine
    caches the PixelDraws of one seed only (MappingEngine.draws), so after a change of seed nothing else would
    hold the counter that the old seed's graph still advances.  Bodies that draw return their PixelDraws, and
    the entry keeps it alive as long as the graph."""

    def graph(self, key, body, warm=None, rewind=()):
        """(graph, body's return value, whether it was captured by this call) of `key`; a hit runs nothing."""
        if key in self:
            return self[key] + (False,)
        saved = [t.clone() for t in rewind]
        if warm is not None:
            warm()
        g = torch.cuda.CUDAGraph()
        with capture(g):
            out = body()
        for t, s in zip(rewind, saved):
            t.copy_(s)
        self[key] = (g, out)
        return g, out, True

    def drop(self, kind=None):
        """Forget the graphs of one kind (all of them: None)."""
        for key in [k for k in self if kind is None or k.kind == kind]:
            del self[key]


SPLIT_FWD = True  # decoder-parallel forward (nslam_query_fwd_ws); False: one wave runs every decoder


# the re-exports, after the switches above: the submodules import span from this package
from ._check import bound_list  # noqa: E402,F401
from .sampler import sample_importance, sample_z  # noqa: E402,F401
from .grid import channels_last, grid_sample, grid_sample_bwd, grid_sample_fwd  # noqa: E402,F401
from .query import (DEC_FOR_STAGE, DEC_ID, QueryMeta, fill_cfg, query_decoder, query_fwd_launch,  # noqa: E402,F401
                    query_points)
from .composite import composite, composite_density, render_loss  # noqa: E402,F401
from .mapping import FusedAdam, PixelDraws, gather_rays, rows_pack, rows_unpack  # noqa: E402,F401
from .camera import (CAM_GRAD_WS_DOUBLES, cam_grad, cam_grad_batch, cam_grad_parts, cam_grad_step,  # noqa: E402,F401
                     cam_pose, cam_pose_batch, cam_vector_batch, loss_sum_best)
from .image import undistort_u8  # noqa: E402,F401
from .vis import vis_panels  # noqa: E402,F401
from .mesh import (marching_cubes, mesh_components, mesh_face_cull, mesh_keep_components,  # noqa: E402,F401
                   point_masks, points_in_hull)
from .raster import (CULL_MODES, RASTER_ALL, RASTER_BIG, RASTER_CLEAR, RASTER_MAX_VIEWS,  # noqa: E402,F401
                     RASTER_RESOLVE, RASTER_SMALL, RASTER_SMALL_MAX_PIXELS, RASTER_WS_BYTES, SCENE_ALL,
                     SCENE_MAX_POINT_SIZE, SCENE_POINTS, raster_list_length, raster_workspace, render_depth,
                     render_scene, scene_workspace)
from .evaluation import (NN_MAX_CELLS, NN_PER_CELL, NNGrid, depth_l1, face_areas, frustum_seen,  # noqa: E402,F401
                         kabsch_sums, nn_cell_grid, sample_surface, transform_points, views_see_any)
from .imap import imap_params, imap_query, imap_query_rays, imap_query_struct, imap_struct  # noqa: E402,F401
from .fusion import (depth_maps, gray_pyramid, icp_sums, photo_sums, tsdf_block_range,  # noqa: E402,F401
                     tsdf_integrate, tsdf_marching_cubes, tsdf_raycast, tsdf_touch)
from .metrics import (MS_SSIM_LEVELS, MS_SSIM_MIN_SIDE, SSIM_TILE, SSIM_WIN, image_errors, ssim,  # noqa: E402,F401
                      ssim_window)
