"""The layout of the ops package (no GPU calls): every public name resolves on ops, and the two switches that
other code assigns on the package (ops.TIMER, ops.SPLIT_FWD) reach the submodules that read them."""
import importlib
import inspect
import pkgutil

# every public top-level name ops.py defined before it became a package (dir() of that module, its imports left
# out), and the public spellings of the seven names that were used from outside under a leading underscore
SURFACE = (
    "CAM_GRAD_WS_DOUBLES", "CULL_MODES", "FusedAdam", "KernelTimer", "NNGrid", "NN_MAX_CELLS", "NN_PER_CELL",
    "PixelDraws", "QueryMeta", "RASTER_ALL", "RASTER_BIG", "RASTER_CLEAR", "RASTER_MAX_VIEWS", "RASTER_RESOLVE",
    "RASTER_SMALL", "RASTER_SMALL_MAX_PIXELS", "RASTER_WS_BYTES", "SCENE_ALL", "SCENE_MAX_POINT_SIZE", "SCENE_POINTS",
    "SPLIT_FWD", "TIMER", "cam_grad", "cam_grad_batch", "cam_grad_parts", "cam_grad_step", "cam_pose",
    "cam_pose_batch", "cam_vector_batch", "capture", "channels_last", "composite", "composite_density", "depth_l1",
    "depth_maps", "face_areas", "frustum_seen", "gather_rays", "grid_sample", "grid_sample_bwd", "grid_sample_fwd",
    "icp_sums", "imap_params", "imap_query", "imap_query_rays", "kabsch_sums", "loss_sum_best", "marching_cubes",
    "mesh_components", "mesh_face_cull", "mesh_keep_components", "nn_cell_grid", "point_masks", "points_in_hull",
    "query_decoder", "query_fwd_launch", "query_points", "raster_list_length", "raster_workspace", "render_depth",
    "render_loss", "render_scene", "rows_pack", "rows_unpack", "sample_importance", "sample_surface", "sample_z",
    "scene_workspace", "transform_points", "tsdf_block_range", "tsdf_integrate", "tsdf_marching_cubes",
    "tsdf_raycast", "tsdf_touch", "undistort_u8", "views_see_any", "vis_panels",
    "DEC_FOR_STAGE", "DEC_ID", "span", "bound_list", "fill_cfg", "imap_struct", "imap_query_struct",
)
# the names the rest of the package, the bench, the tools and the tests are known to use
USED_OUTSIDE = (
    "FusedAdam", "sample_z", "gather_rays", "composite", "composite_density", "TIMER", "KernelTimer", "SPLIT_FWD",
    "capture", "cam_pose", "cam_pose_batch", "cam_vector_batch", "cam_grad", "cam_grad_parts", "cam_grad_batch",
    "cam_grad_step", "CAM_GRAD_WS_DOUBLES", "loss_sum_best", "NNGrid", "nn_cell_grid", "NN_MAX_CELLS", "render_depth",
    "render_scene", "raster_workspace", "raster_list_length", "scene_workspace", "RASTER_CLEAR", "RASTER_SMALL",
    "RASTER_BIG", "RASTER_RESOLVE", "RASTER_WS_BYTES", "RASTER_SMALL_MAX_PIXELS", "SCENE_POINTS", "CULL_MODES",
    "PixelDraws", "undistort_u8", "vis_panels", "render_loss", "points_in_hull", "point_masks", "marching_cubes",
    "mesh_face_cull", "mesh_components", "mesh_keep_components", "imap_params", "imap_query", "imap_query_rays",
    "sample_importance", "depth_l1", "views_see_any", "transform_points", "kabsch_sums", "frustum_seen", "face_areas",
    "sample_surface", "rows_pack", "rows_unpack", "query_points", "query_decoder", "query_fwd_launch", "QueryMeta",
    "channels_last", "grid_sample", "grid_sample_fwd", "tsdf_block_range", "tsdf_touch", "tsdf_integrate",
    "tsdf_marching_cubes", "tsdf_raycast", "depth_maps", "icp_sums",
)
OLD_SPELLINGS = ("_DEC_FOR_STAGE", "_DEC_ID", "_span", "_bound_list", "_fill_cfg", "_imap_struct",
                 "_imap_query_struct")
SWITCHES = ("TIMER", "SPLIT_FWD")


def _submodules(ops):
    return [importlib.import_module(f"{ops.__name__}.{m.name}") for m in pkgutil.iter_modules(ops.__path__)]


def test_surface(pkg):
    """Every public name resolves as ops.<name>; a submodule that holds the name holds the same object; no
    submodule holds a copy of a switch; no alias of an old spelling is left."""
    ops = pkg.ops
    assert len(set(SURFACE)) == len(SURFACE) == 77 + 7
    assert set(USED_OUTSIDE) <= set(SURFACE)
    subs = _submodules(ops)
    assert len(subs) >= 10
    for name in SURFACE:
        assert hasattr(ops, name), name
        for sub in subs:
            if hasattr(sub, name):
                assert name not in SWITCHES, (sub.__name__, name)
                assert getattr(sub, name) is getattr(ops, name), (sub.__name__, name)
    for name in OLD_SPELLINGS:
        for mod in [ops] + subs:
            assert not hasattr(mod, name), (mod.__name__, name)


def test_timer_reaches_every_module(pkg):
    """span is the package's one function in every submodule that opens spans, and it reads ops.TIMER when
    called."""
    ops = pkg.ops
    users = [sub for sub in _submodules(ops) if "span(" in inspect.getsource(sub)]
    assert {"query", "composite", "mapping", "camera"} <= {sub.__name__.rsplit(".", 1)[1] for sub in users}
    for sub in users:
        assert sub.span is ops.span, sub.__name__

    class Recorder:
        def __init__(self):
            self.names = []

        def span(self, name):
            self.names.append(name)
            return ("span of", self, name)

    saved = ops.TIMER
    try:
        rec = ops.TIMER = Recorder()
        assert ops.span("x") == ("span of", rec, "x") and rec.names == ["x"]
        ops.TIMER = None
        nothing = ops.span("y")
        assert nothing is ops.span("z") and rec.names == ["x"]
        with nothing:  # the no-op: enters and leaves, swallows nothing
            pass
        try:
            with nothing:
                raise KeyError("passes through")
        except KeyError:
            pass
        else:
            raise AssertionError("the no-op span swallowed an exception")
    finally:
        ops.TIMER = saved


def test_split_fwd_reaches_the_launch(pkg, monkeypatch):
    """query_fwd_launch reads ops.SPLIT_FWD when it is called: assigning the switch on the package chooses
    between nslam_query_fwd_ws and nslam_query_fwd, and an explicit split overrides it."""
    import torch
    ops, query = pkg.ops, pkg.ops.query
    calls = []

    class FakeLib:
        def nslam_query_fwd_workspace_size(self, cfg, n):
            return 64

        def nslam_query_fwd_ws(self, *args):
            calls.append("nslam_query_fwd_ws")
            return 0

        def nslam_query_fwd(self, *args):
            calls.append("nslam_query_fwd")
            return 0

    fake = FakeLib()
    monkeypatch.setattr(query, "lib", lambda: fake)
    monkeypatch.setattr(query, "ptr", lambda t: 0)
    monkeypatch.setattr(query, "stream_ptr", lambda device=None: 0)
    monkeypatch.setattr(ops, "TIMER", None)
    cfg = pkg._lib.NslamQueryCfg()
    pts, raw = torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 4)

    monkeypatch.setattr(ops, "SPLIT_FWD", True)
    query.query_fwd_launch(cfg, pts, 8, raw)
    assert calls == ["nslam_query_fwd_ws"]
    ops.SPLIT_FWD = False  # a plain assignment on the package, as the tests and probes that switch it do
    query.query_fwd_launch(cfg, pts, 8, raw)
    assert calls == ["nslam_query_fwd_ws", "nslam_query_fwd"]
    query.query_fwd_launch(cfg, pts, 8, raw, split=True)
    assert calls == ["nslam_query_fwd_ws", "nslam_query_fwd", "nslam_query_fwd_ws"]
    ops.SPLIT_FWD = True
    query.query_fwd_launch(cfg, pts, 8, raw, split=False)
    assert calls[3:] == ["nslam_query_fwd"]
