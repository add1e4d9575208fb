"""The plan records that key the cached hipGraphs (mapper.StagePlan / SetupPlan, tracker.FramePlan) and
ops.GraphCache, on the CPU.

A graph bakes host values into its kernel arguments, so every setting a captured body reads must change the
record that keys the graph.  The tables below name each such setting once: mutating it changes the record, an
equal configuration gives an equal record.  GraphCache is driven with a stub in place of the capture.
"""
import collections
import contextlib
import importlib
from types import SimpleNamespace

import pytest
import torch

P = importlib.import_module("nice-slam_amd")
ops = P.ops


def cfg():
    lrs = lambda d, c, m, f, k: {"decoders_lr": d, "coarse_lr": c, "middle_lr": m, "fine_lr": f, "color_lr": k}  # noqa: E731
    return {
        "coarse": False, "occupancy": True, "scale": 1,
        "tracking": {"lr": 0.001, "device": "cpu", "iters": 3, "gt_camera": False, "pixels": 200, "seperate_LR": False,
                     "w_color_loss": 0.5, "ignore_edge_W": 20, "ignore_edge_H": 20, "handle_dynamic": True,
                     "use_color_in_tracking": True, "const_speed_assumption": True},
        "mapping": {"device": "cpu", "fix_fine": True, "BA_cam_lr": 0.001, "fix_color": False, "pixels": 600, "iters": 6,
                    "w_color_loss": 0.2, "fine_iter_ratio": 0.6, "middle_iter_ratio": 0.4, "mapping_window_size": 5,
                    "frustum_feature_selection": True, "keyframe_selection_method": "overlap",
                    "stage": {"coarse": lrs(0.0, 0.001, 0.0, 0.0, 0.0), "middle": lrs(0.0, 0.0, 0.1, 0.0, 0.0),
                              "fine": lrs(0.0, 0.0, 0.005, 0.005, 0.0), "color": lrs(0.005, 0.0, 0.005, 0.005, 0.005)}},
    }


def slam():
    return SimpleNamespace(nice=True, bound=torch.tensor([[-1.0, 1.0]] * 3), H=96, W=128, fx=60.0, fy=61.0, cx=63.5,
                           cy=47.5, shared_decoders=None, shared_c={}, renderer=None, estimate_c2w_list=None,
                           gt_c2w_list=None, mapping_idx=torch.zeros(1).int())


def window(F=3, n_per=200, c0=1, ncam=2, device_draws=True):
    return SimpleNamespace(F=F, n_per=n_per, c0=c0, ncam=ncam, ar=None if device_draws else torch.arange(4))


def mapper():
    mp = P.Mapper(cfg(), None, slam())
    mp._draw_seed = 1234
    return mp


def tracker():
    tr = P.Tracker(cfg(), None, slam())
    tr._draw_seed = 77
    return tr


def stage_plans(mp, iters=6, lr_factor=1.0, **win):
    return mp._stage_plans(iters, lr_factor, window(**win))


def test_stage_plans_of_the_base_call():
    plans = stage_plans(mapper())
    assert [(p.kind, p.stage, p.iters) for p in plans] == [("stage", "middle", 3), ("stage", "fine", 1),
                                                           ("stage", "color", 2)]
    assert [p.first for p in plans] == [True, False, False]
    assert [p.prefetch for p in plans] == [True, True, False]  # (BA's colour stage draws its rays serially)
    assert [p.cam_lr for p in plans] == [0.0, 0.0, 0.001]       # (the cameras move in the colour stage alone)
    assert plans[2].lrs == (0.005, 0.0, 0.005, 0.005, 0.005) and plans[0].lrs == (0.0, 0.0, 0.1, 0.0, 0.0)
    assert all((p.F, p.n_per, p.c0, p.ncam, p.H, p.W, p.intrinsics, p.seed, p.trainable, p.record)
               == (3, 200, 1, 2, 96, 128, (60.0, 61.0, 63.5, 47.5), 1234, ("color",), False) for p in plans)
    assert stage_plans(mapper()) == plans  # an equal configuration: equal records (and equal hashes)
    assert [hash(p) for p in stage_plans(mapper())] == [hash(p) for p in plans]


def _set(name, value):
    return lambda mp: setattr(mp, name, value)


def _stage_rate(stage, name, value):
    return lambda mp: mp.cfg["mapping"]["stage"][stage].__setitem__(name, value)


# (what changes, how, keyword arguments of the call, the stages whose record must change)
ALL = ("middle", "fine", "color")
STAGE_TABLE = [
    ("iteration count", None, dict(iters=12), ALL),
    ("stage split", _set("middle_iter_ratio", 0.2), {}, ("middle", "fine")),
    ("frames F", None, dict(F=4), ALL),
    ("pixels per frame n_per", None, dict(n_per=150), ALL),
    ("first camera slot c0", None, dict(c0=0), ALL),
    ("camera count ncam", None, dict(ncam=1), ALL),
    ("no BA", None, dict(c0=0, ncam=0), ALL),
    ("lr_factor", None, dict(lr_factor=0.5), ALL),
    ("decoders_lr", _stage_rate("color", "decoders_lr", 0.0025), {}, ("color",)),
    ("coarse_lr", _stage_rate("fine", "coarse_lr", 0.01), {}, ("fine",)),
    ("middle_lr", _stage_rate("middle", "middle_lr", 0.05), {}, ("middle",)),
    ("fine_lr", _stage_rate("fine", "fine_lr", 0.0025), {}, ("fine",)),
    ("color_lr", _stage_rate("color", "color_lr", 0.0025), {}, ("color",)),
    ("BA_cam_lr", _set("BA_cam_lr", 0.0005), {}, ("color",)),
    ("fix_color", _set("fix_color", True), {}, ALL),
    ("fix_fine", _set("fix_fine", False), {}, ALL),
    ("losses recorded", _set("loss_history", []), {}, ALL),
    ("eager draws: no prefetch", None, dict(device_draws=False), ("middle", "fine")),
    ("H", _set("H", 100), {}, ALL),
    ("W", _set("W", 120), {}, ALL),
    ("fx", _set("fx", 59.0), {}, ALL),
    ("fy", _set("fy", 59.0), {}, ALL),
    ("cx", _set("cx", 60.0), {}, ALL),
    ("cy", _set("cy", 40.0), {}, ALL),
    ("draw seed", _set("_draw_seed", 4321), {}, ALL),
]


@pytest.mark.parametrize("what,mutate,kw,changed", STAGE_TABLE, ids=[t[0] for t in STAGE_TABLE])
def test_stage_plan_covers(what, mutate, kw, changed):
    base = {p.stage: p for p in stage_plans(mapper())}
    mp = mapper()
    if mutate is not None:
        mutate(mp)
    got = {p.stage: p for p in stage_plans(mp, **kw)}
    for stage in ALL:
        if stage in changed:
            assert got[stage] != base[stage] and got[stage] not in base.values(), stage
        else:  # (a graph of an untouched stage is reused)
            assert got[stage] == base[stage], stage


def test_stage_plan_first_run_and_coarse():
    plans = stage_plans(mapper(), c0=0, ncam=0)
    assert [p.first for p in plans] == [False] * 3 and [p.prefetch for p in plans] == [True] * 3
    assert all(p.cam_lr == 0.0 for p in plans)
    coarse = P.Mapper(cfg(), None, slam(), coarse_mapper=True)
    plans = coarse._stage_plans(4, 1.0, window(c0=0, ncam=0))
    assert [(p.stage, p.iters, p.lrs) for p in plans] == [("coarse", 4, (0.0, 0.001, 0.0, 0.0, 0.0))]


SETUP_TABLE = [
    ("keyframe count", None, 3),
    ("frustum_feature_selection", _set("frustum_feature_selection", False), 2),
    ("coarse_mapper", _set("coarse_mapper", True), 2),
    ("get_mask_from_c2w hooked", _set("get_mask_from_c2w", lambda *a: None), 2),
    ("fix_color (the optimiser it zeroes)", _set("fix_color", True), 2),
    ("H", _set("H", 100), 2),
    ("fx", _set("fx", 59.0), 2),
]


@pytest.mark.parametrize("what,mutate,n_kf", SETUP_TABLE, ids=[t[0] for t in SETUP_TABLE])
def test_setup_plan_covers(what, mutate, n_kf):
    base = mapper()._setup_plan(2)
    assert base.kind == "setup" and base == mapper()._setup_plan(2)
    assert (base.n_kf, base.frustum, base.coarse, base.hooked) == (2, True, False, False)
    mp = mapper()
    if mutate is not None:
        mutate(mp)
    assert mp._setup_plan(n_kf) != base


FRAME_TABLE = [
    ("iters", _set("num_cam_iters", 4), False),
    ("n", _set("tracking_pixels", 100), False),
    ("speed", None, True),
    ("seperate_LR", _set("seperate_LR", True), False),
    ("cam_lr", _set("cam_lr", 0.0005), False),
    ("draw seed", _set("_draw_seed", 78), False),
]


@pytest.mark.parametrize("what,mutate,speed", FRAME_TABLE, ids=[t[0] for t in FRAME_TABLE])
def test_frame_plan_covers(what, mutate, speed):
    base = tracker()._frame_plan(speed=False)
    assert base == tracker()._frame_plan(speed=False) and hash(base) == hash(tracker()._frame_plan(speed=False))
    assert base == ("frame", 3, 200, False, False, 0.001, None, 77)
    tr = tracker()
    if mutate is not None:
        mutate(tr)
    assert tr._frame_plan(speed=speed) != base


def test_frame_plan_lr_quat_follows_cam_lr():
    tr = tracker()
    tr.seperate_LR = True
    a = tr._frame_plan()
    assert a.lr_quat == 0.001 * 0.2 and P.Tracker._lr2(a) == {"lr_quat": a.lr_quat, "best_before_step": True}
    assert P.Tracker._lr2(a, zero=True) == {"lr_quat": 0.0, "best_before_step": True}
    tr.cam_lr = 0.0005
    b = tr._frame_plan()
    assert b.lr_quat == 0.0005 * 0.2 and b != a
    assert P.Tracker._lr2(tracker()._frame_plan()) == {}


def test_set_stage_lr_reads_the_plan_alone():
    """The rates reach the optimisers from the record (graph and eager alike), zero for the warm-up."""
    mp = mapper()
    plan = stage_plans(mp, lr_factor=0.5)[2]
    opt = SimpleNamespace(param_groups=[{"lr": None} for _ in range(5)])
    win = SimpleNamespace(ncam=2, copt=SimpleNamespace(param_groups=[{"lr": None}]))
    mp.cfg["mapping"]["stage"]["color"]["color_lr"] = 123.0  # (after the plan was made: not read again)
    mp.BA_cam_lr = 456.0
    P.Mapper._set_stage_lr(plan, opt, win)
    assert [g["lr"] for g in opt.param_groups] == [0.0025, 0.0, 0.0025, 0.0025, 0.0025]
    assert win.copt.param_groups[0]["lr"] == 0.001
    P.Mapper._set_stage_lr(plan, opt, win, zero=True)
    assert [g["lr"] for g in opt.param_groups] == [0.0] * 5 and win.copt.param_groups[0]["lr"] == 0.0


def test_shared_predicate(monkeypatch):
    owner = SimpleNamespace(graphs=True, _iter_hook=None, generator=None)
    assert P.common.device_draws(None) and P.common.replays_graphs(owner)
    assert not P.common.replays_graphs(SimpleNamespace(graphs=False, _iter_hook=None, generator=None))
    assert not P.common.replays_graphs(SimpleNamespace(graphs=True, _iter_hook=print, generator=None))
    g = torch.Generator()
    assert not P.common.device_draws(g)
    assert not P.common.replays_graphs(SimpleNamespace(graphs=True, _iter_hook=None, generator=g))
    monkeypatch.setattr(P.common, "select_uv", lambda *a, **k: None)  # pinned draws: eager
    assert not P.common.device_draws(None) and not P.common.replays_graphs(owner)


# -- ops.GraphCache with a stub in place of the capture -------------------------------------------
Key = collections.namedtuple("Key", "kind n")


@pytest.fixture
def stub_capture(monkeypatch):
    log = []

    class Graph:
        pass

    @contextlib.contextmanager
    def capture(graph):
        log.append("capture on")
        yield
        log.append("capture off")

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
    monkeypatch.setattr(ops, "capture", capture)
    return log, Graph


def test_graph_cache_sequence_and_hit(stub_capture):
    log, Graph = stub_capture
    cache = ops.GraphCache()
    ctr = torch.tensor([5])

    def warm():
        log.append("warm")
        ctr.add_(1)  # (the warm-up draws)

    def body():
        log.append("body")
        return "out"

    g, out, captured = cache.graph(Key("stage", 1), body, warm, rewind=[ctr])
    assert isinstance(g, Graph) and out == "out" and captured is True
    assert log == ["warm", "capture on", "body", "capture off"]  # warm before the capture, body inside it
    assert int(ctr) == 5                                           # the snapshot is restored
    assert len(cache) == 1 and cache[Key("stage", 1)] == (g, "out")
    # a hit runs neither the warm-up nor the body
    del log[:]
    g2, out2, captured2 = cache.graph(Key("stage", 1), body, warm, rewind=[ctr])
    assert g2 is g and out2 == "out" and captured2 is False and log == [] and int(ctr) == 5
    # an equal key built anew is the same entry; another key is another graph
    g3, _, c3 = cache.graph(Key("stage", 2), body)
    assert c3 is True and g3 is not g and len(cache) == 2 and log == ["capture on", "body", "capture off"]


def test_graph_cache_drop_and_len(stub_capture):
    cache = ops.GraphCache()
    for key in (Key("stage", 1), Key("stage", 2), Key("setup", 1), Key("frame", 1)):
        cache.graph(key, lambda: None)
    assert len(cache) == 4 and isinstance(cache, dict)
    cache.drop("stage")
    assert sorted(cache) == [Key("frame", 1), Key("setup", 1)] and len(cache) == 2
    cache.drop("no such kind")
    assert len(cache) == 2
    cache.drop()
    assert len(cache) == 0


def test_a_failed_capture_stores_nothing(stub_capture):
    cache = ops.GraphCache()

    def body():
        raise RuntimeError("boom")

    with pytest.raises(RuntimeError, match="boom"):
        cache.graph(Key("stage", 1), body)
    assert len(cache) == 0


def test_mapper_and_tracker_own_a_graph_cache():
    mp, tr = mapper(), tracker()
    assert isinstance(mp._graphs, ops.GraphCache) and isinstance(tr._graphs, ops.GraphCache)
    assert len(mp._graphs) == 0 and len(tr._graphs) == 0
    assert mp._fopt == {}
