"""engine.backward_plan — which backward launches an iteration consists of, on which stream, and who updates
what — against a table written out by hand from the rule it replaces (the planning lines of the former
MappingEngine.query_bwd), and the engine's environment knobs.

m, f, c = middle, fine, color; stream 0 = the caller's, k = the k-th side stream.
"""
import importlib

import pytest

engine = importlib.import_module("nice-slam_amd.engine")

M, F, C = "middle", "fine", "color"
COLOR = dict(decs=(M, F, C), dec_grads=(C,), masks=True, tape=True, n=450)
WG, LEAN3 = ("wgrad", (C,)), ("lean", (M, F, C))

# (case, arguments over COLOR, units, streams, merge_adam)
TABLE = [
    ("colour stage", {}, (WG, LEAN3), (0, 1), True),
    ("wgrad second", dict(wgrad_first=False), (LEAN3, WG), (0, 1), False),
    ("serial", dict(concurrent=False), (WG, LEAN3), (0, 0), False),
    ("ordered (sharded)", dict(ordered=True), (WG, LEAN3), (0, 1), False),
    ("per-branch Adam", dict(adam_merge=False), (WG, LEAN3), (0, 1), False),
    ("no on_branch", dict(has_on_branch=False), (WG, LEAN3), (0, 1), False),
    ("per-decoder launches", dict(merge=False), (("one", (M,)), ("one", (F,)), ("one", (C,))), (0, 1, 2), False),
    ("no points", dict(n=0), (LEAN3,), (0,), False),
    ("no tape", dict(tape=False), (("lean", (M, F)), ("one", (C,))), (0, 1), False),
    ("no masks", dict(masks=False, tape=False), (("one", (M,)), ("one", (F,)), ("one", (C,))), (0, 1, 2), False),
    ("colour stage, frozen (tracking, BA)", dict(dec_grads=()), (LEAN3,), (0,), False),
    ("middle stage", dict(decs=(M,), dec_grads=()), (("lean", (M,)),), (0,), False),
    ("fine stage, fine trainable", dict(decs=(M, F), dec_grads=(F,)), (("lean", (M,)), ("one", (F,))), (0, 1), False),
    ("coarse stage", dict(decs=("coarse",), dec_grads=()), (("lean", ("coarse",)),), (0,), False),
]


@pytest.mark.parametrize("case,over,units,streams,merge_adam", TABLE, ids=[t[0] for t in TABLE])
def test_backward_plan_table(case, over, units, streams, merge_adam):
    kw = dict(COLOR, **over)
    plan = engine.backward_plan(kw.pop("decs"), kw.pop("dec_grads"), **kw)
    assert tuple((k, tuple(n)) for k, n in plan.units) == units
    assert tuple(plan.streams) == streams
    assert plan.has_wgrad is any(k == "wgrad" for k, _ in units)
    assert plan.merge_adam is merge_adam


def test_stage_decoders_are_the_tables():
    """The decs the table passes are the stages' (ops.DEC_FOR_STAGE)."""
    ops = importlib.import_module("nice-slam_amd.ops")
    assert tuple(ops.DEC_FOR_STAGE["color"]) == (M, F, C)
    assert tuple(ops.DEC_FOR_STAGE["fine"]) == (M, F)
    assert tuple(ops.DEC_FOR_STAGE["middle"]) == (M,)
    assert tuple(ops.DEC_FOR_STAGE["coarse"]) == ("coarse",)


@pytest.mark.parametrize("var", ["NSLAM_LIVE_POINTS", "NSLAM_ADAM_MERGE", "NSLAM_WGRAD_FIRST", "NSLAM_PREFETCH_STREAM"])
def test_knobs_reject_unknown_values(monkeypatch, var):
    monkeypatch.setenv(var, "yes")
    with pytest.raises(ValueError, match=var):
        engine.env_knobs()


def test_knob_defaults_and_values(monkeypatch):
    for var in ("NSLAM_LIVE_POINTS", "NSLAM_ADAM_MERGE", "NSLAM_WGRAD_FIRST", "NSLAM_PREFETCH_STREAM"):
        monkeypatch.delenv(var, raising=False)
    default = {"wgrad_first": True, "prefetch_stream": "lean", "adam_merge": True, "live_points": True}
    assert engine.env_knobs() == default
    monkeypatch.setenv("NSLAM_LIVE_POINTS", "0")
    monkeypatch.setenv("NSLAM_PREFETCH_STREAM", "own")
    assert engine.env_knobs() == dict(default, live_points=False, prefetch_stream="own")


def test_retired_variables_do_nothing(monkeypatch):
    for var in ("NSLAM_LIVE_POINTS", "NSLAM_ADAM_MERGE", "NSLAM_WGRAD_FIRST", "NSLAM_PREFETCH_STREAM"):
        monkeypatch.delenv(var, raising=False)
    before = engine.env_knobs()
    monkeypatch.setenv("NSLAM_ADAM_ON", "main")
    monkeypatch.setenv("NSLAM_PREFETCH_AT", "no such place")
    assert engine.env_knobs() == before
    assert sorted(before) == ["adam_merge", "live_points", "prefetch_stream", "wgrad_first"]
