"""The enqueue trace of an engine iteration: which ops.span opens on which stream, in which order.

A recorder stands in for ops.TIMER; every span appends (name, label), label = "main" for the stream current
when the case started and "side0", "side1", ... for the others in order of first appearance.  Callbacks the
engine is given (post_bwd, exchange, allreduce) append an entry of their own the same way.  The expected
traces (tests/golden/engine_traces.json) were recorded by tests/golden/make_engine_traces.py with engine.py
as it was before the backward plan, the launchers and the prefetch ring were split out of query_bwd and
iteration: the split moves no launch to another place or stream.
"""
import copy
import importlib
import json
import os

import pytest
import torch

from conftest import GOLDEN
from test_gpu_dropins import Scene, base_cfg
from test_gpu_fused import _frames, _nice

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
KEYS = ("grid_middle", "grid_fine", "grid_color")
HW = (96, 128)
TRACES = os.path.join(GOLDEN, "engine_traces.json")


class Recorder:
    """ops.TIMER stand-in: span(name) logs (name, stream label) when it opens."""

    def __init__(self):
        self.log = []
        self.labels = {torch.cuda.current_stream(DEV).cuda_stream: "main"}

    def mark(self, name):
        st = torch.cuda.current_stream(DEV).cuda_stream
        if st not in self.labels:
            self.labels[st] = f"side{len(self.labels) - 1}"
        self.log.append([name, self.labels[st]])

    def span(self, name):
        return _Mark(self, name)


class _Mark:
    def __init__(self, rec, name):
        self.rec, self.name = rec, name

    def __enter__(self):
        self.rec.mark(self.name)
        return self

    def __exit__(self, *exc):
        return False


def _mapping(tiny, stage="color", iters=2, pix=False, prefetch=False, bind=False, post_bwd=False, knobs=None,
             exchange=False, allreduce=False):
    sc, frames = _frames(tiny)
    nice, c = _nice(sc)
    eng = P.engine.MappingEngine(nice, c, sc.bound, 32, 16, device=DEV)
    for k, v in (knobs or {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    groups = [{"params": [eng.decs["color"].param], "lr": 0.005}]
    masks = []
    if bind:
        for lo, hi in ((0.0, 0.5), (0.4, 1.0)):  # low-x half, then the high-x part
            m = {}
            for k in KEYS:
                Z, Y, X = c[k].shape[2:]
                x = torch.arange(X, device=DEV)
                m[k] = ((x >= int(X * lo)) & (x < max(1, int(X * hi))))[:, None, None].expand(X, Y, Z).contiguous()
            masks.append(m)
        eng.bind_masks(masks[0])
        for k in KEYS:
            r, nlv = eng.live_rows(k)
            groups.append({"params": [c[k]], "lr": 0.005, "rows": r, "n_live": nlv})
    else:
        groups += [{"params": [c[k]], "lr": 0.005} for k in KEYS]
    opt = P.ops.FusedAdam(groups)
    px = None
    if pix:
        px = torch.randint(HW[0] * HW[1], (3 * 150,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))
    rec = Recorder()
    kw = {}
    if post_bwd:
        kw["post_bwd"] = lambda parts, ro, rd, z: rec.mark("post_bwd")
    if exchange:
        kw["exchange"] = lambda keys, dnames: rec.mark("exchange")
    if allreduce:
        kw["allreduce"] = lambda grads: rec.mark("allreduce")
    P.ops.TIMER = rec
    try:
        for it in range(iters):
            if bind and it == 1:
                eng.bind_masks(masks[1])
            eng.iteration(stage, frames, px, 150, HW, (sc.fx, sc.fy, sc.cx, sc.cy), opt, seed=11, prefetch=prefetch,
                          **kw)
    finally:
        P.ops.TIMER = None
    torch.cuda.synchronize()
    return rec.log


def _tracking(tiny, cam_tail=True, cam_parts=True, lr_quat=None):
    sc = Scene(tiny)
    slam = sc.slam(base_cfg())
    te = P.engine.TrackingEngine(copy.deepcopy(slam.shared_decoders), slam.shared_c, sc.bound, 32, 16, (sc.H, sc.W),
                                 (sc.fx, sc.fy, sc.cx, sc.cy), ignore_edge=(20, 20), w_color=0.5,
                                 handle_dynamic=True, use_color=True, device=DEV)
    te.cam_tail, te.cam_parts = cam_tail, cam_parts
    cam = P.common.get_tensor_from_camera(sc.c2w).cuda().requires_grad_(True)
    opt = P.ops.FusedAdam([{"params": [cam], "lr": 0.001}])
    pix = torch.randint(te.n_window(), (200,), generator=torch.Generator().manual_seed(11)).cuda()
    depth, color = sc.depth.cuda(), sc.color.cuda()
    rec = Recorder()
    P.ops.TIMER = rec
    try:
        for _ in range(2):
            te.iteration(cam, depth, color, pix, opt, lr_quat=lr_quat)
    finally:
        P.ops.TIMER = None
    torch.cuda.synchronize()
    return rec.log


CASES = {
    "color_pixels": lambda t: _mapping(t, pix=True),
    "color_prefetch": lambda t: _mapping(t, iters=3, prefetch=True),
    "color_prefetch_bound_rebind": lambda t: _mapping(t, iters=3, prefetch=True, bind=True),
    "color_post_bwd": lambda t: _mapping(t, pix=True, post_bwd=True),
    "middle_prefetch": lambda t: _mapping(t, stage="middle", iters=3, prefetch=True),
    "wgrad_second": lambda t: _mapping(t, iters=3, prefetch=True, knobs={"wgrad_first": False}),
    "serial": lambda t: _mapping(t, iters=3, prefetch=True, knobs={"concurrent": False}),
    "per_decoder": lambda t: _mapping(t, iters=3, prefetch=True, knobs={"merge": False}),
    "branch_adam_own_stream": lambda t: _mapping(t, iters=3, prefetch=True,
                                                 knobs={"adam_merge": False, "prefetch_stream": "own"}),
    "exchange": lambda t: _mapping(t, pix=True, exchange=True),
    "allreduce": lambda t: _mapping(t, pix=True, allreduce=True),
    "track": lambda t: _tracking(t),
    "track_no_tail": lambda t: _tracking(t, cam_tail=False),
    "track_no_parts": lambda t: _tracking(t, cam_parts=False),
    "track_lr_quat": lambda t: _tracking(t, lr_quat=0.0005),
}


@pytest.fixture(scope="module")
def expected():
    with open(TRACES) as f:
        return json.load(f)


def test_every_case_has_a_recorded_trace(expected):
    assert sorted(expected) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_enqueue_trace_unchanged(tiny, expected, case):
    got = CASES[case](tiny)
    want = expected[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: entry {i}: {g} recorded as {w}"
    assert len(got) == len(want)
    assert len({lab for _, lab in got}) >= 1 and any(name == "query_bwd" for name, _ in got)
