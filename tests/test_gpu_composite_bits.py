"""The ray compositor's outputs bit for bit against the commit before the occupancy / density / loss kernels
were folded into one templated compositor, and the standing invariant that came with it.

  bits       tests/golden/composite_bits.json holds a SHA-256 per output tensor (little-endian bytes of the
             contiguous CPU copy) of every entry point of nslam_composite.hip on the seeded cases of
             ray_edge_cases.py, recorded by tests/golden/make_composite_bits.py with the parent commit's
             library.  Each case is recomputed with the built library and its digests compared for equality.
             The digests pin the toolchain's expf / exp lowering: if a later toolchain changes them, record the
             file again from the then-parent; the comparison stays an equality.
  invariant  nslam_render_loss composites exactly as nslam_composite_fwd: same depth, var and colour in bits,
             with and without occ_add.
"""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest
import torch

import ray_edge_cases as rc

pytestmark = pytest.mark.gpu
P = importlib.import_module("nice-slam_amd")
DEV = torch.device("cuda:0")
BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_bits.json")
NULL_S, DENSITY_NULL_S = 130, 65  # test_composite_bwd_null_cotangents' three chunks; one sample into chunk 1


def dev(t):
    return t.to(DEV) if t is not None else None


def digest(t):
    a = t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).hexdigest()


# Every case returns (got, ref): the kernels' tensors by name, and float64 references for the names that have
# one (only printed on a mismatch, never compared against a bar here).
def composite(S):
    c = rc.composite_case(S)
    raw = dev(c["raw"]).requires_grad_(True)
    depth, var, rgb = P.ops.composite(raw, dev(c["z"]))
    (g_raw,) = torch.autograd.grad((depth, var, rgb), (raw,), [dev(t) for t in c["cots"]])
    return dict(depth=depth, var=var, rgb=rgb, g_raw=g_raw), c["ref"]


def composite_null(which):
    c = rc.composite_case(NULL_S)
    raw, z = dev(c["raw"]), dev(c["z"])
    cots = [dev(t) for t in c["cots"]]  # (held to the end of the call: ptr() does not keep a tensor alive)
    ptrs = [P._lib.ptr(t) if i == which else None for i, t in enumerate(cots)]
    g = torch.full_like(raw, -7.0)
    code = P._lib.lib().nslam_composite_bwd(P._lib.ptr(raw), P._lib.ptr(z), raw.shape[0], raw.shape[1], ptrs[0],
                                            ptrs[1], ptrs[2], P._lib.ptr(g), P._lib.stream_ptr(DEV))
    P._lib.check(code, "nslam_composite_bwd")
    return dict(g_raw=g), {}


def density(S):
    c = rc.density_case(S)
    raw = dev(c["raw"]).requires_grad_(True)
    rd = dev(c["rays_d"]).requires_grad_(True)
    depth, var, rgb, weights = P.ops.composite_density(raw, dev(c["z"]), rd)
    g_raw, g_rd = torch.autograd.grad((depth, var, rgb), (raw, rd), [dev(t) for t in c["cots"]])
    return dict(depth=depth, var=var, rgb=rgb, weights=weights, g_raw=g_raw, g_rays_d=g_rd), c["ref"]


def density_null_weights():
    c = rc.density_case(DENSITY_NULL_S)
    raw, z, rd = dev(c["raw"]), dev(c["z"]), dev(c["rays_d"])
    n, S = z.shape
    depth = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    var, rgb = torch.full_like(depth, -7.0), torch.full((n, 3), -7.0, device=DEV)
    L, ptr = P._lib.lib(), P._lib.ptr
    code = L.nslam_composite_density_fwd(ptr(raw), ptr(z), ptr(rd), n, S, ptr(depth), ptr(var), ptr(rgb), None,
                                         P._lib.stream_ptr(DEV))
    P._lib.check(code, "nslam_composite_density_fwd")
    return dict(depth=depth, var=var, rgb=rgb), c["ref"]


def density_null_g_rays_d():
    c = rc.density_case(DENSITY_NULL_S)
    raw, z, rd = dev(c["raw"]), dev(c["z"]), dev(c["rays_d"])
    n, S = z.shape
    gd, gv, gc = (dev(t) for t in c["cots"])
    g = torch.full_like(raw, -7.0)
    L, ptr = P._lib.lib(), P._lib.ptr
    code = L.nslam_composite_density_bwd(ptr(raw), ptr(z), ptr(rd), n, S, ptr(gd), ptr(gv), ptr(gc), ptr(g), None,
                                         P._lib.stream_ptr(DEV))
    P._lib.check(code, "nslam_composite_density_bwd")
    return dict(g_raw=g), c["ref"]


def run_loss(c, occ_add):
    kind, use_color, hd, w = rc.LOSS_MODES[c["mode"]]
    raw = dev(c["raw_a"] if occ_add else c["raw"])
    occ = dev(c["occ_b"]).contiguous() if occ_add else None
    depth, var, color, ray_loss, g_raw = P.ops.render_loss(raw, dev(c["z"]), dev(c["gt_depth"]), dev(c["gt_color"]),
                                                           dev(c["keep"]), mode=kind, use_color=use_color,
                                                           handle_dynamic=hd, w_color=w, occ_add=occ)
    return dict(depth=depth, var=var, color=color, ray_loss=ray_loss, g_raw=g_raw.reshape(c["raw"].shape))


def loss(S, n, mode, occ_add):
    c = rc.loss_case(S, n, mode)
    return run_loss(c, occ_add), c["ref"]


CASES = {f"composite-S{S}": (composite, (S,)) for S in rc.COMPOSITE_S}
CASES.update({f"composite-S{NULL_S}-only-{name}": (composite_null, (i,))
              for i, name in enumerate(("g_depth", "g_var", "g_color"))})
CASES.update({f"density-S{S}": (density, (S,)) for S in rc.DENSITY_S})
CASES[f"density-S{DENSITY_NULL_S}-no-weights"] = (density_null_weights, ())
CASES[f"density-S{DENSITY_NULL_S}-no-g_rays_d"] = (density_null_g_rays_d, ())
CASES.update({f"loss-S{S}-n{n}-{mode}-{'occ_add' if occ else 'raw'}": (loss, (S, n, mode, occ))
              for S, n in rc.LOSS_CASES for mode in sorted(rc.LOSS_MODES) for occ in (False, True)})


def run_case(name):
    fn, args = CASES[name]
    return fn(*args)


def test_fixture_lists_every_case():
    with open(BITS) as f:
        assert sorted(json.load(f)["digests"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_parent(name):
    with open(BITS) as f:
        want = json.load(f)["digests"][name]
    got, ref = run_case(name)
    have = {k: digest(v) for k, v in got.items()}
    again = None
    for k in sorted(got):
        if have[k] == want.get(k):
            continue
        again = again if again is not None else run_case(name)[0]  # a fresh recomputation: does the run repeat?
        msg = f"{name} {k}: digest differs from the recorded one; a second run "
        msg += "repeats the first" if torch.equal(again[k], got[k]) else \
            f"differs from the first by max-abs {rc.max_abs(again[k].cpu(), got[k].cpu()):.3e}"
        if k in ref:
            msg += f"; max-abs against the float64 reference {rc.max_abs(got[k].cpu(), ref[k]):.3e}"
        print(msg)
    assert have == want, (name, sorted(k for k in set(have) | set(want) if have.get(k) != want.get(k)))


@pytest.mark.parametrize("occ_add", [False, True], ids=["raw", "occ_add"])
def test_render_loss_composites_as_the_compositor(occ_add):
    """nslam_render_loss and nslam_composite_fwd go through one ray_fwd: equal depth, var and colour in bits.
    With occ_add the compositor's fourth channel is raw[..., 3] + occ, formed in float32 on the device."""
    c = rc.loss_case(130, 1030, "mapper_color")
    got = run_loss(c, occ_add)
    raw = dev(c["raw"])
    if occ_add:
        raw = dev(c["raw_a"]).clone()
        raw[..., 3] = raw[..., 3] + dev(c["occ_b"])
    depth, var, color = P.ops.composite(raw, dev(c["z"]))
    assert float(depth.abs().max()) > 0
    assert torch.equal(got["depth"], depth) and torch.equal(got["var"], var) and torch.equal(got["color"], color)
