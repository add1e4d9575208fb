"""The standalone trilinear lookup of csrc/nslam_grid.hip, and the feature grids' channels-last layout."""
import ctypes

import torch

from . import span
from .._lib import check, lib, ptr, stream_ptr


def channels_last(g: torch.Tensor) -> torch.Tensor:
    """[1,C,Z,Y,X] grid as physically [Z][Y][X][C] (no copy when it already is)."""
    if g.dim() != 5 or g.shape[0] != 1 or g.shape[1] != 32:
        raise ValueError(f"feature grid must be [1,32,Z,Y,X], got {tuple(g.shape)}")
    if g.dtype != torch.float32:
        raise ValueError("feature grids are float32")
    if not g.is_contiguous(memory_format=torch.channels_last_3d):
        g = g.contiguous(memory_format=torch.channels_last_3d)
    return g


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, coords):
        g = channels_last(grid.detach())
        c = coords.detach().float().reshape(-1, 3).contiguous()
        out = torch.empty(c.shape[0], 32, dtype=torch.float32, device=c.device)
        dims = (ctypes.c_int32 * 3)(g.shape[2], g.shape[3], g.shape[4])
        if c.shape[0]:
            check(lib().nslam_grid_sample_fwd(ptr(g), dims, ptr(c), c.shape[0], ptr(out), stream_ptr(c.device)),
                  "nslam_grid_sample_fwd")
        ctx.save_for_backward(g, c)
        return out

    @staticmethod
    def backward(ctx, gout):
        g, c = ctx.saved_tensors
        gg = torch.zeros_like(g, memory_format=torch.channels_last_3d) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        dims = (ctypes.c_int32 * 3)(g.shape[2], g.shape[3], g.shape[4])
        if c.shape[0]:
            check(lib().nslam_grid_sample_bwd(ptr(g), dims, ptr(c), c.shape[0], ptr(gout.contiguous().float()),
                                              ptr(gg), ptr(gc), stream_ptr(c.device)), "nslam_grid_sample_bwd")
        return gg, gc


def grid_sample_fwd(grid, coords, out):
    """nslam_grid_sample_fwd without autograd: out [M,32] = trilinear features of the normalised
    coords [M,3] in a channels-last grid (bench / bulk-query form; grid_sample() is the
    differentiable drop-in)."""
    if not grid.is_contiguous(memory_format=torch.channels_last_3d):
        raise ValueError("grid must be channels-last")
    dims = (ctypes.c_int32 * 3)(grid.shape[2], grid.shape[3], grid.shape[4])
    with span("grid_fwd"):
        rc = lib().nslam_grid_sample_fwd(ptr(grid), dims, ptr(coords), coords.shape[0], ptr(out),
                                         stream_ptr(coords.device))
    check(rc, "nslam_grid_sample_fwd")


def grid_sample_bwd(grid, coords, gout, ggrid, gcoords=None):
    """nslam_grid_sample_bwd without autograd: ggrid += scatter of gout (atomics); gcoords = d/dcoords."""
    dims = (ctypes.c_int32 * 3)(grid.shape[2], grid.shape[3], grid.shape[4])
    with span("grid_bwd"):
        rc = lib().nslam_grid_sample_bwd(ptr(grid), dims, ptr(coords), coords.shape[0], ptr(gout), ptr(ggrid),
                                         ptr(gcoords), stream_ptr(coords.device))
    check(rc, "nslam_grid_sample_bwd")


def grid_sample(grid, coords):
    """[M,32] trilinear features of normalised coords [M,3] (x,y,z) — F.grid_sample semantics."""
    return _GridSample.apply(grid, coords)
