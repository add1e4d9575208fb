"""The live-point entry points reject bad arguments before any launch (no GPU calls)."""
import ctypes


def _colour_cfg(pkg):
    """A colour-stage config with fake (aligned, never dereferenced) device pointers."""
    cfg = pkg._lib.NslamQueryCfg()
    cfg.stage = pkg._lib.STAGES["color"]
    for d in range(4):
        cfg.grid[d].data = 4096
        cfg.grid[d].dims[0] = cfg.grid[d].dims[1] = cfg.grid[d].dims[2] = 8
        cfg.packed[d] = 4096
    return cfg


def test_live_points_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    vp4 = ctypes.c_void_p * 4
    idx, nl = vp4(4096, 4096, 4096, 4096), vp4(4096, 4096, 4096, 4096)
    bad = pkg._lib.NslamQueryCfg()
    bad.stage = 7
    assert L.nslam_live_points(ctypes.byref(bad), 0b1110, 4096, 96, idx, nl, 4096, 1 << 20, None) == -1  # stage
    c = _colour_cfg(pkg)
    need = L.nslam_live_points_workspace_size(96)
    assert need > 0 and L.nslam_live_points_workspace_size(0) == 0
    # 300 points: two 256-point blocks, each with 4 ballots and a count per decoder slot
    assert L.nslam_live_points_workspace_size(300) == 4 * (2 * 4 * 8 + 2 * 4)
    assert L.nslam_live_points(ctypes.byref(c), 0, 4096, 96, idx, nl, 4096, need, None) == -1          # no decoders
    assert L.nslam_live_points(ctypes.byref(c), 1, 4096, 96, idx, nl, 4096, need, None) == -1          # coarse
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, None, 96, idx, nl, 4096, need, None) == -1     # no points
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 1 << 31, idx, nl, 4096, 1 << 40, None) == -1
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 96, None, nl, 4096, need, None) == -1    # no lists
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 96, idx, nl, 4096, need - 1, None) == -3  # short ws
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 96, idx, nl, None, need, None) == -3     # no ws
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 96, idx, nl, 4100, need, None) == -3     # unaligned
    hole = vp4(4096, 4096, None, 4096)
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 96, hole, nl, 4096, need, None) == -1    # a NULL list
    assert L.nslam_live_points(ctypes.byref(c), 0b1110, 4096, 96, idx, hole, 4096, need, None) == -1   # a NULL count


def test_bwd_decoders_live_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    vp4 = ctypes.c_void_p * 4
    idx, nl = vp4(4096, 4096, 4096, 4096), vp4(4096, 4096, 4096, 4096)
    c = _colour_cfg(pkg)
    colour = 1 << pkg._lib.DEC_COLOR
    call = lambda cfg, mask, g=4096, i=idx, n=nl: L.nslam_query_bwd_decoders_live(  # noqa: E731
        ctypes.byref(cfg), mask, 4096, 96, g, i, n, None)
    assert call(c, colour) == -2                    # no saved masks
    c.saved_masks = 4096
    assert call(c, 0) == -1                         # no decoders
    assert call(c, 1 << pkg._lib.DEC_COARSE) == -1  # not a decoder of the stage
    assert call(c, colour, g=None) == -1            # no cotangent
    assert call(c, colour, i=None) == -1            # no lists
    assert call(c, colour, n=vp4()) == -1           # a NULL count
    c.need_pts_grad = 1
    assert call(c, colour) == -2                    # d/dpts needs every point
    c.need_pts_grad = 0
    c.dgrad[pkg._lib.DEC_COLOR].base = 4096
    c.dgrad[pkg._lib.DEC_COLOR].count = 100
    assert call(c, colour) == -2                    # no parameter gradients in the lean launch
    c.dgrad[pkg._lib.DEC_COLOR].base = None
    assert L.nslam_query_bwd_decoders_live(ctypes.byref(c), colour, None, 0, None, idx, nl, None) == 0  # empty batch
