"""Lens undistortion, csrc/nslam_image.hip."""
import ctypes

import torch

from .._lib import check, lib, ptr, stream_ptr
from ._check import _expect


def undistort_u8(src, fx, fy, cx, cy, dist, out=None):
    """nslam_undistort_u8: cv2.undistort(src, K, dist) with its defaults (new camera matrix K, bilinear,
    zero border; 1/32-pixel positions, integer weights — include/nslam.h) for a contiguous uint8 device image
    [H, W, C] or [H, W], C in 1..4, and dist = (k1, k2, p1, p2, k3).  One launch on the current stream, no
    host synchronisation.  Returns a new image (or `out`, which may not be src)."""
    _expect("undistort_u8", [(src, torch.uint8, (None, None) + tuple(src.shape[2:3]))],
            "src must be a contiguous uint8 [H, W] or [H, W, C]")
    C = 1 if src.dim() == 2 else src.shape[2]
    dist = [float(v) for v in dist]
    if len(dist) != 5:
        raise ValueError(f"undistort_u8: dist must be (k1, k2, p1, p2, k3), got {len(dist)} coefficients")
    if not 1 <= C <= 4:
        raise ValueError(f"undistort_u8: 1..4 channels, got {C}")
    if out is None:
        out = torch.empty_like(src)
    _expect("undistort_u8", [(out, torch.uint8, src.shape)])
    if out.data_ptr() == src.data_ptr() and src.numel():
        raise ValueError("undistort_u8: out may not alias src")
    if src.numel() == 0:
        return out
    rc = lib().nslam_undistort_u8(ptr(src), src.shape[0], src.shape[1], C, float(fx), float(fy), float(cx), float(cy),
                                  (ctypes.c_double * 5)(*dist), ptr(out), stream_ptr(src.device))
    check(rc, "nslam_undistort_u8")
    return out
