"""Rendering-quality metrics, csrc/nslam_metrics.hip: the sums behind PSNR and depth L1, SSIM and MS-SSIM means."""
import ctypes
import math

import torch

from .._lib import check, lib, ptr, stream_ptr
from ._check import _want

SSIM_WIN = 11          # taps of the Gaussian window (sigma 1.5)
SSIM_TILE = 32         # outputs per side of one workgroup's tile (csrc/nslam_metrics.hip kTile)
MS_SSIM_LEVELS = 5
MS_SSIM_MIN_SIDE = 161  # five levels need min(H, W) > 160
MASK_MODES = {"none": 0, "depth": 1}


def ssim_window():
    """The window as the float32 values the kernel multiplies with: exp(-(i-5)²/(2·1.5²)) / Σ, in float64, rounded."""
    g = [math.exp(-((i - SSIM_WIN // 2) ** 2) / (2.0 * 1.5 ** 2)) for i in range(SSIM_WIN)]
    total = math.fsum(g)
    return (ctypes.c_float * SSIM_WIN)(*[v / total for v in g])


def _image_pair(fn, a, b, names, c_dims):
    """Both of a pair or neither; float32 [B,H,W(,C)] each, of one shape."""
    if (a is None) != (b is None):
        raise ValueError(f"{fn}: {names[0]} and {names[1]} come as a pair")
    if a is None:
        return None
    shape = (None, None, None) + ((c_dims,) if c_dims else ())
    _want(a, names[0], torch.float32, shape)
    _want(b, names[1], torch.float32, tuple(a.shape))
    return tuple(a.shape)


def image_errors(color=None, gt_color=None, depth=None, gt_depth=None, mask="none", clamp=True):
    """nslam_image_errors → float64 [B,4] on the device (no host synchronisation): Σ(color − gt_color)² over the
    counted colour values (colour clamped to [0,1] first when `clamp`), their number, Σ|depth − gt_depth| over
    the pixels with gt_depth > 0, their number.

    color, gt_color float32 [B,H,W,C], C = 1 or 3; depth, gt_depth float32 [B,H,W]; either pair may be None (gt_depth
    alone may come with the colours, as their mask).  mask: "none" counts every pixel for the colour error,
    "depth" only those with gt_depth > 0."""
    if mask not in MASK_MODES:
        raise ValueError(f"image_errors: mask must be one of {sorted(MASK_MODES)}, got {mask!r}")
    cs = _image_pair("image_errors", color, gt_color, ("color", "gt_color"), (1, 3))
    if depth is None and gt_depth is not None:
        _want(gt_depth, "gt_depth", torch.float32, (None, None, None))
        ds = tuple(gt_depth.shape)
    else:
        ds = _image_pair("image_errors", depth, gt_depth, ("depth", "gt_depth"), None)
    if cs is None and depth is None:
        raise ValueError("image_errors: neither a colour pair nor a depth pair")
    if cs is not None and ds is not None and cs[:3] != ds:
        raise ValueError(f"image_errors: colour images {list(cs[:3])} and depth images {list(ds)} differ in shape")
    if mask == "depth" and cs is not None and gt_depth is None:
        raise ValueError("image_errors: mask='depth' needs gt_depth")
    shp = cs if cs is not None else ds
    b, n_pix, ch = int(shp[0]), int(shp[1]) * int(shp[2]), (int(cs[3]) if cs is not None else 1)
    if n_pix == 0:
        raise ValueError("image_errors: the images have no pixels")
    dev = (color if color is not None else gt_depth).device
    out = torch.empty(b, 4, dtype=torch.float64, device=dev)
    if b == 0:
        return out
    ws = torch.empty(lib().nslam_image_errors_workspace_size(b, n_pix), dtype=torch.uint8, device=dev)
    rc = lib().nslam_image_errors(ptr(color), ptr(gt_color), ptr(depth), ptr(gt_depth), b, n_pix, ch,
                                  MASK_MODES[mask], int(bool(clamp)), ptr(out), ptr(ws), ws.numel(), stream_ptr(dev))
    check(rc, "nslam_image_errors")
    return out


def ssim(x, y, data_range=1.0, levels=1):
    """nslam_ssim → float64 [B,levels,C,2] on the device (no host synchronisation): per image, level and channel the
    spatial means of the SSIM map and of the CS map (DESIGN §7j has the definition).

    x, y float32 [B,H,W,C], C = 1 or 3.  levels 1 (min(H,W) >= 11) or 5 (min(H,W) > 160: the last level still
    holds a window)."""
    levels = int(levels)
    if levels not in (1, MS_SSIM_LEVELS):
        raise ValueError(f"ssim: levels must be 1 or {MS_SSIM_LEVELS}, got {levels}")
    if not float(data_range) > 0.0:
        raise ValueError("ssim: data_range must be positive")
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or int(x.shape[3]) not in (1, 3):
        raise ValueError("ssim: x must be [B,H,W,C] with C = 1 or 3")
    b, h, w, c = (int(v) for v in x.shape)
    need = SSIM_WIN if levels == 1 else MS_SSIM_MIN_SIDE
    if min(h, w) < need:
        raise ValueError(f"ssim: levels={levels} needs sides of at least {need}, got {h} x {w}")
    _want(x, "x", torch.float32, (b, h, w, c))
    _want(y, "y", torch.float32, (b, h, w, c))
    out = torch.empty(b, levels, c, 2, dtype=torch.float64, device=x.device)
    if b == 0:
        return out
    ws = torch.empty(lib().nslam_ssim_workspace_size(b, h, w, c, levels), dtype=torch.uint8, device=x.device)
    rc = lib().nslam_ssim(ptr(x), ptr(y), b, h, w, c, float(data_range), ssim_window(), levels, ptr(out), ptr(ws),
                          ws.numel(), stream_ptr(x.device))
    check(rc, "nslam_ssim")
    return out
