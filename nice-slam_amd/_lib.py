"""ctypes binding of libnslam.so (include/nslam.h).

The product path calls the HIP kernels only through this module.  There is no CPU fallback:
if the shared library is missing, or a tensor is not on a HIP device, the call raises.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NSLAM_LIB") or os.path.join(_HERE, "libnslam.so")  # NSLAM_LIB: instrumented builds

ABI_VERSION = 24

# The named values of include/nslam.h (NSLAM_<name>).  This module is the only place that restates them: the
# rest of the package imports them from here, and tests/test_abi_cpu.py compiles the header and compares each.
NSLAM_OK, NSLAM_EINVAL, NSLAM_EUNSUPPORTED, NSLAM_EWORKSPACE, NSLAM_EHIP = 0, -1, -2, -3, -1000
EMB = 93
STAGES = {"coarse": 0, "middle": 1, "fine": 2, "color": 3}  # NSLAM_STAGE_*
DEC_COARSE, DEC_MIDDLE, DEC_FINE, DEC_COLOR = 0, 1, 2, 3
MAX_FRAMES = 32  # of nslam_gather_rays, the camera batches and the TSDF touch / integrate calls
LOSS_MAPPER, LOSS_TRACKER = 0, 1
ADAM_MAX_SEGS = 16
CAM_GRAD_WS_DOUBLES = 32 * 12
RASTER_CLEAR, RASTER_SMALL, RASTER_BIG, RASTER_RESOLVE, RASTER_ALL = 1, 2, 4, 8, 15
CULL_MODES = {"none": 0, "back": 1, "front": 2}  # NSLAM_CULL_*
SCENE_POINTS, SCENE_ALL = 16, 31


class NslamGrid(ctypes.Structure):
    _fields_ = [
        ("data", ctypes.c_void_p),
        ("grad", ctypes.c_void_p),
        ("dims", ctypes.c_int32 * 3),
        ("pad_", ctypes.c_int32),
        ("lo", ctypes.c_double * 3),
        ("hi", ctypes.c_double * 3),
        ("slot", ctypes.c_void_p),  # ABI v6: frustum-compacted gradient (NULL = dense)
    ]


class NslamDecGrad(ctypes.Structure):
    _fields_ = [
        ("base", ctypes.c_void_p),
        ("w", ctypes.c_int64 * 5),
        ("b", ctypes.c_int64 * 5),
        ("wc", ctypes.c_int64 * 5),
        ("bc", ctypes.c_int64 * 5),
        ("wo", ctypes.c_int64),
        ("bo", ctypes.c_int64),
        ("B", ctypes.c_int64),
        ("count", ctypes.c_int64),
    ]


class NslamQueryCfg(ctypes.Structure):
    _fields_ = [
        ("stage", ctypes.c_int32),
        ("need_pts_grad", ctypes.c_int32),
        ("bound_lo", ctypes.c_double * 3),
        ("bound_hi", ctypes.c_double * 3),
        ("grid", NslamGrid * 4),
        ("packed", ctypes.c_void_p * 4),
        ("dgrad", NslamDecGrad * 4),
        ("rays_o", ctypes.c_void_p),
        ("rays_d", ctypes.c_void_p),
        ("z_vals", ctypes.c_void_p),
        ("n_samples", ctypes.c_int64),
        ("saved_masks", ctypes.c_void_p),
        ("defer_occ", ctypes.c_int32),  # ABI v7
        ("fwd_variant", ctypes.c_int32),  # ABI v18 (NSLAM_FWD_*: 0 default = 1 units, the one kernel)
        ("act_tape", ctypes.c_void_p),  # ABI v9: colour-decoder activation tape (NULL = none)
        ("g_h4", ctypes.c_void_p),  # ABI v17: colour decoder's d/dh4 [M][32] (NULL = none)
    ]


class NslamFrame(ctypes.Structure):
    _fields_ = [("depth", ctypes.c_void_p), ("color", ctypes.c_void_p), ("c2w", ctypes.c_void_p),
                ("cam", ctypes.c_void_p), ("c2w_out", ctypes.c_void_p)]


class NslamLossCfg(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("use_color", ctypes.c_int32), ("handle_dynamic", ctypes.c_int32),
                ("w_color", ctypes.c_float), ("occ_add", ctypes.c_void_p)]


class NslamDraw(ctypes.Structure):  # ABI v7 in-kernel pixel draws
    _fields_ = [("seed", ctypes.c_uint64), ("counter", ctypes.c_void_p), ("ticket", ctypes.c_void_p),
                ("world", ctypes.c_int32), ("rank", ctypes.c_int32), ("gt_max", ctypes.c_void_p),
                ("gt_max_key", ctypes.c_void_p)]


class NslamCamTail(ctypes.Structure):
    """nslam_cam_tail (ABI v23): the camera's Adam step, the iteration's loss and the best pose."""
    _fields_ = [("cam", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step", ctypes.c_void_p), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("ray_loss", ctypes.c_void_p),
                ("n_rays", ctypes.c_int64), ("loss_out", ctypes.c_void_p), ("best_loss", ctypes.c_void_p),
                ("best", ctypes.c_void_p)]


class NslamCamTailLr2(ctypes.Structure):
    """nslam_cam_tail_lr2: the tail with the quaternion's own Adam rate and the pre-step best pose."""
    _fields_ = [("tail", NslamCamTail), ("lr_quat", ctypes.c_float), ("best_before_step", ctypes.c_int32)]


class NslamAdamSeg(ctypes.Structure):
    _fields_ = [
        ("param", ctypes.c_void_p),
        ("grad", ctypes.c_void_p),
        ("exp_avg", ctypes.c_void_p),
        ("exp_avg_sq", ctypes.c_void_p),
        ("step", ctypes.c_void_p),
        ("rows", ctypes.c_void_p),
        ("n", ctypes.c_int64),
        ("row_len", ctypes.c_int32),
        ("lr", ctypes.c_float),
        ("grad_rows", ctypes.c_int32),  # ABI v6: compact [n][row_len] gradient of a row-masked segment
        ("pad_", ctypes.c_int32),
        ("mirror_idx", ctypes.c_void_p),  # ABI v7: packed-copy slots [n][2] of a dense segment
        ("mirror", ctypes.c_void_p),
        ("n_live", ctypes.c_void_p),  # ABI v19: device int64 live count (NULL = n)
    ]


class NslamImapParams(ctypes.Structure):
    """nslam_imap_params / nslam_imap_grads: the iMAP* module's tensors in state_dict layout."""
    _fields_ = [("B", ctypes.c_void_p), ("w", ctypes.c_void_p * 4), ("b", ctypes.c_void_p * 4),
                ("wo", ctypes.c_void_p), ("bo", ctypes.c_void_p)]


class NslamImapQuery(ctypes.Structure):
    _fields_ = [("pts", ctypes.c_void_p), ("rays_o", ctypes.c_void_p), ("rays_d", ctypes.c_void_p),
                ("z_vals", ctypes.c_void_p), ("n_samples", ctypes.c_int64), ("bound_lo", ctypes.c_double * 3),
                ("bound_hi", ctypes.c_double * 3)]


# short names of the table below: vp is a device buffer (or the stream), the typed pointers are host arrays
P = ctypes.POINTER
ci, i32, i64, u64, sz = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
f32, f64, vp = ctypes.c_float, ctypes.c_double, ctypes.c_void_p
i32p, i64p, u8p, f32p, dp, vpp = P(i32), P(i64), P(ctypes.c_uint8), P(f32), P(f64), P(vp)
qcfg, ipp, iqp = P(NslamQueryCfg), P(NslamImapParams), P(NslamImapQuery)

# Every entry point include/nslam.h declares, in the header's order: name -> (restype, argtypes).  Adding one is
# its prototype in the header and its line here; tests/test_abi_cpu.py parses the header and compares the two.
SIGNATURES = {
    "nslam_pack_layout": (ci, [ci, ci, i32p, ci]),
    "nslam_sample_rays": (ci, [vp, vp, vp, vp, i64, dp, dp, vp, i32, vp, i32, i32, vp, vp, sz, vp]),
    "nslam_query_fwd": (ci, [qcfg, vp, i64, vp, vp]),
    "nslam_query_fwd_ws": (ci, [qcfg, vp, i64, vp, vp, sz, vp]),
    "nslam_query_fwd_workspace_size": (sz, [qcfg, i64]),
    "nslam_query_bwd": (ci, [qcfg, vp, i64, vp, vp, vp, sz, vp]),
    "nslam_query_bwd_workspace_size": (sz, [qcfg, i64]),
    "nslam_query_bwd_decoder": (ci, [qcfg, i32, i32, vp, i64, vp, vp, vp, sz, vp]),
    "nslam_query_bwd_decoder_workspace_size": (sz, [qcfg, i32, i64]),
    "nslam_query_saved_size": (sz, [i64]),
    "nslam_query_tape_size": (sz, [i64]),
    "nslam_query_bwd_decoders": (ci, [qcfg, i32, vp, i64, vp, vpp, vp]),
    # live-point lists of the mask-only mapping backward (additive: no ABI bump)
    "nslam_live_points": (ci, [qcfg, i32, vp, i64, vpp, vpp, vp, sz, vp]),
    "nslam_live_points_workspace_size": (sz, [i64]),
    "nslam_query_bwd_decoders_live": (ci, [qcfg, i32, vp, i64, vp, vpp, vpp, vp]),
    "nslam_color_wgrad": (ci, [qcfg, vp, i64, vp, vp, sz, vp]),
    "nslam_composite_fwd": (ci, [vp, vp, i64, i32, vp, vp, vp, vp]),
    "nslam_composite_bwd": (ci, [vp, vp, i64, i32, vp, vp, vp, vp, vp]),
    "nslam_grid_sample_fwd": (ci, [vp, i32p, vp, i64, vp, vp]),
    "nslam_grid_sample_bwd": (ci, [vp, i32p, vp, i64, vp, vp, vp, vp]),
    "nslam_gather_rays": (ci, [P(NslamFrame), i32, i64, vp, i32, i32, i32, i32, i32, i32, f32, f32, f32, f32, dp, dp,
                               vp, vp, vp, vp, vp, P(NslamDraw), vp, vp]),
    "nslam_render_loss": (ci, [P(NslamLossCfg), vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "nslam_render_loss_workspace_size": (sz, [P(NslamLossCfg), i64]),
    "nslam_adam_step": (ci, [P(NslamAdamSeg), i32, f32, f32, f32, i32, vp, vp]),
    "nslam_rows_pack": (ci, [vp, vp, i64, i32, vp, i64, vp, vp]),
    "nslam_rows_unpack": (ci, [vp, vp, i64, i32, vp, vp, i64, vp]),
    "nslam_cam_grad": (ci, [vp, vp, vp, vp, vp, i64, i32, vp, vp]),
    "nslam_cam_grad_parts": (ci, [vp, vp, vpp, i32, vp, vp, i64, i32, vp, vp, vp, vp]),
    "nslam_cam_grad_batch": (ci, [vp, vp, i64, i32, i64p, i64, vpp, i32, vp, vp, i64, i32, vp, vp, vp, vp]),
    "nslam_cam_grad_step": (ci, [P(NslamCamTail), vp, vpp, i32, vp, vp, i64, i32, vp, vp, vp, vp]),
    # TUM-RGBD: separate learning rates on the fused camera tail (additive: no ABI bump)
    "nslam_cam_grad_step_lr2": (ci, [P(NslamCamTailLr2), vp, vpp, i32, vp, vp, i64, i32, vp, vp, vp, vp]),
    "nslam_cam_pose_batch": (ci, [vp, vp, i64, i32, vp]),
    "nslam_frustum_rows": (ci, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
    "nslam_frustum_rows_workspace_size": (sz, [i64]),
    "nslam_loss_sum_best": (ci, [vp, i64, vp, vp, vp, vp, i32, vp]),
    "nslam_cam_vector_batch": (ci, [vp, i64, i32, vp, vp, vp]),
    "nslam_cam_pose": (ci, [vp, vp, vp]),
    # mesh extraction (additive: no ABI bump)
    "nslam_point_masks": (ci, [vp, i64, vp, i32, vp, i32, i32, f32, f32, f32, f32, i32, i32, i64, vp, vp, vp, vp, sz,
                               vp]),
    "nslam_point_masks_workspace_size": (sz, [i64, i32, i64]),
    "nslam_mc_count": (ci, [vp, i32, i32, i32, f32, vp, sz, vp]),
    "nslam_mc_emit": (ci, [vp, i32, i32, i32, f32, dp, dp, vp, vp, i64, i64, vp, vp, vp]),
    "nslam_mc_workspace_size": (sz, [i32, i32, i32]),
    "nslam_points_in_hull": (ci, [vp, i32, i64, vp, i32, vp, vp]),
    "nslam_mesh_face_cull": (ci, [vp, i64, vp, i64, vp, vp]),
    "nslam_mesh_components": (ci, [vp, i64, vp, i64, vp, vp, vp, vp]),
    "nslam_mesh_select": (ci, [vp, i64, vp, vp, vp, f64, vp, vp, vp]),
    "nslam_mesh_remap": (ci, [vp, i64, vp, vp, vp]),
    # TSDF fusion: block range, touch masks, integration, marching cubes over the pool (additive: no ABI bump)
    "nslam_tsdf_block_range": (ci, [vp, vp, i32, i32, i32, f64, f64, f64, f64, i32, f32, f64, f64, vp, vp, vp]),
    "nslam_tsdf_touch": (ci, [vp, vp, i32, i32, i32, f64, f64, f64, f64, i32, f32, f64, f64, i32p, i32p, vp, vp, vp]),
    "nslam_tsdf_integrate": (ci, [vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, f32, f64, f32, i32p, i32p, vp, vp,
                                  vp, i64, i64, vp, vp, vp, i64, vp]),
    "nslam_tsdf_mc_count": (ci, [vp, vp, vp, i64, vp, i32p, i32p, vp, vp, vp]),
    "nslam_tsdf_mc_emit": (ci, [vp, vp, vp, i64, vp, i64, vp, i32p, i32p, f64, vp, vp, vp, vp, i64, i64, vp, vp, vp,
                                vp]),
    # depth odometry: depth maps, the volume's ray cast, ICP sums (additive: no ABI bump)
    "nslam_depth_maps": (ci, [vp, i32, i32, f32, f32, f32, f32, f32, f32, vp, vp, vp]),
    "nslam_tsdf_raycast": (ci, [vp, vp, vp, vp, i64, i32p, i32p, f64, f64, dp, i32, i32, f64, f64, f64, f64, f64, f64,
                                vp, vp, vp]),
    "nslam_icp_partials": (i64, [i32, i32, i32]),
    "nslam_icp_sums": (ci, [vp, vp, i32, i32, i32, dp, vp, vp, i32, i32, dp, f64, f64, f64, f64, f64, f64, vp, i64,
                            vp, vp, vp]),
    # its photometric term: grey pyramid, photometric sums (additive: no ABI bump)
    "nslam_gray_pyramid_size": (i64, [i32, i32, i32]),
    "nslam_gray_pyramid": (ci, [vp, i32, i32, i32, vp, vp]),
    "nslam_photo_sums": (ci, [vp, i32, i32, vp, i32, i32, vp, i32, i32, i32, vp, i32, i32, dp, dp, f64, f64, f64, f64,
                              f64, f64, vp, i64, vp, vp, vp]),
    # evaluation: frustum culling, surface samples, nearest neighbours, ICP sums (additive: no ABI bump)
    "nslam_frustum_seen": (ci, [vp, i64, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp]),
    "nslam_face_areas": (ci, [vp, i64, vp, i64, vp, vp]),
    "nslam_sample_surface": (ci, [vp, i64, vp, vp, i64, i64, u64, vp, vp, vp]),
    "nslam_nn_build": (ci, [vp, i64, dp, f64, i32p, vp, vp]),
    "nslam_nn_query": (ci, [vp, i64, vp, vp, i64, vp, i64, dp, f64, i32p, f64, vp, vp, vp]),
    "nslam_transform_points": (ci, [vp, i64, dp, vp, vp]),
    "nslam_kabsch_sums": (ci, [vp, vp, i64, vp, i64, vp, i64, vp]),
    "nslam_kabsch_partials": (i64, [i64]),
    # depth L1: view rejection, per-view error, mesh rasteriser (additive: no ABI bump)
    "nslam_views_see_any": (ci, [vp, i64, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp]),
    "nslam_depth_l1": (ci, [vp, vp, i64, i64, vp, vp]),
    "nslam_raster_depth": (ci, [vp, i64, vp, i64, vp, i32, i32, i32, f64, f64, f64, f64, f64, f64, i64, i32, vp, vp,
                                sz, vp]),
    "nslam_raster_workspace_size": (sz, [i64]),
    # replay: the scene renderer of visualizer.py's frames (additive: no ABI bump)
    "nslam_scene_render": (ci, [vp, i64, vp, i64, vp, vp, i32, u8p, vp, vp, i64, f64, vp, i32, i32, i32, f64, f64, f64,
                                f64, f64, f64, i32, u8p, f64, i64, i32, vp, vp, vp, vp, sz, vp]),
    "nslam_scene_workspace_size": (sz, [i64, i32, i32, i32]),
    # TUM-RGBD: lens undistortion (additive: no ABI bump)
    "nslam_undistort_u8": (ci, [vp, i32, i32, i32, f64, f64, f64, f64, dp, vp, vp]),
    # the visualiser's panel mosaic (additive: no ABI bump)
    "nslam_vis_panels": (ci, [vp, vp, vp, vp, i32, i32, vp, vp, vp]),
    # iMAP*: the 256-wide Fourier MLP, density compositing, the hierarchical sampler (additive: no ABI bump)
    "nslam_imap_packed_size": (sz, []),
    "nslam_imap_pack": (ci, [ipp, vp, vp]),
    "nslam_imap_tape_size": (sz, [i64]),
    "nslam_imap_fwd": (ci, [ipp, vp, iqp, i64, vp, vp, vp]),
    "nslam_imap_bwd_workspace_size": (sz, [i64]),
    "nslam_imap_bwd": (ci, [ipp, vp, iqp, i64, vp, vp, ipp, vp, vp, sz, vp]),
    "nslam_composite_density_fwd": (ci, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp]),
    "nslam_composite_density_bwd": (ci, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp]),
    "nslam_sample_importance": (ci, [vp, vp, vp, i64, i32, i32, vp, vp, vp]),
    # rendering evaluation: PSNR / depth-L1 sums, SSIM and MS-SSIM means (additive: no ABI bump)
    "nslam_image_errors_workspace_size": (sz, [i32, i64]),
    "nslam_image_errors": (ci, [vp, vp, vp, vp, i32, i64, i32, i32, i32, vp, vp, sz, vp]),
    "nslam_ssim_workspace_size": (sz, [i32, i32, i32, i32, i32]),
    "nslam_ssim": (ci, [vp, vp, i32, i32, i32, i32, f64, f32p, i32, vp, vp, sz, vp]),
    "nslam_workspace_size": (sz, [ci, i64]),
    "nslam_strerror": (ctypes.c_char_p, [ci]),
    "nslam_abi_version": (ci, []),
}
EXPORTS = tuple(SIGNATURES)

_lib = None


def lib():
    """Load libnslam.so once (fails loudly when it has not been built) and bind SIGNATURES."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                               "(make -C nice-slam_amd/csrc); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        # a stale build (older ABI, or one that lacks an export) gets the rebuild message, not an
        # AttributeError from the first missing symbol
        missing = [n for n in EXPORTS if not hasattr(L, n)]
        if missing:
            raise RuntimeError(f"{LIB_PATH} does not export {', '.join(missing)}: rebuild it "
                               "(make -C nice-slam_amd/csrc)")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.nslam_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libnslam.so ABI {L.nslam_abi_version()} != {ABI_VERSION}: rebuild it")
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != NSLAM_OK:
        msg = lib().nslam_strerror(rc).decode()
        raise RuntimeError(f"{what} failed: rc={rc} ({msg})")


def ptr(t):
    """Device pointer of a tensor (None → NULL); refuses host tensors (no CPU fallback)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("nice-slam_amd kernels run on the HIP device only; got a CPU tensor")
    return t.data_ptr()


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def pack_layout(kind: int, nc: int = 1):
    out = (ctypes.c_int32 * 4)()
    n = lib().nslam_pack_layout(kind, nc, out, 4)
    if n != 4:
        raise RuntimeError(f"nslam_pack_layout({kind},{nc}) failed: {n}")
    return {"total": out[0], "vec": out[1], "nf": out[2], "nb": out[3]}
