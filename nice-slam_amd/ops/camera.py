"""The camera kernels of csrc/nslam_camera.hip: poses, camera gradients, the fused tail, the loss sum."""
import ctypes

import torch

from . import span
from .. import _lib
from .._lib import CAM_GRAD_WS_DOUBLES, check, lib, ptr, stream_ptr
from ._check import _expect


def cam_pose(cam, out):
    """nslam_cam_pose (ABI v8): out [3,4] f32 = get_camera_from_tensor(cam [7]) in one launch."""
    _expect("cam_pose", [(cam, torch.float32, (7,))], "cam must be a contiguous float32 [7]")
    _expect("cam_pose", [(out, torch.float32, (3, 4))], "out must be a contiguous float32 [3, 4]")
    check(lib().nslam_cam_pose(ptr(cam), ptr(out), stream_ptr(cam.device)), "nslam_cam_pose")
    return out


def cam_grad(cam, c2w, g_pts, z, rd, out):
    """nslam_cam_grad (ABI v8): out [7] f32 = d loss / d cam through pts = t + (R·dir)·z and
    get_camera_from_tensor (Renderer.py:172-174, common.py:137-176), from g_pts [N*S,3] f64,
    z [N,S] f64, rays_d [N,3] f32 and the c2w [3,4] f32 the rays were built with."""
    n, S = z.shape
    _expect("cam_grad", [(cam, torch.float32, (7,)), (c2w, torch.float32, (3, 4)), (g_pts, torch.float64, (n * S, 3)),
                         (z, torch.float64, (n, S)), (rd, torch.float32, (n, 3)), (out, torch.float32, (7,))])
    with span("cam_grad"):
        rc = lib().nslam_cam_grad(ptr(cam), ptr(c2w), ptr(g_pts), ptr(z), ptr(rd), n, S, ptr(out), stream_ptr(cam.device))
    check(rc, "nslam_cam_grad")
    return out


def cam_grad_parts(cam, c2w, g_pts, z, rd, out, ws, ticket):
    """nslam_cam_grad_parts (ABI v15): cam_grad from the per-decoder d/dpts buffers g_pts (list of
    [N*S,3] f64, summed per point in list order inside the kernel) over several workgroups; ws: f64
    [NSLAM_CAM_GRAD_WS_DOUBLES], ticket: int32 [1] zeroed once (both persistent, one per caller)."""
    n, S = z.shape
    _expect("cam_grad_parts", [(cam, torch.float32, (7,)), (c2w, torch.float32, (3, 4)), (z, torch.float64, (n, S)),
                               (rd, torch.float32, (n, 3)), (out, torch.float32, (7,)),
                               (ws, torch.float64, (CAM_GRAD_WS_DOUBLES,)), (ticket, torch.int32, (1,))] +
            [(g, torch.float64, (n * S, 3)) for g in g_pts])
    bufs = (ctypes.c_void_p * len(g_pts))(*[ptr(g) for g in g_pts])
    with span("cam_grad"):
        rc = lib().nslam_cam_grad_parts(ptr(cam), ptr(c2w), bufs, len(g_pts), ptr(z), ptr(rd), n, S, ptr(out), ptr(ws),
                                        ptr(ticket), stream_ptr(cam.device))
    check(rc, "nslam_cam_grad_parts")
    return out


def cam_grad_step(cam, c2w, g_pts, z, rd, g_cam, ws, ticket, adam, ray_loss, loss_out, best_loss=None, best=None,
                  lr_quat=None, best_before_step=False):
    """nslam_cam_grad_step (ABI v23): cam_grad_parts, then in its last workgroup the camera's Adam step in
    place (adam = (exp_avg [7], exp_avg_sq [7], step [1], lr, beta1, beta2, eps)), loss_out = the fixed-order
    sum of ray_loss and, with best_loss / best, the best-pose update — bit-identical to cam_grad_parts +
    FusedAdam.step + loss_sum_best, in one launch.
    lr_quat (a rate for elements 0..3) or best_before_step (best = the camera before the step) select
    nslam_cam_grad_step_lr2, the reference's seperate_LR loop (Tracker.py:202-247) on the same kernel."""
    n, S = z.shape
    ex, ex2, stp, lr, b1, b2, eps = adam
    checks = [(cam, torch.float32, (7,)), (c2w, torch.float32, (3, 4)), (z, torch.float64, (n, S)),
              (rd, torch.float32, (n, 3)), (g_cam, torch.float32, (7,)), (ws, torch.float64, (CAM_GRAD_WS_DOUBLES,)),
              (ticket, torch.int32, (1,)), (ex, torch.float32, (7,)), (ex2, torch.float32, (7,)),
              (stp, torch.float32, (1,)), (ray_loss, torch.float64, (ray_loss.numel(),)),
              (loss_out, torch.float64, ())]
    if best_loss is not None:
        checks += [(best_loss, torch.float64, ()), (best, torch.float32, (7,))]
    _expect("cam_grad_step", checks + [(g, torch.float64, (n * S, 3)) for g in g_pts])
    tail = _lib.NslamCamTail(ptr(cam), ptr(ex), ptr(ex2), ptr(stp), float(lr), float(b1), float(b2), float(eps),
                             ptr(ray_loss), ray_loss.numel(), ptr(loss_out), ptr(best_loss), ptr(best))
    bufs = (ctypes.c_void_p * len(g_pts))(*[ptr(g) for g in g_pts])
    fn, name = lib().nslam_cam_grad_step, "nslam_cam_grad_step"
    if lr_quat is not None or best_before_step:
        tail = _lib.NslamCamTailLr2(tail, float(lr if lr_quat is None else lr_quat), int(bool(best_before_step)))
        fn, name = lib().nslam_cam_grad_step_lr2, "nslam_cam_grad_step_lr2"
    with span("cam_grad"):
        rc = fn(ctypes.byref(tail), ptr(c2w), bufs, len(g_pts), ptr(z), ptr(rd), n, S, ptr(g_cam), ptr(ws),
                ptr(ticket), stream_ptr(cam.device))
    check(rc, name)
    return loss_out


def cam_vector_batch(c2w, out, copy=None):
    """nslam_cam_vector_batch (ABI v22): out[k] = get_tensor_from_camera(c2w[k]) for c2w [n, 3|4, 4] f32
    (common.camera_tensors' arithmetic, one launch); copy: optional second [n, 7] f32 receiving the same."""
    n = c2w.shape[0]
    _expect("cam_vector_batch", [(c2w, torch.float32, (range(1, 65), (3, 4), 4))],
            "c2w must be a contiguous float32 [n, 3|4, 4], 1 <= n <= 64")
    _expect("cam_vector_batch", [(t, torch.float32, (n, 7)) for t in ((out,) if copy is None else (out, copy))],
            "out / copy must be contiguous float32 [n, 7]")
    rc = lib().nslam_cam_vector_batch(ptr(c2w), c2w.shape[1] * 4, n, ptr(out), ptr(copy),
                                      stream_ptr(c2w.device))
    check(rc, "nslam_cam_vector_batch")
    return out


def cam_pose_batch(cams, c2w):
    """nslam_cam_pose_batch (ABI v19): c2w[k, :3, :4] = get_camera_from_tensor(cams[k]) for cams [n, 7] f32
    and c2w [n, 3 or 4, 4] f32 (both contiguous), one launch."""
    n = cams.shape[0]
    _expect("cam_pose_batch", [(cams, torch.float32, (n, 7))], "cams must be a contiguous float32 [n, 7]")
    _expect("cam_pose_batch", [(c2w, torch.float32, (n, (3, 4), 4))], "c2w must be a contiguous float32 [n, 3|4, 4]")
    with span("cam_pose"):
        rc = lib().nslam_cam_pose_batch(ptr(cams), ptr(c2w), c2w.shape[1] * 4, n, stream_ptr(cams.device))
    check(rc, "nslam_cam_pose_batch")
    return c2w


def loss_sum_best(ray_loss, out, best_loss=None, cam=None, best=None):
    """nslam_loss_sum_best (ABI v21): out (float64 device scalar) = ray_loss.sum() in a fixed order (one
    workgroup: the same value on every call); with best_loss: if out < best_loss, best_loss = out and
    best = cam (the tracker's best-pose update, Tracker.py:245-247).  Returns out."""
    if ray_loss.dtype != torch.float64 or out.dtype != torch.float64 or not ray_loss.is_contiguous():
        raise ValueError("loss_sum_best: a contiguous float64 ray_loss and a float64 scalar out")
    if best_loss is not None and (best_loss.dtype != torch.float64 or cam.dtype != torch.float32
                                  or best.shape != cam.shape or not (cam.is_contiguous() and best.is_contiguous())):
        raise ValueError("loss_sum_best: a float64 best_loss and two contiguous float32 vectors of one shape")
    check(lib().nslam_loss_sum_best(ptr(ray_loss), ray_loss.numel(), ptr(out),
                                    ptr(best_loss) if best_loss is not None else None,
                                    ptr(cam) if best_loss is not None else None,
                                    ptr(best) if best_loss is not None else None,
                                    cam.numel() if best_loss is not None else 0, stream_ptr(ray_loss.device)),
          "nslam_loss_sum_best")
    return out


def cam_grad_batch(cams, c2w, ray_begin, n_per, g_pts, z, rd, out, ws, tickets):
    """nslam_cam_grad_batch (ABI v19): out [n, 7] = d loss / d cams [n, 7] of the bundle-adjustment cameras,
    camera k's rays being [ray_begin[k], ray_begin[k] + n_per) of the batch (z [N, S] f64, rd [N, 3] f32,
    g_pts: list of [N*S, 3] f64 d/dpts shares); c2w [n, 3|4, 4] the poses rendered with; ws f64
    [n * NSLAM_CAM_GRAD_WS_DOUBLES], tickets int32 [n] zeroed once (persistent per caller)."""
    n = cams.shape[0]
    N, S = z.shape
    _expect("cam_grad_batch", [(cams, torch.float32, (n, 7)), (z, torch.float64, (N, S)), (rd, torch.float32, (N, 3)),
                               (out, torch.float32, (n, 7)), (ws, torch.float64, (n * CAM_GRAD_WS_DOUBLES,)),
                               (tickets, torch.int32, (n,))] + [(g, torch.float64, (N * S, 3)) for g in g_pts])
    _expect("cam_grad_batch", [(c2w, torch.float32, (n, None, None))], "c2w must be a contiguous float32 [n, 3|4, 4]")
    rb = (ctypes.c_int64 * n)(*[int(r) for r in ray_begin])
    bufs = (ctypes.c_void_p * len(g_pts))(*[ptr(g) for g in g_pts])
    with span("cam_grad"):
        rc = lib().nslam_cam_grad_batch(ptr(cams), ptr(c2w), c2w.shape[1] * 4, n, rb, int(n_per), bufs, len(g_pts),
                                        ptr(z), ptr(rd), N, S, ptr(out), ptr(ws), ptr(tickets), stream_ptr(cams.device))
    check(rc, "nslam_cam_grad_batch")
    return out
