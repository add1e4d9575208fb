/*
 * nslam.h — C-ABI of libnslam.so, the MI355X (gfx950) hot path of NICE-SLAM's volumetric renderer.
 *
 * The reference (LongruiDong/nice-slam) is pure PyTorch; it has no native/FFI boundary.  Each
 * entry point below replaces a specific piece of the reference's Python hot path (file:line are
 * relative to the reference checkout), and is bound from Python by ctypes in
 * nice-slam_amd/_lib.py (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Contract (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises;
 *   - no globals, no persistent allocations: re-entrant across threads/processes (the reference
 *     runs tracker, mapper and coarse mapper concurrently on one GPU, src/NICE_SLAM.py:288-307);
 *   - return 0 on success, a negative NSLAM_E* code on bad arguments, or NSLAM_EHIP - hipError
 *     when a launch fails.  nslam_strerror() maps codes to text.
 *
 * Grid layout: a feature grid is the reference's [1, C=32, Z, Y, X] float32 tensor stored
 * channels-last, i.e. physically [Z][Y][X][32] (torch.channels_last_3d); one trilinear corner
 * is one 128-byte row.
 */
#ifndef NSLAM_H
#define NSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSLAM_C_DIM 32
#define NSLAM_HIDDEN 32
#define NSLAM_EMB 93

enum {
  NSLAM_OK = 0,
  NSLAM_EINVAL = -1,       /* bad pointer / size / enum */
  NSLAM_EUNSUPPORTED = -2, /* configuration outside the NICE-SLAM path (e.g. S > 256) */
  NSLAM_EWORKSPACE = -3,   /* workspace too small */
  NSLAM_EHIP = -1000       /* NSLAM_EHIP - hipError_t */
};

enum { NSLAM_STAGE_COARSE = 0, NSLAM_STAGE_MIDDLE = 1, NSLAM_STAGE_FINE = 2, NSLAM_STAGE_COLOR = 3 };
enum { NSLAM_DEC_COARSE = 0, NSLAM_DEC_MIDDLE = 1, NSLAM_DEC_FINE = 2, NSLAM_DEC_COLOR = 3 };
/* nslam_query_cfg.fwd_variant (ABI v18): nslam_query_fwd_ws has one kernel, UNITS = one one-wave
 * workgroup per decoder and 32-point tile, and DEFAULT means it.  The values 2 and 3 named forwards
 * that were retired; they, and every other value, are NSLAM_EINVAL. */
enum { NSLAM_FWD_DEFAULT = 0, NSLAM_FWD_UNITS = 1 };

/* One feature grid (src/NICE_SLAM.py:192-250) with the bound it is normalised against
 * (decoder.bound, src/NICE_SLAM.py:152-157; the coarse decoder uses bound*2). */
typedef struct nslam_grid {
  const float* data; /* channels-last [Z][Y][X][32]; NULL when the stage does not read it */
  float* grad;       /* same layout, accumulated with atomics; NULL = no grid gradient      */
  int32_t dims[3];   /* Z, Y, X (= D, H, W of F.grid_sample)                                 */
  int32_t pad_;
  double lo[3];      /* x, y, z lower bound (float64, as the reference)                      */
  double hi[3];      /* x, y, z upper bound                                                  */
  /* ABI v6, frustum-compacted gradient: slot == NULL -> `grad` is a dense grid like `data`; else
   * `grad` is [n_rows][32] for the frustum-selected voxels (Mapper.py:314-333) and slot[Z*Y*X]
   * maps a voxel row to its compact row (-1: not selected, its gradient is not formed — the
   * reference optimises only the masked vector, Mapper.py:394-401). */
  const int32_t* slot;
} nslam_grid;

/* Where a decoder's parameter gradients go: `base` is a flat float32 buffer and the offsets are
 * element offsets of each parameter in it (natural row-major [out][in] layout, i.e. the layout
 * of nn.Linear.weight).  base == NULL: no parameter gradients for this decoder. */
typedef struct nslam_dec_grad {
  float* base;
  int64_t w[5], b[5];   /* pts_linears.i.weight / .bias                       */
  int64_t wc[5], bc[5]; /* fc_c.i.weight / .bias (unused for the coarse MLP)  */
  int64_t wo, bo;       /* output_linear.weight / .bias                       */
  int64_t B;            /* embedder._B [3][93] (unused for the coarse MLP)    */
  int64_t count;        /* floats in the flat buffer (all parameters)         */
} nslam_dec_grad;

/* Point query: NICE.forward + Renderer.eval_points
 * (src/conv_onet/models/decoder.py:168-342, src/utils/Renderer.py:23-61). */
typedef struct nslam_query_cfg {
  int32_t stage;            /* NSLAM_STAGE_*                                             */
  int32_t need_pts_grad;    /* backward: write d loss / d pts                             */
  double bound_lo[3];       /* OOB test bound (strict <, >), Renderer.py:43-46            */
  double bound_hi[3];
  nslam_grid grid[4];       /* indexed by NSLAM_DEC_*                                     */
  const float* packed[4];   /* packed decoder weights (nslam_pack_layout), NULL if unused */
  nslam_dec_grad dgrad[4];  /* parameter-gradient destinations                            */
  /* Ray form of the point list (ABI v4): when rays_o != NULL the points are generated in-kernel
   * as pts[r*S + s] = rays_o[r] + rays_d[r] * z_vals[r][s] in float64 (Renderer.py:172-174,
   * float32 rays promoted) and the `pts` argument is ignored.  The backward's g_pts (ABI v5: also
   * in ray form) is d loss / d pts per generated point, [M][3] float64. */
  const float* rays_o;      /* [M/S][3] float32 */
  const float* rays_d;      /* [M/S][3] float32 */
  const double* z_vals;     /* [M/S][S] float64 */
  int64_t n_samples;        /* S */
  /* ReLU masks saved by the forward (ABI v4; NULL = none): nslam_query_fwd writes every
   * evaluated decoder's masks here and nslam_query_bwd then skips the forward recompute of the
   * decoders that have no parameter gradients (their backward needs only the masks).
   * nslam_query_saved_size(M) bytes; layout [decoder][tile of 32 points][layer 0..4][64] uint16. */
  uint16_t* saved_masks;
  /* ABI v7: nslam_query_fwd_ws with defer_occ = 1 leaves raw[...,3] = the fine occupancy and the
   * middle occupancy in ws (float [M]) instead of adding them in a separate pass: the consumer
   * adds it on read (nslam_loss_cfg.occ_add = ws), saving a launch per query. */
  int32_t defer_occ;
  /* ABI v18: how nslam_query_fwd_ws spreads the fine / colour stage over the chip (NSLAM_FWD_*; 0 = the
   * library's default).  Every variant computes the same values in the same order: bit-identical
   * outputs, masks and activation tape. */
  int32_t fwd_variant;
  /* ABI v9: activation tape of the colour decoder (NULL = none).  nslam_query_fwd[_ws] writes the
   * post-ReLU hidden tiles h0..h4 of every 32-point tile ([tile][layer][32 points][32 features]
   * float, nslam_query_tape_size(M) bytes; layout private to the library); with it and saved_masks the colour decoder's weight-gradient
   * backward reads them instead of recomputing its forward (Mapper.py:503). */
  float* act_tape;
  /* ABI v17: cotangent of the colour decoder's last hidden layer h4, [M][32] float32, 16-byte aligned
   * (else NSLAM_EINVAL; NULL = none),
   * added to its output layer's Woᵀg in every backward of the colour decoder.  A direct caller of
   * MLP(color=True) (decoder.py:154-159,198-203) forms the 4th output row h4·Wo[3] + bo[3] itself
   * (NICE.forward overwrites that row, decoder.py:341) and passes d/dh4 here. */
  const float* g_h4;
} nslam_query_cfg;

/* ---- packing ------------------------------------------------------------------------------
 * Decoder weights are re-laid-out into MFMA fragment order by the caller (a gather with the
 * index map described here).  kind 0 = MLP with Fourier embedding and `nc` feature blocks
 * (middle/color nc=1, fine nc=2); kind 1 = MLP_no_xyz (coarse).  Writes up to `n` int32 values:
 *   out[0] = total packed floats, out[1] = offset of the vector section, out[2] = fwd frag count,
 *   out[3] = bwd frag count.  Returns the number of values written or <0. */
int nslam_pack_layout(int kind, int nc, int32_t* out, int n);

/* ---- sampler: src/utils/Renderer.py:82-174 (perturb=0, N_importance=0) ---------------------
 * z_vals[N][S0+S1] (float64) for rays_o/rays_d [N][3] float32 and gt_depth [N] float32
 * (NULL = no depth: S1 is forced to 0 and near = 0.01).  t_strat = torch.linspace(0,1,S0)
 * (float32), t_surf = torch.linspace(0,1,S1).double() — passed in so the sampler uses the very
 * values the reference uses.  The batch-global max(gt_depth) (Renderer.py:109,144) is computed
 * over the N rays unless gt_max (a DEVICE float) is given — a ray-sharded job passes the
 * all-reduced maximum so every shard samples exactly as the full batch would.
 * ws must hold nslam_workspace_size(NSLAM_WS_SAMPLER, N) bytes. */
int nslam_sample_rays(const float* rays_o, const float* rays_d, const float* gt_depth, const float* gt_max,
                      int64_t n_rays, const double* bound_lo, const double* bound_hi, /* HOST pointers, 3 each */
                      const float* t_strat, int32_t s0, const double* t_surf, int32_t s1,
                      int32_t lindisp, double* z_vals, void* ws, size_t ws_bytes, void* stream);

/* ---- fused point query ------------------------------------------------------------------------
 * raw[M][4] float32 for pts[M][3] float64 (Renderer.eval_points incl. `ret[~mask,3]=100`). */
int nslam_query_fwd(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, float* raw, void* stream);
/* The same result with the decoders evaluated by separate workgroups (ABI v5): fine and colour
 * stages launch 2-3x the waves of nslam_query_fwd (latency hiding at mapping batch sizes) and
 * combine fine + middle occupancy afterwards.  ws: nslam_query_fwd_workspace_size(cfg, M) bytes
 * (0 for the coarse and middle stages, which fall through to nslam_query_fwd). */
int nslam_query_fwd_ws(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, float* raw, void* ws,
                       size_t ws_bytes, void* stream);
size_t nslam_query_fwd_workspace_size(const nslam_query_cfg* cfg, int64_t n_pts);

/* Backward of nslam_query_fwd for cotangent g_raw[M][4]: accumulates grid gradients into
 * cfg->grid[i].grad (atomics, caller zero-initialises), adds parameter gradients into
 * cfg->dgrad[i] (per-workgroup LDS accumulation → partial slabs in `ws` → deterministic
 * reduction) and writes g_pts[M][3] float64 when cfg->need_pts_grad.
 * ws must hold nslam_query_bwd_workspace_size(cfg, n_pts) bytes (0 when no parameter grads). */
int nslam_query_bwd(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, const float* g_raw,
                    double* g_pts, void* ws, size_t ws_bytes, void* stream);
size_t nslam_query_bwd_workspace_size(const nslam_query_cfg* cfg, int64_t n_pts);
/* One decoder's share of nslam_query_bwd (ABI v4): its grid gradient, its parameter gradients
 * and its d/dpts (written, or added when accumulate_pts).  Decoders whose gradients go to
 * different buffers may run concurrently on different streams (the mapping iteration does:
 * grids and decoder gradients are disjoint; with need_pts_grad the calls must be ordered).
 * ws: nslam_query_bwd_decoder_workspace_size(cfg, dec, n_pts) bytes. */
int nslam_query_bwd_decoder(const nslam_query_cfg* cfg, int32_t dec, int32_t accumulate_pts, const double* pts,
                            int64_t n_pts, const float* g_raw, double* g_pts, void* ws, size_t ws_bytes,
                            void* stream);
size_t nslam_query_bwd_decoder_workspace_size(const nslam_query_cfg* cfg, int32_t dec, int64_t n_pts);
size_t nslam_query_saved_size(int64_t n_pts);
size_t nslam_query_tape_size(int64_t n_pts); /* ABI v9 */
/* ABI v10 (v16 signature): the backward of several decoders in ONE launch — the grid gradient and
 * d/dpts share of nslam_query_bwd_decoder of every decoder d in dec_mask (bit d), their workgroups
 * interleaved over the grid, so decoders that would run as concurrent launches on separate streams
 * need no cross-stream fork / join.  Requires cfg->saved_masks (the forward's ReLU masks): every
 * decoder runs the mask-only backward.  No parameter gradients are formed here: a decoder in dec_mask
 * with dgrad[d].base != NULL is NSLAM_EUNSUPPORTED (the colour decoder's come from nslam_color_wgrad).
 * With cfg->need_pts_grad, g_pts[d] (a host array of 4 device pointers) receives decoder d's d/dpts
 * [M][3] float64 (written, not accumulated).  Replaces the per-decoder loop of
 * Tracker.optimize_cam_in_batch's backward (Tracker.py:125) / Mapper.optimize_map's (Mapper.py:503). */
int nslam_query_bwd_decoders(const nslam_query_cfg* cfg, int32_t dec_mask, const double* pts, int64_t n_pts,
                             const float* g_raw, double* const* g_pts, void* stream);
/* Live-point lists (additive, no ABI bump).  With a frustum-compacted grid gradient (nslam_grid.slot) a
 * mapping backward without d/dpts has one output per decoder: the scatter into the selected rows.  A point
 * whose 8 corner rows of grid[d] all have slot < 0 contributes nothing (the reference never forms those
 * gradients, Mapper.py:314-333,394-401), yet nslam_query_bwd_decoders runs its whole cotangent chain and
 * scatter walk.  For every decoder d in dec_mask (bit d), nslam_live_points writes live_idx[d] (device int32,
 * capacity n_pts): the indices, ascending, of the valid points with at least one corner row of grid[d] whose
 * slot >= 0 — the corners are formed by the query kernels' own arithmetic, so the list is exactly what the
 * scatter would keep — and *n_live[d] (device int64) = their count.  A grid without a slot map keeps every
 * point.  live_idx / n_live: HOST arrays of 4 device pointers, indexed by NSLAM_DEC_*.  Three launches
 * (flags + per-block counts, a scan of the counts, the indices), deterministic; nothing of the iteration's
 * map state is read but the slot maps, so with the rays of a batch known the lists can be formed ahead of
 * the backward on another stream.  A list is valid for the slot maps it was formed from: after a slot map
 * is rewritten the lists are formed again.  ws: nslam_live_points_workspace_size(n_pts) bytes, 8-byte
 * aligned.  n_pts < 2^31. */
int nslam_live_points(const nslam_query_cfg* cfg, int32_t dec_mask, const double* pts, int64_t n_pts,
                      int32_t* const* live_idx, int64_t* const* n_live, void* ws, size_t ws_bytes, void* stream);
size_t nslam_live_points_workspace_size(int64_t n_pts);
/* nslam_query_bwd_decoders over each decoder's live points only: lane p of 32-point tile t of decoder d
 * takes point live_idx[d][32 t + p] (its point, cotangent row and ReLU masks are gathered by that index);
 * lanes at or past *n_live[d] write nothing.  The launch is sized for n_pts points whatever the lists hold
 * (workgroups past a list's end exit at once), so a captured hipGraph stays valid for later lists.  The grid
 * gradients equal nslam_query_bwd_decoders' up to the order of their float atomics: each point's cotangent
 * is computed independently of the tile it sits in, only the runs of equal voxels merged before the atomics
 * regroup.  cfg->need_pts_grad is NSLAM_EUNSUPPORTED (d/dpts is needed for every point); otherwise the
 * requirements of nslam_query_bwd_decoders. */
int nslam_query_bwd_decoders_live(const nslam_query_cfg* cfg, int32_t dec_mask, const double* pts, int64_t n_pts,
                                  const float* g_raw, const int32_t* const* live_idx, const int64_t* const* n_live,
                                  void* stream);
/* ABI v16: the colour decoder's parameter gradients of a colour-stage backward (added into
 * cfg->dgrad[COLOR]; Mapper.py:503 for color_decoder.parameters(), decoder.py:177-203) from the
 * forward's activation tape and ReLU masks (cfg->act_tape, cfg->saved_masks) and the cotangent
 * g_raw[M][4] — the cotangent chain, the colour feature and the Fourier features are recomputed, so
 * the call reads nothing the grid-gradient backward (nslam_query_bwd_decoders) writes and the two may
 * run concurrently on different streams.  Split-K over the points, deterministic.
 * ws >= nslam_query_bwd_decoder_workspace_size(cfg, NSLAM_DEC_COLOR, M) bytes. */
int nslam_color_wgrad(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, const float* g_raw, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- compositing: raw2outputs_nerf_color, src/common.py:204-245 (occupancy mode) ------------ */
int nslam_composite_fwd(const float* raw, const double* z_vals, int64_t n_rays, int32_t n_samples,
                        double* depth, double* var, float* color, void* stream);
/* g_raw[N][S][4] from cotangents g_depth[N], g_var[N] (float64), g_color[N][3] (float32);
 * any cotangent pointer may be NULL (= zeros). */
int nslam_composite_bwd(const float* raw, const double* z_vals, int64_t n_rays, int32_t n_samples,
                        const double* g_depth, const double* g_var, const float* g_color, float* g_raw,
                        void* stream);

/* ---- standalone trilinear lookup (F.grid_sample 5-D, bilinear, border, align_corners=True;
 *      the op of src/conv_onet/models/decoder.py:173-174) ----------------------------------------
 * coords[M][3] float32 normalised (x,y,z in [-1,1]); out[M][32]. */
int nslam_grid_sample_fwd(const float* grid, const int32_t* dims, const float* coords, int64_t n,
                          float* out, void* stream);
/* grad_grid (atomics, may be NULL) and grad_coords[M][3] (may be NULL) from grad_out[M][32].
 * `dims` (Z, Y, X) is a HOST pointer in both grid_sample entry points. */
int nslam_grid_sample_bwd(const float* grid, const int32_t* dims, const float* coords, int64_t n,
                          const float* grad_out, float* grad_grid, float* grad_coords, void* stream);

/* ---- mapping / tracking iteration (ABI v4) ------------------------------------------------ */
#define NSLAM_MAX_FRAMES 32

/* One RGB-D frame resident on the device (keyframe_dict entry / current frame). */
typedef struct nslam_frame {
  const float* depth; /* [H][W] float32                              */
  const float* color; /* [H][W][3] float32                           */
  const float* c2w;   /* [3 or 4][4] float32 row-major camera-to-world (may be NULL when cam is set) */
  /* ABI v21: the pose given by its camera 7-vector instead (get_camera_from_tensor, common.py:137-176, the
   * arithmetic of nslam_cam_pose): the gather forms it itself and, when c2w_out is not NULL, also writes
   * it there ([3][4] row-major) for later launches — the tracker's camera iteration needs no pose launch */
  const float* cam;   /* [7] float32 (q, t) or NULL                   */
  float* c2w_out;     /* [3][4] float32 or NULL                        */
} nslam_frame;

/* In-kernel pixel draws (ABI v7): with pix == NULL and draw != NULL the select_uv indices are drawn
 * on the device — uniform over the window, from a counter-based splitmix64 stream keyed by
 * (seed, *counter, ray), NOT torch.randint's Philox sequence — and *counter advances by one per
 * call (the last workgroup bumps it, stream-ordered), so a hipGraph replay draws fresh pixels
 * without host RNG work.  ticket: device uint32, zero-initialised once, reserved for the call. */
typedef struct nslam_draw {
  uint64_t seed;
  uint64_t* counter;
  uint32_t* ticket;
  /* Ray sharding without a collective (world > 1; world = 1, rank = 0: a single rank).  The
   * global batch holds n_per * world pixels per frame, drawn from ONE stream (every rank passes
   * the same seed); this call's ray (f, k) is global ray f*n_per*world + rank*n_per + k.
   * gt_max (device float, may be NULL) receives max(gt_depth) over the kept rays of the whole
   * global batch (Renderer.py:107-111,144), which every rank evaluates itself — each thread
   * re-draws its pixel slot for every rank — so the sampler needs no all-reduce.
   * gt_max_key: device uint32, zero-initialised once, required with gt_max. */
  int32_t world;
  int32_t rank;
  float* gt_max;
  uint32_t* gt_max_key;
} nslam_draw;

/* n_kept (ABI v7, device int64, may be NULL) is incremented by the number of kept rays.
 * get_samples (src/common.py:92-134: get_sample_uv + select_uv + get_rays_from_uv) for
 * n_frames frames (HOST array, <= NSLAM_MAX_FRAMES) x n_per pixels each, plus the inside-mask
 * prefilter of Mapper.py:469-481 / Tracker.py:93-104.  pix[f*n_per + k] is select_uv's randint
 * index into the frame's window [h0,h1) x [w0,w1) (row-major over the window).  Outputs are
 * [n_frames*n_per] rays in frame order.  With bound_lo/bound_hi (HOST, float64 [3]) a ray whose
 * bound-exit distance is < gt depth gets keep = 0 and gt_depth = 0 (it then contributes nothing:
 * the prefilter removes it in the reference); NULL bounds keep every ray. */
int nslam_gather_rays(const nslam_frame* frames, int32_t n_frames, int64_t n_per, const int64_t* pix,
                      int32_t H, int32_t W, int32_t h0, int32_t h1, int32_t w0, int32_t w1, float fx, float fy,
                      float cx, float cy, const double* bound_lo, const double* bound_hi, float* rays_o,
                      float* rays_d, float* gt_depth, float* gt_color, uint8_t* keep, const struct nslam_draw* draw,
                      int64_t* n_kept, void* stream);

/* Rendering loss fused with compositing and its backward (the loss is a sum of per-ray terms).
 *   mode NSLAM_LOSS_MAPPER (Mapper.py:487-501):
 *     L = sum_{keep, gt>0} |gt - depth| + [use_color] w_color * sum_{keep} |gt_c - color|
 *   mode NSLAM_LOSS_TRACKER (Tracker.py:110-123), u = var (detached):
 *     r = |gt - depth| / sqrt(u + 1e-10);  m = keep & gt>0 [& r < 10 median_{keep}(r) if handle_dynamic]
 *     L = sum_m r + [use_color] w_color * sum_m |gt_c - color|
 * Writes depth/var (float64 [N]) and color (float32 [N][3]) like nslam_composite_fwd, the
 * per-ray loss terms ray_loss (float64 [N], may be NULL) and, when g_raw != NULL, dL/draw
 * [N][S][4] for dL = 1.  keep may be NULL (all rays kept).  The tracker's median needs
 * N <= 16384 rays. ws: nslam_render_loss_workspace_size bytes. */
enum { NSLAM_LOSS_MAPPER = 0, NSLAM_LOSS_TRACKER = 1 };
typedef struct nslam_loss_cfg {
  int32_t mode;
  int32_t use_color;
  int32_t handle_dynamic;
  float w_color;
  const float* occ_add; /* ABI v7: NULL, or [N*S] float added to raw[...,3] on read (the middle
                           occupancy of a deferred-combine query, decoder.py:331-334 order) */
} nslam_loss_cfg;
int nslam_render_loss(const nslam_loss_cfg* cfg, const float* raw, const double* z_vals, int64_t n_rays,
                      int32_t n_samples, const float* gt_depth, const float* gt_color, const uint8_t* keep,
                      double* depth, double* var, float* color, double* ray_loss, float* g_raw, void* ws,
                      size_t ws_bytes, void* stream);
size_t nslam_render_loss_workspace_size(const nslam_loss_cfg* cfg, int64_t n_rays);

/* Adam (torch.optim.Adam, weight_decay 0, amsgrad off: Tracker.py:126, Mapper.py:504) over up to
 * NSLAM_ADAM_MAX_SEGS parameter segments in one launch.  A segment is dense (rows == NULL: n
 * floats) or row-masked (n row indices of row_len floats each, row_len % 4 == 0 and 16-byte
 * aligned param/grad/state): the frustum-selected voxels of a channels-last grid
 * (Mapper.py:314-333), updated in place in the dense grid with state for the selected rows only
 * (exp_avg/exp_avg_sq are [n][row_len], in row-list order).  Like torch, every segment has its
 * own step count (`step`, a device float, 0 before the first update): the launch uses step+1
 * and a second single-wave launch advances every segment's step (graph-replay safe); `ticket`
 * is unused since ABI v5 (may be NULL).  Pass only segments that have a gradient
 * this iteration (torch skips parameters whose .grad is None).  With zero_grad the grad entries
 * read are reset to 0. */
#define NSLAM_ADAM_MAX_SEGS 16
typedef struct nslam_adam_seg {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;
  const int32_t* rows;
  int64_t n;
  int32_t row_len;
  float lr;
  int32_t grad_rows; /* ABI v6, row-masked segments: 1 = grad is compact [n][row_len] in row-list order
                        (the frustum-compacted gradient of nslam_grid.slot); 0 = grad is dense like param */
  int32_t pad_;
  /* ABI v7, dense segments: after the update param[e] is also stored to mirror[mirror_idx[2e]] and
   * mirror[mirror_idx[2e+1]] (-1 = none): the MFMA-packed copy of a decoder (nslam_pack_layout)
   * stays current without a re-pack pass.  mirror == NULL: no mirror. */
  const int32_t* mirror_idx;
  float* mirror;
  /* ABI v19: NULL, or a DEVICE int64: the segment updates only its first min(*n_live, n) rows (row-masked)
   * or elements (dense).  A frustum selection made on the device (Mapper.optimize_map's per-call mask,
   * Mapper.py:314-333) then needs no host read-back of its size: the segment, its Adam state and its
   * launch are sized for the capacity n (every voxel of the grid), so a captured hipGraph of the
   * iteration stays valid for every later call's selection. */
  const int64_t* n_live;
} nslam_adam_seg;
/* ticket: NULL = the step counts advance in a second single-wave launch; else a device uint32
 * (zero-initialised, re-armed by the call itself) with which the update kernel's last workgroup
 * advances them — one launch per step (ABI v9).  A ticket belongs to one call at a time: calls that
 * may run concurrently (other streams, other processes) each pass their own. */
int nslam_adam_step(const nslam_adam_seg* segs, int32_t n_segs, float beta1, float beta2, float eps,
                    int32_t zero_grad, uint32_t* ticket, void* stream);
/* Sparse gradient exchange of a ray-sharded mapping iteration (ABI v5).  Only the frustum-
 * selected grid rows reach Adam (Mapper.py:314-333,394-401,504), so only they need summing across
 * ranks: nslam_rows_pack copies rows[i] (row_len floats each, row_len % 4 == 0, 16-byte aligned
 * grid and out) of `grid` to out[i*row_len ...] and appends the n_tail floats of `tail` (the
 * decoder gradients); the caller all-reduces `out` (n_rows*row_len + n_tail floats) and
 * nslam_rows_unpack writes it back.  Row indices are in units of row_len floats from `grid`, so
 * one call covers every grid of a flat gradient buffer. */
int nslam_rows_pack(const float* grid, const int32_t* rows, int64_t n_rows, int32_t row_len, const float* tail,
                    int64_t n_tail, float* out, void* stream);
int nslam_rows_unpack(const float* in, const int32_t* rows, int64_t n_rows, int32_t row_len, float* grid,
                      float* tail, int64_t n_tail, void* stream);

/* ABI v9.  Camera gradient of a tracking iteration (Tracker.py:110-126): the 7-vector gradient of
 * the loss through pts = t + (R·dir)·z (Renderer.py:172-174, common.py:80-89) and
 * get_camera_from_tensor (common.py:137-176), in one single-workgroup launch:
 *   g_t = Σ g_pts;  g_R = (Σ_r g_d,r d_rᵀ)·R with g_d,r = Σ_s z_rs g_pts,rs (dir = Rᵀ d);
 *   g_q = s (G + Gᵀ) q − s² (qᵀ G q) q,  s = 2/|q|²,  G = Σ_ij g_R,ij M_ij  (R = I + s·P(q)).
 * cam [7] (w,x,y,z,tx,ty,tz), c2w [3,4] the pose rendered with, g_pts [n_rays*n_samples,3] f64,
 * z_vals [n_rays,n_samples] f64, rays_d [n_rays,3] f32; writes g_cam [7] f32.
 * NSLAM_EUNSUPPORTED when 3*n_rays*n_samples >= 2^31 (32-bit g_pts offsets). */
int nslam_cam_grad(const float* cam, const float* c2w, const double* g_pts, const double* z_vals, const float* rays_d,
                   int64_t n_rays, int32_t n_samples, float* g_cam, void* stream);
/* ABI v15: the same gradient from n_parts (1..4) d/dpts buffers — the frozen decoders' shares of
 * nslam_query_bwd_decoders — summed per point in buffer order ((g0 + g1) + g2, float64), over up to
 * 32 workgroups whose partial sums meet in ws (NSLAM_CAM_GRAD_WS_DOUBLES doubles; the last workgroup,
 * by `ticket` — a device uint32 zeroed once and re-armed by the call — adds them in workgroup order:
 * deterministic).  Replaces the buffer adds + single-workgroup nslam_cam_grad of a tracking iteration.
 * nslam_cam_grad is one workgroup of the same kernel over one buffer (no ws, no ticket): up to 1024 points,
 * where this call is one workgroup too, the two give the same bits. */
#define NSLAM_CAM_GRAD_WS_DOUBLES (32 * 12)
int nslam_cam_grad_parts(const float* cam, const float* c2w, const double* const* g_pts, int32_t n_parts,
                         const double* z_vals, const float* rays_d, int64_t n_rays, int32_t n_samples, float* g_cam,
                         double* ws, uint32_t* ticket, void* stream);

/* ABI v19.  The camera gradients of bundle adjustment (Mapper.py:346-363, 441-448, 503): n_cams
 * cameras, camera k's rays being rays [ray_begin[k], ray_begin[k] + n_rays_per) of the batch (one frame
 * of the mapping window each).  cams [n_cams][7] and g_cam [n_cams][7] contiguous f32; c2w: camera k's
 * pose rendered with at c2w + k * c2w_stride floats ([3,4] row-major rows of 4); g_pts as in
 * nslam_cam_grad_parts (1..4 buffers over the whole batch, summed per point in buffer order), z_vals /
 * rays_d over the whole batch.  ray_begin: HOST array.  One launch, up to 32 workgroups per camera;
 * ws: n_cams * NSLAM_CAM_GRAD_WS_DOUBLES doubles; tickets: n_cams device uint32 zeroed once (re-armed by
 * the call).  Per camera the arithmetic and order are nslam_cam_grad_parts' over its slice: the same
 * values bit for bit. */
int nslam_cam_grad_batch(const float* cams, const float* c2w, int64_t c2w_stride, int32_t n_cams,
                         const int64_t* ray_begin, int64_t n_rays_per, const double* const* g_pts, int32_t n_parts,
                         const double* z_vals, const float* rays_d, int64_t n_rays, int32_t n_samples, float* g_cam,
                         double* ws, uint32_t* tickets, void* stream);
/* ABI v23.  A tracking iteration's camera tail fused into nslam_cam_grad_parts' last workgroup: after g_cam
 * is formed, Adam on the camera 7-vector in place (torch.optim.Adam, Tracker.py:126: nslam_adam_step's
 * element update and bias corrections with the step count *step, then *step += 1), *loss_out = the sum of
 * ray_loss[0..n_rays) (nslam_loss_sum_best's fixed-order tree: the same value), and, when best_loss is not
 * NULL, the best-pose update (Tracker.py:245-247) with the stepped camera.  Bit-identical to
 * nslam_cam_grad_parts + nslam_adam_step + nslam_loss_sum_best in that order, in one launch. */
typedef struct nslam_cam_tail {
  float* cam;        /* [7], read by the gradient and stepped in place */
  float* exp_avg;    /* [7] Adam state */
  float* exp_avg_sq; /* [7] */
  float* step;       /* [1] step count */
  float lr, beta1, beta2, eps;
  const double* ray_loss; /* [n_rays] the iteration's per-ray losses */
  int64_t n_rays;
  double* loss_out;  /* [1] */
  double* best_loss; /* [1] or NULL */
  float* best;       /* [7] (with best_loss) */
} nslam_cam_tail;
int nslam_cam_grad_step(const nslam_cam_tail* tail, const float* c2w, const double* const* g_pts, int32_t n_parts,
                        const double* z_vals, const float* rays_d, int64_t n_rays, int32_t n_samples, float* g_cam,
                        double* ws, uint32_t* ticket, void* stream);
/* Additive (ABI stays 24).  nslam_cam_grad_step for the reference's tracking.seperate_LR loop
 * (Tracker.py:202-247, the TUM-RGBD configs): the quaternion and the translation are two Adam groups there,
 * both stepped every iteration — elementwise, that is one 7-vector whose elements 0..3 step with lr_quat and
 * 4..6 with tail.lr, with one step count.  That loop rebuilds camera_tensor = cat([quad, T]) before each
 * iteration, so the candidate it keeps (Tracker.py:245-247) is the camera BEFORE the iteration's step: with
 * best_before_step != 0, best receives the camera values read at kernel entry (0: the stepped camera, as
 * nslam_cam_grad_step).  With lr_quat == tail.lr and best_before_step == 0 the call gives
 * nslam_cam_grad_step's bits (the same kernel). */
typedef struct nslam_cam_tail_lr2 {
  nslam_cam_tail tail;
  float lr_quat;            /* Adam rate of elements 0..3 (the quaternion) */
  int32_t best_before_step; /* the best pose is the camera before the step */
} nslam_cam_tail_lr2;
int nslam_cam_grad_step_lr2(const nslam_cam_tail_lr2* tail, const float* c2w, const double* const* g_pts,
                            int32_t n_parts, const double* z_vals, const float* rays_d, int64_t n_rays,
                            int32_t n_samples, float* g_cam, double* ws, uint32_t* ticket, void* stream);

/* ABI v19: nslam_cam_pose for n cameras in one launch: c2w + k * c2w_stride = get_camera_from_tensor(cams[k]). */
int nslam_cam_pose_batch(const float* cams, float* c2w, int64_t c2w_stride, int32_t n, void* stream);

/* ABI v20.  The frustum voxel selection of Mapper.get_mask_from_c2w (Mapper.py:93-164) after its two
 * projection GEMMs, compacted into a capacity-bound row list (what MappingEngine.bind_masks builds with
 * torch ops, in one pass of four launches).  Inputs in the reference's point order
 * i = (ix*ny + iy)*nz + iz of its meshgrid: uvz [N][3] float64 = (points @ w2c[:3,:3]ᵀ + w2c[:3,3])
 * .double() * (-1, 1, 1) @ Kᵀ and near [N] (uint8 bool) = |points - t|² < 0.25, both formed by the
 * caller; depth [H][W] float32 (the current frame).  Computes uv = (uvz[:2] / (uvz[2] + 1e-5)) as
 * float, cv2.remap's bilinear depth at uv (1/32-pixel fixed-point positions, zero border), zero depths
 * replaced by the maximum over all N points, and mask = (0 < u < W, 0 < v < H, 0 <= -z <= depth + 0.5)
 * | near; then, over voxels v = (iz*ny + iy)*nx + ix (channels-last order): slot[v] = the rank of v among
 * the selected voxels or -1, rows[rank] = v (ascending), *n_live = their count.  mask_ref: optional [N]
 * uint8 mask in the reference order.  ws: nslam_frustum_rows_workspace_size(N) bytes. */
int nslam_frustum_rows(const double* uvz, const uint8_t* near, const float* depth, int32_t H, int32_t W, int32_t nx,
                       int32_t ny, int32_t nz, int32_t* slot, int32_t* rows, int64_t* n_live, uint8_t* mask_ref,
                       void* ws, size_t ws_bytes, void* stream);
size_t nslam_frustum_rows_workspace_size(int64_t n_vox);

/* ABI v21.  The camera iteration's loss and its best-pose bookkeeping in one launch: *loss_out = the sum of
 * ray_loss[0..n_rays) (float64; a fixed-order tree over one workgroup: the same value every call), then,
 * when best_loss is not NULL, the tracker's best-pose update with that sum (Tracker.py:245-247: if loss <
 * best_loss: best_loss = loss, candidate = camera_tensor), on the device: if *loss_out < *best_loss
 * (float64), *best_loss = *loss_out and best[0..n) = cam[0..n) (n <= 64, float32).
 * Replaces optimize_cam_in_batch's loss.sum() (Tracker.py:110-123) and that comparison, so the tracker's
 * camera loop needs no reduction launch and no host read-back.  (ABI v24 removed v20's nslam_track_best,
 * the same update as a launch of its own, which this entry point and nslam_cam_grad_step superseded.) */
int nslam_loss_sum_best(const double* ray_loss, int64_t n_rays, double* loss_out, double* best_loss, const float* cam,
                        float* best, int32_t n, void* stream);

/* ABI v22.  The inverse map for n poses in one launch: cams[k] (7 float32) = get_tensor_from_camera(c2w +
 * k * c2w_stride) (common.py:179-201, as common.camera_tensors restates it on the device: quaternion
 * (w,x,y,z) by the trace / largest-diagonal branch rule in float64, normalised, w >= 0, then T, rounded to
 * float32 once); cams_copy (optional) receives the same 7-vectors.  Replaces the tracker's per-frame
 * camera_tensor and best-pose initialisation (Tracker.py:199-200, 225) and bundle adjustment's camera
 * set-up (Mapper.py:349-363), each ~70 torch launches.  n <= 64, c2w_stride >= 12 floats. */
int nslam_cam_vector_batch(const float* c2w, int64_t c2w_stride, int32_t n, float* cams, float* cams_copy,
                           void* stream);

/* ABI v9.  c2w [3,4] f32 = get_camera_from_tensor(cam [7]) (common.py:137-176, quad2rotation's
 * products and differences, no FMA contraction), one thread.  |q|² is summed ((w²+x²)+y²)+z²;
 * the order of torch's (quad*quad).sum(-1) reduction is not pinned, so the pose matches the
 * reference to within ~1 ulp per entry (bit-identical for most poses), not bit-for-bit. */
int nslam_cam_pose(const float* cam, float* c2w, void* stream);

/* Mesh extraction (Mesher.get_mesh, src/utils/Mesher.py); additive, no ABI bump.
 *
 * Seen / forecast / unseen masks of n points (float32 [n][3]) against n_frames keyframes (Mesher.py:53-212).
 * w2c: device float32 [n_frames][16], row-major world-to-camera matrices (inverted by the caller on the
 * host, as the reference does).  depth: device float32 [n_frames][H][W] (may be NULL with use_all_frames,
 * which reads no depth).  Per point and keyframe, in float32 without FMA contraction: cam = w2c . [p, 1]
 * (four products summed left to right), cam.x negated, uv = K . cam, z = uv.z + 1e-8, uv /= z;
 * seen: 0 < u < W, 0 < v < H, z < 0; forecast: the same with the image grown by 1000 pixels per side.
 * depth_test: the depth is sampled at uv as F.grid_sample does (bilinear, zero padding, align_corners) and
 * seen also needs |(-cam.z) - sample| < 2.4, forecast -cam.z < the maximum sample over ALL points of the
 * chunk of points_batch_size points the point lies in (one maximum per chunk and keyframe, Mesher.py:166).
 * Without depth_test both need -cam.z < max(depth) * 1.1.  forecast &= ~seen, unseen = neither; the three
 * outputs are uint8 [n].  ws: the size function's bytes (the per-chunk maxima). */
int nslam_point_masks(const float* pts, int64_t n, const float* w2c, int32_t n_frames, const float* depth, int32_t H,
                      int32_t W, float fx, float fy, float cx, float cy, int32_t depth_test, int32_t use_all_frames,
                      int64_t points_batch_size, uint8_t* seen, uint8_t* forecast, uint8_t* unseen, void* ws,
                      size_t ws_bytes, void* stream);
size_t nslam_point_masks_workspace_size(int64_t n, int32_t n_frames, int64_t points_batch_size);

/* Marching cubes of vol (device float32 [nx][ny][nz], z fastest) at `level`.  An edge crosses when
 * (a < level) != (b < level); every lattice point owns its +x, +y and +z edges.
 * Pass 1 writes into ws (the size function's bytes = 4 nx ny nz): flags uint8 [N][3] (the owned edge
 * crosses), then ntri uint8 [N] (triangles of the cell whose low corner the point is).  The caller turns both
 * into exclusive int32 prefix sums vert_off [N][3] and face_off [N]; their totals are n_verts and n_faces.
 * Pass 2 writes verts float64 [n_verts][3] = origin + (index + t) * spacing with t = (level - a) / (b - a) in
 * float32 along the crossing edge, and faces int32 [n_faces][3] (vertex ids), vertices in owner-edge order,
 * faces in cell order.  Face normals (right-hand rule) point toward decreasing field values.  The case
 * table is csrc/nslam_mc_table.h (tools/gen_mc_table.py); a cell's triangles are the table's loops in the
 * table's winding, each fanned from the apex that csrc/nslam_mc_fan.h chooses (the rule is stated with
 * nslam_tsdf_mc_emit below, which shares it): no directed edge occurs twice and no two faces use the same
 * three vertices, also where a face of a cell holds four crossings, and the negated volume at the negated
 * level gives the same triangles reversed.  A value equal to the level is not below it (t is then 0 or 1 and
 * triangles of zero area are legitimate); +-inf and NaN values are not pinned down.  A volume with a dimension
 * of 1 holds no cell: pass 1 then flags nothing (n_verts = n_faces = 0), and pass 2 with a count above zero
 * is NSLAM_EINVAL.  NSLAM_EUNSUPPORTED when 3 N >= 2^31. */
int nslam_mc_count(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, void* ws, size_t ws_bytes,
                   void* stream);
int nslam_mc_emit(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, const double* origin,
                  const double* spacing, const int32_t* vert_off, const int32_t* face_off, int64_t n_verts,
                  int64_t n_faces, double* verts, int32_t* faces, void* stream);
size_t nslam_mc_workspace_size(int32_t nx, int32_t ny, int32_t nz);

/* inside[i] = 1 when planes[k] . (p_i, 1) <= 0 for every k (planes: device float64 [m][4], outward
 * normals); pts is float64 [n][3] when is_double, else float32. */
int nslam_points_in_hull(const void* pts, int32_t is_double, int64_t n, const double* planes, int32_t m,
                         uint8_t* inside, void* stream);
/* keep[f] = 0 when all three vertices of face f have vmask set, else 1. */
int nslam_mesh_face_cull(const int32_t* faces, int64_t n_faces, const uint8_t* vmask, int64_t n_verts, uint8_t* keep,
                         void* stream);
/* Connected components over shared vertices: label int32 [n_verts] = the smallest vertex id of the
 * vertex's component (hook and compress, repeated until the device word `flag` stays clear; synchronises the
 * stream once per round); area float64 [n_verts]: area[l] = the summed triangle area of component l (atomic
 * float64 sums: the last bits vary from run to run), 0 elsewhere. */
int nslam_mesh_components(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t* label,
                          double* area, int32_t* flag, void* stream);
/* keep[f] = the face's component is *largest (device int64; NULL = unused) or has area > threshold;
 * used[v] = 1 for every vertex of a kept face (the caller zeroes used). */
int nslam_mesh_select(const int32_t* faces, int64_t n_faces, const int32_t* label, const double* area,
                      const int64_t* largest, double threshold, uint8_t* keep, uint8_t* used, void* stream);
/* out[f][c] = new_id[faces[f][c]]. */
int nslam_mesh_remap(const int32_t* faces, int64_t n_faces, const int32_t* new_id, int32_t* out, void* stream);

/* TSDF fusion of depth frames (the volume of Mesher.get_bound_from_frames, src/utils/Mesher.py:214-279;
 * csrc/nslam_tsdf.hip); additive, no ABI bump.  The algorithm of open3d's ScalableTSDFVolume /
 * UniformTSDFVolume, restated; the library is absent, so parity with it is unpinned.
 *
 * Geometry: voxel edge L (`voxel`), truncation `trunc` with 2 trunc <= 16 L, blocks of 16^3 voxels with edge
 * B = 16.0 * L anchored at the world origin: a point p lies in block floor(p / B) per axis (true floor).
 * Voxel (gx, gy, gz) (global integer index, block * 16 + local) has its centre at ((double)g + 0.5) * L, rounded
 * to float32 for the projection.
 * Storage: a dense int32 table over the box of block indices [block_lo, block_hi) per axis (HOST int32 [3]
 * each; cell key = ((bx - lo.x) * ny + (by - lo.y)) * nz + (bz - lo.z); an entry is a pool id or -1), and a
 * pool of n_pool blocks: tsdf float32 [n_pool][4096], weight float32 [n_pool][4096], colour float32
 * [3][color_stride] with channel c of voxel i at color_pool[c * color_stride + i] (color_stride >= 4096 n_pool),
 * a voxel at (x * 16 + y) * 16 + z of its block.  pool_key int32 [n_pool] is a block's cell key.  The box is not
 * empty, has at most 2^27 cells and indices within +-2^26.  No kernel allocates: the caller grows the pool
 * before nslam_tsdf_integrate, and every table and pool index is checked before use.
 * Poses: c2w float64 [K][16] and w2c float32 [K][16] (row-major, device) are a camera's pose and its inverse
 * (inverted by the caller on the host) in the +z-forward, y-down convention.
 * A depth d is valid when d > 0 && d <= depth_trunc (NaN is not).  Samples are the pixels with u % stride == 0
 * and v % stride == 0.  For a valid sample, in float64 without FMA contraction:
 *   p_cam = (((u - cx) * d) / fx, ((v - cy) * d) / fy, d);   p = ((m0 x + m1 y) + m2 z) + m3 per row of c2w
 * and its blocks are floor((p - trunc) / B) .. floor((p + trunc) / B) per axis (1 to 8 blocks; indices saturate
 * at +-2^30, a p that is not finite makes the sample invalid).
 *
 * nslam_tsdf_block_range: bounds int32 [6] = the per-axis minimum of floor((p - trunc) / B) and maximum of
 * floor((p + trunc) / B) over the valid samples of n_frames >= 1 frames (INT32_MAX / INT32_MIN without one),
 * n_valid int64 = their number.  Integer atomicMin / atomicMax / atomicAdd.
 * nslam_tsdf_touch (n_frames <= 32): mask uint32 [cells], zeroed here, gets bit f ORed into every block of
 * every valid sample of frame f; blocks outside the table are skipped and n_outside int64 counts the samples
 * that have one.
 * nslam_tsdf_integrate (n_frames <= 32): list_key / list_id / list_mask [n_list] are the cell key, pool id and
 * touch mask of the blocks with a non-zero mask.  Every voxel of a listed block loops over the set bits of its
 * block's mask in ascending frame order (a frame updates only the blocks its own samples touched) with its state
 * in registers: one read and one write per call.  Per voxel centre p and frame, float32 without FMA contraction:
 *   cam = ((m0 p.x + m1 p.y) + m2 p.z) + m3 per row of w2c;            skip unless cam.z > 0
 *   uf = ((cam.x * fx) / cam.z + cx) + 0.5f,  vf likewise;               skip unless 1e-4f <= uf < (float)W - 1e-4f
 *   u = (int)uf, v = (int)vf;  d = depth[f][v][u];                       (and vf with H); skip an invalid d
 *   xn = ((float)u - cx) / fx,  yn likewise;  m = sqrtf((xn xn + yn yn) + 1.0f)
 *   sdf = (d - cam.z) * m;                                               skip unless sdf > -trunc
 *   t = fminf(1.0f, sdf * (1.0f / trunc))
 *   tsdf = (tsdf * w + t) / (w + 1.0f);  each colour channel the same way from color uint8 [K][H][W][3] at
 *   (u, v) (when color_pool is not NULL; color must then be given);  w = w + 1.0f
 * nslam_tsdf_mc_count / nslam_tsdf_mc_emit: marching cubes with the voxel centres as lattice points.  A cell
 * is valid when its 8 corners lie in allocated blocks (neighbours through the table) and have weight > 0; a
 * corner is below when tsdf < 0; every voxel owns its +x, +y, +z edges; an edge has a vertex if and only if its
 * ends differ and a valid cell contains it.  Count writes flags uint8 [4096 n_pool][3] (zeroed here) and ntri
 * uint8 [4096 n_pool]; the caller forms the exclusive int32 prefix sums vert_off and face_off, as for
 * nslam_mc_count.  Emit writes verts float64 [n_verts][3] = (((double)g + 0.5) + t) * L along the edge with
 * t = f0 / (f0 - f1) in float32, colors uint8 [n_verts][3] = floor(c + 0.5f) clamped, c = (|f1| c0 + |f0| c1) /
 * (|f0| + |f1|) in float32 (when color_pool and colors are given), and faces int32 [n_faces][3] from the loops
 * of csrc/nslam_mc_table.h with the winding flipped: right-hand normals point toward increasing TSDF, the free
 * side.  A row of that table is a fan per loop from the loop's first vertex; both extractors (csrc/
 * nslam_mc_fan.h) fan every loop (l0 .. l(n-1)) instead from a vertex lk none of whose diagonals (lk, lj), j not
 * adjacent to k, lies in a face of the cell (two edges lie in a common face when they share an (axis, side)
 * pair; every loop of every case has such a vertex), and of those vertices from the one with the lowest edge
 * id: triangles (lk, l(k+i), l(k+i+1)), i = 1 .. n-2, indices mod n, in the row's loop order.  A diagonal then
 * belongs to two triangles of its own cell only, so no mesh edge has more than two faces, also where a face of
 * a cell holds four crossings; and the choice depends neither on where the loop's listing starts nor on its
 * direction, so a case and its complement (the same loops, reversed) get the same triangles, reversed.
 * Vertices are in pool / owner-edge order, faces in pool / cell order.
 * NSLAM_EINVAL (before any device call): a null pointer, n_frames outside its range, stride < 1, voxel or trunc
 * not positive, 2 trunc > 16 voxel, an empty or oversized box.  NSLAM_EUNSUPPORTED: 3 * 4096 * n_pool >= 2^31,
 * H * W >= 2^31.  No valid sample, n_list == 0, n_pool == 0 and no crossing are legal. */
int nslam_tsdf_block_range(const float* depth, const double* c2w, int32_t n_frames, int32_t H, int32_t W, double fx,
                           double fy, double cx, double cy, int32_t stride, float depth_trunc, double voxel,
                           double trunc, int32_t* bounds, int64_t* n_valid, void* stream);
int nslam_tsdf_touch(const float* depth, const double* c2w, int32_t n_frames, int32_t H, int32_t W, double fx,
                     double fy, double cx, double cy, int32_t stride, float depth_trunc, double voxel, double trunc,
                     const int32_t* block_lo, const int32_t* block_hi, uint32_t* mask, int64_t* n_outside,
                     void* stream);
int nslam_tsdf_integrate(const float* depth, const uint8_t* color, const float* w2c, int32_t n_frames, int32_t H,
                         int32_t W, float fx, float fy, float cx, float cy, float depth_trunc, double voxel,
                         float trunc, const int32_t* block_lo, const int32_t* block_hi, const int32_t* list_key,
                         const int32_t* list_id, const uint32_t* list_mask, int64_t n_list, int64_t n_pool,
                         float* tsdf, float* weight, float* color_pool, int64_t color_stride, void* stream);
int nslam_tsdf_mc_count(const float* tsdf, const float* weight, const int32_t* pool_key, int64_t n_pool,
                        const int32_t* table, const int32_t* block_lo, const int32_t* block_hi, uint8_t* flags,
                        uint8_t* ntri, void* stream);
int nslam_tsdf_mc_emit(const float* tsdf, const float* weight, const float* color_pool, int64_t color_stride,
                       const int32_t* pool_key, int64_t n_pool, const int32_t* table, const int32_t* block_lo,
                       const int32_t* block_hi, double voxel, const uint8_t* flags, const uint8_t* ntri,
                       const int32_t* vert_off, const int32_t* face_off, int64_t n_verts, int64_t n_faces,
                       double* verts, uint8_t* colors, int32_t* faces, void* stream);

/* Depth odometry against the TSDF volume above (KinectFusion's ray cast and projective point-to-plane ICP;
 * csrc/nslam_odometry.hip); additive, no ABI bump.  The reference takes its own-data trajectory from open3d's
 * reconstruction system; the library is absent, so parity with it is unpinned.
 * Conventions are the volume's: camera +z forward and y down, poses float64 row-major [16] on the HOST (rows 0..2
 * are read), maps float32 [H][W][3] on the device, an invalid pixel is NaN in all three components.  One stream,
 * no float atomics: every output is the same from run to run.  Every table, pool and image index is checked
 * before use, every loop has a fixed trip-count cap, and a pose or value that is not finite ends as an invalid
 * pixel.  No FMA contraction anywhere.
 *
 * nslam_depth_maps, float32: a depth d is valid when d > 0 && d <= depth_trunc (NaN is not).
 *   xn = ((float)u - cx) / fx,  yn = ((float)v - cy) / fy;  vertex = (xn * d, yn * d, d), NaN when d is invalid
 *   a = vertex(u + 1, v) - vertex(u, v),  b = vertex(u, v + 1) - vertex(u, v)
 *   c = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);  len = sqrtf((c.x c.x + c.y c.y) + c.z c.z)
 *   n = c / len, negated when (n.x p.x + n.y p.y) + n.z p.z > 0 (p the pixel's vertex: n faces the camera)
 * The normal is NaN when one of the three depths is invalid, when fabsf(d(u + 1, v) - d) > max_jump or
 * fabsf(d(u, v + 1) - d) > max_jump, when len is 0 or not finite, and in the last row and the last column.
 *
 * nslam_tsdf_raycast, float32, one thread per pixel: table / pool_key / tsdf / weight / n_pool / block_lo /
 * block_hi / voxel / trunc are the volume's.  m = c2w rounded to float32, L = (float)voxel, B = 16.0f * L,
 * step = 0.75f * (float)trunc, near / far rounded to float32 (distances along the ray, 0 <= near < far).
 *   dir = ((m0 xn + m1 yn) + m2) per row, then dir / sqrtf((dir.x^2 + dir.y^2) + dir.z^2);  o = column 3
 *   samples lie on the lattice t_k = near + (float)k * step, k < 4096, while t_k <= far;  p = o + t * dir
 * A sample in a block floorf(p / B) that is outside the table or not allocated is invalid, and k advances to
 * max(k + 1, ceilf((te - near) / step)), te the smallest ((float)(b + 1) * B - o) / dir over the axes with
 * dir > 0 and ((float)b * B - o) / dir over those with dir < 0: the first lattice sample at or past the
 * block's exit face.  Otherwise the sample is the trilinear value of the 8 voxel centres around p:
 *   g = p / L - 0.5f,  i = floorf(g),  f = g - i;  lerp(a, b, f) = a + f * (b - a) along x, then y, then z
 * valid only if all 8 lie in allocated blocks and have weight > 0.  A valid sample < 0 whose last valid non-zero
 * sample was > 0 ends the march: a hit when the sample right before it was valid, no hit when an invalid
 * sample lies between the pair.  A valid sample > 0 after one < 0 (a back face), far and the cap end it with
 * no hit.  An invalid sample k right after a valid sample > 0 may have stepped over the whole band behind a
 * surface (it is trunc deep less a voxel for the 8 centres, less than a step): one sample is taken midway, at
 * near + ((float)k - 0.5f) * step, and a valid value < 0 there is a hit between the two.  For a hit between (tp, fp) and (tc, fc):  ts = tp + (tc - tp) * (fp / (fp - fc));  with fs the
 * sample at ts, when valid: ts = ts + (tc - ts) * (fs / (fs - fc)) if fs > 0, ts = tp + (ts - tp) * (fp /
 * (fp - fs)) if fs < 0.  vertex = o + ts * dir (world);  g.c = F(p + L e_c) - F(p - L e_c) of the trilinear
 * field, normal = g / sqrtf((g.x^2 + g.y^2) + g.z^2): toward increasing TSDF.  Vertex and normal are NaN for no
 * hit, for an invalid gradient sample and for a zero gradient.  n_pool == 0 is legal (no hit anywhere).
 *
 * nslam_icp_sums, float64 from the float32 maps: for every source pixel with u % stride == 0 && v % stride == 0
 * whose vertex v and normal ns (camera frame, nslam_depth_maps) are not NaN:
 *   p = ((T0 v.x + T1 v.y) + T2 v.z) + T3 per row of the estimate T;  pc = the same with the model camera's w2c
 *   reject unless pc.z > 0;  uf = ((pc.x * fx) / pc.z + cx) + 0.5, vf likewise: reject unless 0 <= uf < Wm and
 *   0 <= vf < Hm;  q, n = the model maps (world frame) at ((int)vf, (int)uf): reject a NaN
 *   d = p - q: reject unless sqrt((d.x d.x + d.y d.y) + d.z d.z) <= dist_th
 *   reject unless (rn.x n.x + rn.y n.y) + rn.z n.z >= cos_th, rn = (T0 ns.x + T1 ns.y) + T2 ns.z per row
 *   r = (n.x d.x + n.y d.y) + n.z d.z;  J = [p.y n.z - p.z n.y, p.z n.x - p.x n.z, p.x n.y - p.y n.x, n]
 * out float64 [29] = the upper triangle of sum J J^T row by row (21), sum J r (6), sum r r, the inlier count: the
 * normal equations of T <- exp(xi) T, xi = (rotation, translation).  nslam_icp_partials(Hs, Ws, stride) =
 * min(ceil(strided pixels / 256), 1024) workgroups: a thread adds its pixels tid, tid + 256 groups, ... in
 * ascending order, a wave adds its 64 threads by the xor butterfly 32, 16, .. 1, a workgroup its four waves in
 * wave order and stores 29 partials into partial float64 [n_partial >= groups][29] with plain stores; a second
 * launch (one wave per sum) adds the workgroups in ascending order.  mask uint8 [Hs][Ws] (or NULL) is zeroed and gets 1 at every
 * accepted pixel.
 * NSLAM_EINVAL (before any device call): a null pointer (mask excepted), a size or stride < 1, fx or fy zero,
 * depth_trunc <= 0, max_jump or dist_th < 0, cos_th outside [-1, 1], near < 0 or far <= near, a T or w2c that
 * is not finite, voxel / trunc / box as for the volume.  NSLAM_EUNSUPPORTED: 3 H W >= 2^31, 3 * 4096 n_pool >=
 * 2^31.  NSLAM_EWORKSPACE: n_partial < nslam_icp_partials. */
int nslam_depth_maps(const float* depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                     float depth_trunc, float max_jump, float* vertex, float* normal, void* stream);
int nslam_tsdf_raycast(const int32_t* table, const int32_t* pool_key, const float* tsdf, const float* weight,
                       int64_t n_pool, const int32_t* block_lo, const int32_t* block_hi, double voxel, double trunc,
                       const double* c2w, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                       double near, double far, float* vertex, float* normal, void* stream);
int64_t nslam_icp_partials(int32_t H, int32_t W, int32_t stride);
int nslam_icp_sums(const float* src_vertex, const float* src_normal, int32_t Hs, int32_t Ws, int32_t stride,
                   const double* T, const float* model_vertex, const float* model_normal, int32_t Hm, int32_t Wm,
                   const double* w2c, double fx, double fy, double cx, double cy, double dist_th, double cos_th,
                   double* partial, int64_t n_partial, double* out, uint8_t* mask, void* stream);

/* The photometric term of the odometry (csrc/nslam_odometry.hip); additive, no ABI bump.  A source frame is
 * aligned to a reference FRAME (not the volume): its grey level against the reference's, seen through the source's
 * own depth.  open3d's hybrid RGB-D odometry, which the reference's own-data path relies on, is absent: parity
 * with it is unpinned.
 *
 * nslam_gray_pyramid, float32, one rounding per written operation: rgb uint8 [H][W][3] -> out float32
 * [nslam_gray_pyramid_size(H, W, levels)], the levels one after the other.  Level 0 is
 *   g = ((0.299f R + 0.587f G) + 0.114f B) / 255.0f
 * Level l + 1 has ceil(h / 2) x ceil(w / 2) pixels (h x w: level l); its pixel (row j, column i) is the 3 x 3
 * binomial of level l around (2 j, 2 i) with indices clamped to the image, rows first:
 *   hrow(y) = (0.25f L[y][2i - 1] + 0.5f L[y][2i]) + 0.25f L[y][2i + 1];  (0.25f hrow(2j - 1) + 0.5f hrow(2j)) +
 *   0.25f hrow(2j + 1)
 * So level l has ceil(H / 2^l) x ceil(W / 2^l) pixels and its pixel k lies at level-0 coordinate k 2^l: exactly the
 * strided pixels nslam_icp_sums visits at stride 2^l.  One launch per level.  levels: 1 .. 8.
 *
 * nslam_photo_sums, float64 from float32 inputs.  src_vertex [Hs][Ws][3] (source camera frame, NaN = invalid);
 * src_gray [src_h][src_w] and ref_gray [ref_h][ref_w]: level `level` of the two pyramids (src_h = ceil(Hs / 2^l)
 * and so on, else NSLAM_EINVAL); ref_vertex [Hr][Wr][3]: the reference frame's own vertex map in ITS camera frame;
 * T: source camera to world; w2c: the reference camera's world-to-camera; fx .. cy: level-0 intrinsics.  With
 * S = 2^level, for every source pixel (u, v) = (k S, m S) whose vertex s is not NaN, in this order:
 *   p = T s, pc = w2c p (each ((m0 x + m1 y) + m2 z) + m3 per row);  reject unless pc.z > 0
 *   x0 = (pc.x * fx) / pc.z + cx,  y0 likewise
 *   occlusion, at the level-0 pixel ((int)(x0 + 0.5), (int)(y0 + 0.5)): reject unless 0 <= x0 + 0.5 < Wr and
 *   0 <= y0 + 0.5 < Hr, the reference vertex there is not NaN and fabs(pc.z - its z) <= depth_th
 *   xl = x0 / S, yl = y0 / S, i0 = floor(xl), j0 = floor(yl): reject unless 0 <= i0, i0 + 1 <= ref_w - 1, 0 <= j0,
 *   j0 + 1 <= ref_h - 1 (a reference level narrower or shorter than 2 pixels accepts nothing);  a = xl - i0,
 *   b = yl - j0;  I00 = ref_gray[j0][i0], I10 = [j0][i0 + 1], I01 = [j0 + 1][i0], I11 = [j0 + 1][i0 + 1]
 *   Iref = (1 - b) * ((1 - a) * I00 + a * I10) + b * ((1 - a) * I01 + a * I11)
 *   gx = ((1 - b) * (I10 - I00) + b * (I11 - I01)) / S,  gy = ((1 - a) * (I01 - I00) + a * (I11 - I10)) / S: the
 *   exact derivative of that interpolant per level-0 pixel
 *   r = Iref - src_gray[m][k]: reject unless fabs(r) <= photo_th (1e300 = off)
 *   z = pc.z;  gc = (gx * (fx / z), gy * (fy / z), gx * (-((fx * pc.x) / (z * z))) + gy * (-((fy * pc.y) / (z * z))))
 *   gw = w2c's rotation transposed times gc: gw.c = (M0c * gc.x + M1c * gc.y) + M2c * gc.z
 *   J = [p.y gw.z - p.z gw.y, p.z gw.x - p.x gw.z, p.x gw.y - p.y gw.x, gw]
 * out float64 [29], partial, n_partial >= nslam_icp_partials(Hs, Ws, S) and mask [Hs][Ws] as for nslam_icp_sums,
 * whose two-stage reduction this shares (the same thread, wave, workgroup and final order): two calls give the
 * same bits.  NSLAM_EINVAL: a null pointer (mask excepted), a size < 1, level outside 0 .. 7, level image sides that
 * do not match, fx or fy zero, an intrinsic, T or w2c that is not finite, depth_th or photo_th negative or NaN.
 * NSLAM_EUNSUPPORTED: 3 H W >= 2^31.  NSLAM_EWORKSPACE: n_partial too small. */
int64_t nslam_gray_pyramid_size(int32_t H, int32_t W, int32_t levels);
int nslam_gray_pyramid(const uint8_t* rgb, int32_t H, int32_t W, int32_t levels, float* out, void* stream);
int nslam_photo_sums(const float* src_vertex, int32_t Hs, int32_t Ws, const float* src_gray, int32_t src_h,
                     int32_t src_w, const float* ref_gray, int32_t ref_h, int32_t ref_w, int32_t level,
                     const float* ref_vertex, int32_t Hr, int32_t Wr, const double* T, const double* w2c, double fx,
                     double fy, double cx, double cy, double depth_th, double photo_th, double* partial,
                     int64_t n_partial, double* out, uint8_t* mask, void* stream);

/* Evaluation (src/tools/cull_mesh.py, src/tools/eval_recon.py; csrc/nslam_eval.hip); additive, no ABI bump.
 * No entry point here uses atomics, with one exception: nslam_raster_depth (and the replay's nslam_scene_render on
 * the same passes) combines its hits with an integer atomicMin, which does not depend on the order.  Every output
 * is the same from run to run.
 *
 * seen[i] = 1 when vertex i (float64 [n][3], cast to float32 as the reference does) projects into the image
 * of any of n_frames cameras (cull_mesh.py:47-71, eval_recon.py:62-88).  w2c: device float32 [n_frames][16],
 * row-major, inverted by the caller on the host.  Per vertex and frame, in float32 without FMA contraction:
 * cam = w2c . [p, 1] (four products summed left to right), cam.x negated, uv = K . cam, z = uv.z + 1e-5,
 * uv /= z; seen when 0 <= -z and 0 < u < W and 0 < v < H (strict).  A seen vertex reads no further frame. */
int nslam_frustum_seen(const double* verts, int64_t n, const float* w2c, int32_t n_frames, int32_t H, int32_t W,
                       float fx, float fy, float cx, float cy, uint8_t* seen, void* stream);

/* area[f] = half the float64 cross-product norm of face f (faces int32 [n_faces][3] into verts float64
 * [n_verts][3]).  The caller forms cdf = cumsum(area) on the device. */
int nslam_face_areas(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, double* area,
                     void* stream);
/* `count` area-weighted surface samples (replaces trimesh.sample.sample_surface): sample i takes three
 * uniforms u_k = (mix64(seed ^ mix64(i * 0x9e3779b97f4a7c15 + k)) >> 11) * 2^-53 (splitmix64's finaliser, the
 * stream of the pixel draws), its face is the first f with cdf[f] > u0 * cdf[n_faces - 1] (binary search: a
 * zero-area face is never chosen), the barycentric pair is reflected (u1 + u2 > 1: 1 - u1, 1 - u2) and the
 * point is (v0 + u1 (v1 - v0)) + u2 (v2 - v0) in float64.  points float64 [count][3], face_id int32 [count]
 * (NaN and -1 when the total area is not positive and finite). */
int nslam_sample_surface(const double* verts, int64_t n_verts, const int32_t* faces, const double* cdf,
                         int64_t n_faces, int64_t count, uint64_t seed, double* points, int32_t* face_id,
                         void* stream);

/* Exact float64 nearest neighbours on a uniform cell grid (replaces scipy's cKDTree and open3d's
 * correspondence search).  The grid is lo (host double [3]), the cell edge `cell` and dims (host int32 [3],
 * each >= 1, at most 2^24 cells in all); a point's cell is clamp(floor((p - lo) / cell), 0, dims - 1) per axis
 * and its key (cx * dims[1] + cy) * dims[2] + cz.
 * Build: keys int32 [m] of the targets (float64 [m][3]).  The caller sorts the targets by key (stable, so a
 * cell keeps ascending original indices), keeps the permutation as orig_idx int32 [m] and forms cell_start
 * int32 [cells + 1], the first sorted target of every cell (searchsorted).
 * Query: one thread per query (float64 [n][3]); the query's cell is clamped into the grid and the rings of
 * cells at Chebyshev radius r = 0, 1, 2, ... are scanned until best <= r * cell (every target beyond ring r
 * differs from the query by more than r * cell along some axis, also for a query outside the box), until
 * r * cell >= max_dist, or until the rings cover the grid.  dist float64 [n], idx int32 [n] (the ORIGINAL
 * target index; ties go to the lowest).  max_dist < 0 or +inf: unbounded; else a neighbour farther than
 * max_dist gives +inf and -1.  NSLAM_EINVAL: m <= 0, a non-finite lo / cell / max_dist, dims < 1 or more than
 * 2^24 cells, n_cell_start != cells + 1. */
int nslam_nn_build(const double* targets, int64_t m, const double* lo, double cell, const int32_t* dims,
                   int32_t* keys, void* stream);
int nslam_nn_query(const double* queries, int64_t n, const double* sorted_targets, const int32_t* orig_idx,
                   int64_t m, const int32_t* cell_start, int64_t n_cell_start, const double* lo, double cell,
                   const int32_t* dims, double max_dist, double* dist, int32_t* idx, void* stream);

/* Point-to-point ICP.  out[i] = R p_i + t with rigid = host double [12], the row-major [3][4] matrix (R | t). */
int nslam_transform_points(const double* pts, int64_t n, const double* rigid, double* out, void* stream);
/* The Kabsch sums over the pairs (a_i = src[i], b_i = targets[idx[i]]) with 0 <= idx[i] < m: per workgroup of
 * 1024 points 17 float64 partials [count, Σa (3), Σb (3), Σ a bᵀ (9, row-major), Σ |a - b|²] into
 * partials[wg][17]; n_partials must equal the partial-count function's value for n.  Wave reduction by
 * __shfl_down, then one LDS step; the caller sums the partials in index order. */
int nslam_kabsch_sums(const double* src, const int32_t* idx, int64_t n, const double* targets, int64_t m,
                      double* partials, int64_t n_partials, void* stream);
int64_t nslam_kabsch_partials(int64_t n);

/* Depth L1 of eval_recon.py's calc_2d_metric (:131-210; csrc/nslam_raster.hip, csrc/nslam_eval.hip); additive.
 *
 * any[b] = 1 when some point of the cloud (float64 [n][3]) passes view b's frustum test: nslam_frustum_seen's
 * test and arithmetic with the roles swapped (check_proj: many views, one cloud).  w2c float32 [n_views][16].
 * The kernel only ever stores 1: the caller zeroes `any` (uint8 [n_views]).  At most 65535 views per call. */
int nslam_views_see_any(const double* pts, int64_t n, const float* w2c, int32_t n_views, int32_t H, int32_t W,
                        float fx, float fy, float cx, float cy, uint8_t* any, void* stream);
/* out[b] = mean over the n_pix pixels of view b of |a - b| (float32 [n_views][n_pix] each), float64: per-thread
 * sums in pixel order, __shfl_down over the wave, one LDS step; no atomics.  Background pixels count. */
int nslam_depth_l1(const float* a, const float* b, int64_t n_views, int64_t n_pix, double* out, void* stream);

/* depth float32 [n_views][H][W]: pixel (u, v) gets the camera-space z (not the ray length) of the nearest
 * intersection of the ray through its centre, direction ((u - cx) / fx, (v - cy) / fy, 1), with any triangle of
 * the mesh (verts float64 [n_verts][3], faces int32 [n_faces][3]); 0 where nothing is hit.  w2c: device float64
 * [n_views][12], the row-major [3][4] world-to-camera matrix of a camera that looks along +z with x right and
 * y down.  Only hits with z_near < z <= z_far count, per pixel (a triangle that crosses the near plane draws
 * its part in front of it); both sides of a triangle are visible; edges are inclusive.  A face with zero area,
 * a non-finite vertex or an index outside the vertices draws nothing.
 * The vertex transform and the intersection are float64 without FMA contraction; z is rounded to float32 once
 * and combined with atomicMin on its bits, so the image is bit-identical from run to run, for every
 * small_max_pixels and every workspace size.
 * Passes (separate launches on the stream; NSLAM_RASTER_ALL runs them in order): CLEAR sets the image to +inf
 * and empties the list; SMALL runs one thread per (face, view), which tests a pixel box of at most
 * small_max_pixels pixels itself and appends a larger one to the list in the workspace (when the list is full
 * it tests that box itself too: nothing is dropped); BIG gives every listed item a workgroup; RESOLVE writes 0
 * for +inf.  The workspace size function gives the bytes for a list of `capacity` items (at least 1); a larger
 * workspace holds a longer list.
 * n_views == 0 or n_faces == 0: NSLAM_OK without a launch (depth is not written).  NSLAM_EINVAL: a negative
 * count, H, W, fx or fy not positive, z_near < 0, z_near >= z_far, small_max_pixels < 0, a null pointer, a
 * workspace shorter than that of one item.  NSLAM_EUNSUPPORTED: more than 65535 views in one call. */
enum { NSLAM_RASTER_CLEAR = 1, NSLAM_RASTER_SMALL = 2, NSLAM_RASTER_BIG = 4, NSLAM_RASTER_RESOLVE = 8,
       NSLAM_RASTER_ALL = 15 };
int nslam_raster_depth(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                       const double* w2c, int32_t n_views, int32_t H, int32_t W, double fx, double fy, double cx,
                       double cy, double z_near, double z_far, int64_t small_max_pixels, int32_t passes,
                       float* depth, void* ws, size_t ws_bytes, void* stream);
size_t nslam_raster_workspace_size(int64_t capacity);

/* The frames of visualizer.py (src/tools/viz.py, in place of its open3d window; csrc/nslam_raster.hip); additive.
 * color uint8 [n_views][H][W][3]: a triangle mesh with vertex colours under a head light, and a set of points
 * drawn as depth-tested square sprites, seen from nslam_raster_depth's cameras (w2c, fx, fy, cx, cy, z_near,
 * z_far and the pixel-centre rays are that entry's).  depth float32 [n_views][H][W] (camera-space z of what the
 * pixel shows, 0 for background) and ids int32 [n_views][H][W] (a face index; -2 - the point's index; -1 for
 * background) are written when not NULL.
 * Mesh: verts float64 [n_verts][3], faces int32 [n_faces][3], vert_colors uint8 [n_verts][3] (NULL: every vertex
 * has the HOST colour grey[3]), normals [n_verts][3] unit vectors, float64 when normals_f64 else float32.
 * Points: points float64 [n_points][3], point_colors uint8 [n_points][3], point_size the sprite's edge in pixels.
 * Visibility: every hit is the 64-bit key (float32 bits of z) << 32 | id, id = the face's index or
 * 0x80000000 | the point's index, combined per pixel with a 64-bit unsigned atomicMin: the nearest hit wins and
 * at equal float32 z the lowest id, so a face beats a point.  Min does not depend on the order: the three
 * images are bit-identical from run to run, for every small_max_pixels and every workspace size.  Faces take
 * nslam_raster_depth's passes and arithmetic (with cull NONE and no points, depth has that entry's bits).
 * cull, by the sign of the edge-function sum d . ((b - a) x (c - a)) of the ray direction d: NONE draws both
 * sides, BACK drops the hits with a positive sum (the right-hand normal points away from the camera), FRONT
 * those with a negative one.
 * A point that is non-finite or whose camera z is not in (z_near, z_far] is dropped; otherwise, projected to
 * (px, py), it covers the pixel centres (x, y) with px - s/2 <= x < px + s/2 and py - s/2 <= y < py + s/2
 * inside the image, all at the point's z.  One thread per (point, view).
 * RESOLVE, one thread per pixel: a point's pixel gets the point's colour; a face's pixel recomputes the face's
 * edge functions there, which over their sum are the barycentrics of the hit, interpolates the vertex colours
 * and normals and writes floor(colour * (ambient + (1 - ambient) * |n . d|) + 0.5) per channel, n the normalised
 * interpolated normal (zero length: |n . d| = 1) and d the unit ray direction, both in the world frame; float64
 * without FMA contraction.  Every other pixel gets the HOST colour background[3].
 * Passes: nslam_raster_depth's CLEAR, SMALL, BIG and RESOLVE on the key image, and NSLAM_SCENE_POINTS between
 * BIG and RESOLVE; NSLAM_SCENE_ALL runs all five.  The workspace holds the list and one key per pixel; its
 * size function gives the bytes for a list of `capacity` items (at least 1) and n_views images of H x W.
 * n_faces == 0 (NULL mesh) draws the points, n_points == 0 (NULL point set) the mesh, both zero clear to the
 * background; n_views == 0: NSLAM_OK without a launch.  NSLAM_EINVAL: nslam_raster_depth's conditions, a cull
 * mode or passes outside the enums, ambient outside [0, 1], point_size not positive, a NULL background, a NULL
 * pointer of a non-empty mesh or point set, a workspace shorter than that of one item.  NSLAM_EUNSUPPORTED:
 * point_size above 64, more than 65535 views in one call. */
enum { NSLAM_CULL_NONE = 0, NSLAM_CULL_BACK = 1, NSLAM_CULL_FRONT = 2 };
enum { NSLAM_SCENE_POINTS = 16, NSLAM_SCENE_ALL = 31 };
int nslam_scene_render(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                       const uint8_t* vert_colors, const void* normals, int32_t normals_f64, const uint8_t grey[3],
                       const double* points, const uint8_t* point_colors, int64_t n_points, double point_size,
                       const double* w2c, int32_t n_views, int32_t H, int32_t W, double fx, double fy, double cx,
                       double cy, double z_near, double z_far, int32_t cull, const uint8_t background[3],
                       double ambient, int64_t small_max_pixels, int32_t passes, uint8_t* color, float* depth,
                       int32_t* ids, void* ws, size_t ws_bytes, void* stream);
size_t nslam_scene_workspace_size(int64_t capacity, int32_t n_views, int32_t H, int32_t W);

/* Lens undistortion of a frame's colour image (src/utils/datasets.py:85-88, the TUM-RGBD configs; additive,
 * csrc/nslam_image.hip): dst = cv2.undistort(src, K, dist) with its defaults — the new camera matrix is K,
 * bilinear, constant zero border — for an interleaved uint8 image [H][W][C], C in 1..4, and the five
 * coefficients dist = (k1, k2, p1, p2, k3) (a HOST array).  For the destination pixel (u, v), in float64
 * without FMA contraction:
 *   x = (u - cx)/fx;  y = (v - cy)/fy;  r2 = x*x + y*y;  rad = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *   xd = x*rad + 2*p1*x*y + p2*(r2 + 2*x*x);   yd = y*rad + p1*(r2 + 2*y*y) + 2*p2*x*y
 *   X = rint((xd*fx + cx)*32);  Y = rint((yd*fy + cy)*32)     (half to even: 1/32-pixel positions, clamped to
 *                                                              ±2^30, NaN to -2^30: far outside either way)
 *   x0 = X >> 5, ax = X & 31, y0 = Y >> 5, ay = Y & 31        (arithmetic shift: floor)
 *   dst[v][u][c] = ((32-ax)(32-ay) S(x0,y0) + ax(32-ay) S(x0+1,y0) + (32-ax)ay S(x0,y0+1) + ax ay S(x0+1,y0+1)
 *                   + 512) >> 10,   S(x, y) = src[y][x][c] inside the image, 0 outside
 * so everything after the one rounding step is exact integer arithmetic (the 10-bit weights equal OpenCV's
 * 15-bit table for 5-bit fractions); nslam_frustum_rows' 1/32-pixel convention.  A restatement of OpenCV from
 * its documented behaviour: parity with the library itself is unpinned (absent).  src and dst are device
 * pointers and may not alias.  One thread per destination pixel, one launch, no host synchronisation.
 * NSLAM_EINVAL: a null pointer, src == dst, a negative size, C outside 1..4, fx or fy zero or NaN.  An empty
 * image (H or W zero) is NSLAM_OK without a launch.  NSLAM_EUNSUPPORTED: H*W >= 2^31. */
int nslam_undistort_u8(const uint8_t* src, int32_t H, int32_t W, int32_t C, double fx, double fy, double cx,
                       double cy, const double dist[5], uint8_t* dst, void* stream);

/* The visualiser's six panels (src/utils/Visualizer.py:57-100; additive, csrc/nslam_vis.hip) as one interleaved
 * uint8 image out [2H][3W][3], written whole on the device:
 *   row 0: input depth | generated depth | depth residual     row 1: input RGB | generated RGB | RGB residual
 * gt_depth [H][W] float32, gt_color [H][W][3] float32, depth [H][W] float64 and color [H][W][3] float32 (what
 * render_img returns), vmax a DEVICE float32 scalar (max(gt_depth), an ordinary reduction: no host sync).
 * Residuals are |gt - rendered| (depth in float64, colour in float32), zero where gt_depth == 0.
 * Depth panels are matplotlib's Normalize(0, vmax) then Colormap.__call__(bytes=True) of "plasma", on the value
 * v as a float64:  t = (vmax == 0 ? 0 : v / vmax) * 256;  NaN -> (0, 0, 0);  t < 0 -> row 0;  t >= 256 -> row 255
 * (v == vmax lands there, as matplotlib moves it; so does anything above);  else row (int)t   of the 256 x 3 byte
 * table csrc/nslam_plasma_lut.h (generated from matplotlib by tools/gen_plasma_lut.py).
 * RGB panels are floor(255 * clip(v, 0, 1) + 0.5) in float32 without FMA contraction, NaN as 0: this project's
 * own rule, not pinned to matplotlib's internal image conversion.
 * One thread per output pixel, one launch, no host synchronisation.  NSLAM_EINVAL: a null pointer or a negative
 * size.  An empty image is NSLAM_OK without a launch.  NSLAM_EUNSUPPORTED: 6*H*W >= 2^31. */
int nslam_vis_panels(const float* gt_depth, const float* gt_color, const double* depth, const float* color,
                     int32_t H, int32_t W, const float* vmax, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * iMAP* (configs/imap.yaml, run.py --imap; additive, no ABI bump): the 256-wide Fourier MLP
 * (csrc/nslam_imap.hip), volume-density compositing (csrc/nslam_composite.hip) and the hierarchical sampler
 * (csrc/nslam_sampler.hip).
 *
 * The model is config.get_model(cfg, nice=False) (src/conv_onet/config.py; decoder.py:91-203 with c_dim=0):
 *   e = sin(p.float() @ B)            B [3][93]
 *   h1 = relu(W0 e + b0)              W0 [256][93]
 *   h(i+1) = relu(Wi hi + bi)         Wi [256][256], i = 1..3
 *   raw = Wo h4 + bo                  Wo [4][256]     (no activation; rgb is not squashed)
 * All arithmetic is float32 (v_mfma_f32_32x32x2_f32 for the four hidden layers); sin / cos are the accurate
 * ones of the Fourier features of the NICE decoders. */
typedef struct nslam_imap_params { /* the module's tensors in their natural (state_dict) layout */
  const float* B;    /* embedder._B            [3][93]                */
  const float* w[4]; /* pts_linears.i.weight   [256][93], [256][256]x3 */
  const float* b[4]; /* pts_linears.i.bias     [256]                  */
  const float* wo;   /* output_linear.weight   [4][256]               */
  const float* bo;   /* output_linear.bias     [4]                    */
} nslam_imap_params;

typedef struct nslam_imap_grads { /* caller-owned, same layouts; the backward ADDS into them */
  float* B;
  float* w[4];
  float* b[4];
  float* wo;
  float* bo;
} nslam_imap_grads;

typedef struct nslam_imap_query { /* the points, as the fused NICE query takes them */
  const double* pts;    /* [n][3] float64, or NULL for the ray form                               */
  const float* rays_o;  /* ray form: p = rays_o[r] + rays_d[r] * z_vals[i] in float64, r = i / n_samples */
  const float* rays_d;
  const double* z_vals; /* [n]                                                                    */
  int64_t n_samples;
  double bound_lo[3];   /* Renderer.eval_points' rule (Renderer.py:43-57): a point that is not strictly */
  double bound_hi[3];   /* inside gets raw[3] = 100 (rgb kept); -inf / +inf switch the test off   */
} nslam_imap_query;

/* The hidden layers read their weights as MFMA fragments: nslam_imap_pack writes them (forward and
 * transposed, zero-padded from 93 to 96) into `packed` (nslam_imap_packed_size() bytes) from `params`.
 * Call it again whenever the parameters changed. */
size_t nslam_imap_packed_size(void);
int nslam_imap_pack(const nslam_imap_params* params, float* packed, void* stream);

/* raw [n][4] float32.  tape (NULL = none; nslam_imap_tape_size(n) bytes) receives the post-ReLU activations
 * h1..h4 of every 128-point tile, which the backward reads (its ReLU masks are h > 0; the embedding is
 * recomputed from the points).  n < 2^31. */
size_t nslam_imap_tape_size(int64_t n);
int nslam_imap_fwd(const nslam_imap_params* params, const float* packed, const nslam_imap_query* q, int64_t n,
                   float* raw, void* tape, void* stream);

/* Backward of nslam_imap_fwd for the cotangent g_raw [n][4]: parameter gradients ADDED into `grads` (NULL =
 * none) and, when g_pts is not NULL, d/dp [n][3] float64 (dp = B (de * cos(pB))) WRITTEN to it.  An
 * out-of-bound point passes nothing through its density (the reference overwrites it in place).
 * Three launches plus a reduction: the cotangent chain da(i-1) = Wi^T (da_i * mask_i) per 128-point tile,
 * split-K weight gradients dW_i = sum_p da_i^T h(i-1) per slab of tiles, and a sum of the slabs' partials in a
 * fixed order — no atomics, so two calls with the same inputs give the same bits. */
size_t nslam_imap_bwd_workspace_size(int64_t n);
int nslam_imap_bwd(const nslam_imap_params* params, const float* packed, const nslam_imap_query* q, int64_t n,
                   const float* g_raw, const void* tape, const nslam_imap_grads* grads, double* g_pts, void* ws,
                   size_t ws_bytes, void* stream);

/* raw2outputs_nerf_color(occupancy=False) (src/common.py:222-245) and its backward:
 *   dists_k = float(z_(k+1) - z_k), the last one 1e10;  dists *= |rays_d|  (float32)
 *   alpha_k = 1 - exp(-relu(raw_k[3]) dists_k);  T_k = prod_(j<k) (1 - alpha_j + 1e-10);  w_k = alpha_k T_k
 *   rgb = sum w_k raw_k[:3] (f32);  depth = sum w_k z_k (f64);  var = sum w_k (z_k - depth)^2 (f64)
 * weights [n][S] float32 (may be NULL) is what the importance sampler reads.  The backward writes g_raw
 * [n][S][4] and, when not NULL, g_rays_d [n][3] (the norm factor's edge).  2 <= S <= 256: S = 1 is
 * NSLAM_EUNSUPPORTED (the reference builds the trailing 1e10 from an empty slice there and composites no sample;
 * one opaque sample, which these kernels would compute, is not its answer). */
int nslam_composite_density_fwd(const float* raw, const double* z_vals, const float* rays_d, int64_t n_rays,
                                int32_t n_samples, double* depth, double* var, float* color, float* weights,
                                void* stream);
int nslam_composite_density_bwd(const float* raw, const double* z_vals, const float* rays_d, int64_t n_rays,
                                int32_t n_samples, const double* g_depth, const double* g_var,
                                const float* g_color, float* g_raw, float* g_rays_d, void* stream);

/* sample_pdf(z_mid, weights[..., 1:-1], N, det=True) (src/common.py:19-63) merged with the coarse samples
 * (sort(cat(z_vals, z_samples)), Renderer.py:182-186): z_out [n][S + N] float64; z_samples [n][N] receives the
 * new samples alone (either may be NULL).  u [N] float32 is the
 * deterministic torch.linspace(0, 1, N).  Per ray: pdf = (w + 1e-5) / sum, a sequential float32 cdf, the
 * right-sided search, denom < 1e-5 -> 1, samples in float64.  3 <= S <= 256, 1 <= N <= 128. */
int nslam_sample_importance(const double* z_vals, const float* weights, const float* u, int64_t n_rays,
                            int32_t n_samples, int32_t n_importance, double* z_out, double* z_samples,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Rendering evaluation (csrc/nslam_metrics.hip; additive, no ABI bump): the sums behind PSNR and rendered-depth
 * L1, and SSIM / MS-SSIM.  Every workgroup writes one float64 partial per quantity into `ws` and a
 * second launch adds the partials in index order: no float atomics, two calls give the same bits.
 *
 * nslam_image_errors: color, gt_color float32 [n_images][n_pix][channels] (channels 1 or 3), depth, gt_depth
 * float32 [n_images][n_pix]; either pair may be NULL (gt_depth alone may be given as the colour mask).  out
 * float64 [n_images][4]:
 *   0  sum (color - gt_color)^2 over the counted colour values, color clamped to [0, 1] first when `clamp`
 *   1  the number of counted colour values: all of them (mask_mode 0) or those of pixels with gt_depth > 0 (1)
 *   2  sum |depth - gt_depth| over the pixels with gt_depth > 0        3  their number
 * A missing pair leaves its two sums 0.  mask_mode 1 with colour needs gt_depth. */
size_t nslam_image_errors_workspace_size(int32_t n_images, int64_t n_pix);
int nslam_image_errors(const float* color, const float* gt_color, const float* depth, const float* gt_depth,
                       int32_t n_images, int64_t n_pix, int32_t channels, int32_t mask_mode, int32_t clamp,
                       double* out, void* ws, size_t ws_bytes, void* stream);

/* nslam_ssim: x, y float32 [n_images][H][W][channels] (channels 1 or 3); out float64
 * [n_images][levels][channels][2]: the spatial means of the SSIM map and of the CS map.
 *   window (HOST, 11 floats): g[i] = exp(-(i-5)^2 / (2 1.5^2)) / sum, computed in float64 and rounded; it is
 *   applied along x, then along y ("valid" correlation: the maps are (h-10) x (w-10)), in float32, taps in
 *   ascending order, to x, y, x^2, y^2 and xy;  C1 = (0.01 L)^2, C2 = (0.03 L)^2 for L = data_range;
 *   cs = (2 sxy + C2) / (sx + sy + C2),  ssim = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs.
 * levels is 1 or 5.  Between levels both images are averaged over 2x2 blocks with stride 2 (an odd side is first
 * padded with one zero row / column on each side; the divisor stays 4), so a side s becomes (s + 1) / 2.
 * levels = 1 needs min(H, W) >= 11, levels = 5 needs min(H, W) > 160; anything else is NSLAM_EINVAL.  ws holds
 * the planar pyramid and the partials. */
size_t nslam_ssim_workspace_size(int32_t n_images, int32_t H, int32_t W, int32_t channels, int32_t levels);
int nslam_ssim(const float* x, const float* y, int32_t n_images, int32_t H, int32_t W, int32_t channels,
               double data_range, const float* window, int32_t levels, double* out, void* ws, size_t ws_bytes,
               void* stream);

enum { NSLAM_WS_SAMPLER = 0 };
size_t nslam_workspace_size(int which, int64_t n);

const char* nslam_strerror(int code);
int nslam_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NSLAM_H */
