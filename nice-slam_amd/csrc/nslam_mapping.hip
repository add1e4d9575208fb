// nslam_mapping.hip — the per-iteration glue of Mapper.optimize_map / Tracker.optimize_cam_in_batch
// as single-launch kernels on gfx950, and nothing else:
//   k_gather_rays : get_samples (src/common.py:74-134) for all frames of the window at once, with
//                   the inside-mask prefilter (Mapper.py:469-481, Tracker.py:93-104) folded in;
//   k_adam        : torch.optim.Adam's update (Mapper.py:504, Tracker.py:126) over dense parameter
//                   segments and frustum-masked grid rows (Mapper.py:314-333) in one launch
//                   (k_adam_steps: the step counts, when no ticket is given);
//   k_rows_xfer   : pack / unpack of the frustum-selected gradient rows for the exchange between ranks.
// All are HBM/latency-bound elementwise work: coalesced float4 rows where the layout allows, LDS only
// for the gather's per-workgroup counts.  The camera chain (gradient, pose, loss) is nslam_camera.hip.
#include <math.h>

#include "nslam_dev.h"

namespace {

// ------------------------------------------------------------------------------------------
// pixel sampling + rays + inside mask
// ------------------------------------------------------------------------------------------
struct GatherArgs {
  nslam_frame fr[NSLAM_MAX_FRAMES];
  int32_t nf;
  int64_t n_per, n;
  const int64_t* pix;
  int32_t W, h0, w0, ww;
  float fx, fy, cx, cy;
  int32_t use_bound;
  double lo[3], hi[3];
  float *ro, *rd, *gd, *gc;
  uint8_t* keep;
  nslam_draw draw;  // pix == NULL: in-kernel draws
  int64_t wn;       // window size (h1-h0)*(w1-w0)
  int64_t* n_kept;
};

// splitmix64 finaliser: a counter-based stream (seed, draw counter, ray) -> 64 uniform bits
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// torch.max / torch.min propagate NaN
__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double nanmin(double a, double b) { return (a < b || a != a) ? a : b; }

// One pixel of frame f at window index k: rays_o/rays_d (common.py:74-89), gt depth (0 when the
// inside mask drops the ray), the pixel offset and the mask.
struct RayAt {
  float o[3], d[3], gt;
  int64_t px;
  bool kp;
};

__device__ __forceinline__ RayAt ray_at(const GatherArgs& a, int f, int64_t k) {
  const nslam_frame& fr = a.fr[f];
  // ABI v21: a frame given by its camera 7-vector has its pose formed here (the same values as nslam_cam_pose);
  // either way the 12 entries sit in registers (no pointer that could be private or global memory)
  float P[12];
  if (fr.cam) {
    cam_pose_one(fr.cam, P);
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = fr.c2w[e];
  }
  RayAt r;
  // window index -> (row, col); torch.linspace(W0, W1-1, W1-W0) holds exact integers
  const int64_t row = k / a.ww, col = k - row * a.ww;
  r.px = (a.h0 + row) * a.W + (a.w0 + col);
  const float i = (float)(a.w0 + col), j = (float)(a.h0 + row);
  // dirs = ((i-cx)/fx, -(j-cy)/fy, -1); rays_d = sum(dirs * c2w[:3,:3], -1) (common.py:80-86).
  // On the GPU torch divides by a CPU scalar as a multiply by its float reciprocal
  // (BinaryDivTrueKernel), which is what the reference runs: do the same.
  const float d0 = (i - a.cx) * (1.f / a.fx);
  const float d1 = -(j - a.cy) * (1.f / a.fy);
  const float d2 = -1.f;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float* c2w = &P[4 * m];
    // torch's 3-element sum reduces as (p0 + p2) + p1 on this device (tools/probes/rays_order.py)
    r.d[m] = (d0 * c2w[0] + d2 * c2w[2]) + d1 * c2w[1];
    r.o[m] = c2w[3];
  }
  r.gt = fr.depth[r.px];
  r.kp = true;
  if (a.use_bound) {  // t = (bound - o) / d (float64); t_exit = min_axis max(t_lo, t_hi) >= gt
    double tex = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double tl = (a.lo[m] - (double)r.o[m]) / (double)r.d[m];
      const double th = (a.hi[m] - (double)r.o[m]) / (double)r.d[m];
      const double tm = nanmax(tl, th);
      tex = m == 0 ? tm : nanmin(tex, tm);
    }
    r.kp = tex >= (double)r.gt;
  }
  if (!r.kp) r.gt = 0.f;
  return r;
}

// select_uv's draw for global ray g: Lemire's multiply-shift maps 32 uniform bits onto [0, wn)
// (bias < wn / 2^32)
__device__ __forceinline__ int64_t draw_k(const GatherArgs& a, uint64_t ctr, uint64_t g) {
  return (int64_t)(((mix64(a.draw.seed ^ mix64(ctr * 0x9e3779b97f4a7c15ull + g)) >> 32) * (uint64_t)a.wn) >> 32);
}

__global__ __launch_bounds__(256) void k_gather_rays(GatherArgs a) {
  const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < NSLAM_MAX_FRAMES) {  // the poses formed from 7-vectors, for later launches
    const nslam_frame& fr = a.fr[threadIdx.x];
    if ((int)threadIdx.x < a.nf && fr.cam && fr.c2w_out) cam_pose_one(fr.cam, fr.c2w_out);
  }
  __shared__ uint64_t ctr;
  __shared__ uint32_t wred[2][4];
  const bool drawn = a.pix == nullptr;
  if (threadIdx.x == 0)  // in-kernel draws: every workgroup reads the counter before the last one bumps it
    ctr = drawn ? __hip_atomic_load(a.draw.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
  __syncthreads();
  bool kp = false;
  uint32_t mkey = 0;  // max over the global batch's kept gt (key 0: below every float)
  if (ray < a.n) {
    const int f = (int)(ray / a.n_per);
    const int64_t kk = ray - (int64_t)f * a.n_per;
    const uint64_t g0 = (uint64_t)f * (uint64_t)(a.n_per * a.draw.world) + (uint64_t)kk;  // rank 0's slot
    const int64_t k = drawn ? draw_k(a, ctr, g0 + (uint64_t)a.draw.rank * a.n_per) : a.pix[ray];
    const RayAt r = ray_at(a, f, k);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      a.ro[ray * 3 + m] = r.o[m];
      a.rd[ray * 3 + m] = r.d[m];
      a.gc[ray * 3 + m] = a.fr[f].color[r.px * 3 + m];
    }
    a.gd[ray] = r.gt;
    if (a.keep) a.keep[ray] = r.kp ? 1 : 0;
    kp = r.kp;
    if (a.draw.gt_max) {  // the other ranks' rays of this slot, re-drawn here (no collective)
      mkey = fkey(r.gt);
      for (int j = 0; j < a.draw.world; ++j)
        if (j != a.draw.rank) mkey = max(mkey, fkey(ray_at(a, f, draw_k(a, ctr, g0 + (uint64_t)j * a.n_per)).gt));
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (a.n_kept) {  // kept-ray count: wave ballot, one atomic per workgroup
    const int cnt = __popcll(__ballot(kp));
    if (lane == 0) wred[0][wv] = (uint32_t)cnt;
  }
  if (a.draw.gt_max) {
    mkey = wave_max_u32(mkey);
    if (lane == 0) wred[1][wv] = mkey;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.n_kept) {
      const uint32_t tot = wred[0][0] + wred[0][1] + wred[0][2] + wred[0][3];
      if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(a.n_kept), (unsigned long long)tot);
    }
    if (a.draw.gt_max)
      __hip_atomic_fetch_max(a.draw.gt_max_key, max(max(wred[1][0], wred[1][1]), max(wred[1][2], wred[1][3])),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn) {
      // count this workgroup in (release: its max is in); the last one (acquire: sees every max)
      // publishes the batch max, re-arms the key and ticket and advances the draw counter
      const uint32_t t = __hip_atomic_fetch_add(a.draw.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (t == gridDim.x - 1) {
        if (a.draw.gt_max) {
          const uint32_t key = __hip_atomic_exchange(a.draw.gt_max_key, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          *a.draw.gt_max = fkey_inv(key);
        }
        __hip_atomic_store(a.draw.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a.draw.counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Adam
// ------------------------------------------------------------------------------------------
struct AdamArgs {
  nslam_adam_seg seg[NSLAM_ADAM_MAX_SEGS];
  int64_t blk0[NSLAM_ADAM_MAX_SEGS + 1];  // first workgroup of each segment
  int32_t nseg;
  float b1, b2, eps;
  int32_t zero_grad;
  uint32_t* ticket;  // non-NULL: the last workgroup advances the step counts (no second launch)
};

constexpr int kAdamThreads = 256;
constexpr int kAdamItems = 4;  // float4 rows (or floats) per thread: 4 x 4 loads in flight

// A segment with a device live count (ABI v19 n_live) gets at most kLiveBlocks workgroups, which stride
// over the live rows: its launch does not scale with the capacity it is sized for.
constexpr int64_t kLiveBlocks = 512;

// the element update and its coefficients: adam_coef / adam_one (nslam_dev.h)
__global__ __launch_bounds__(kAdamThreads) void k_adam(AdamArgs a) {
  const int64_t b = blockIdx.x;
  int s = 0;
  while (s + 1 < a.nseg && b >= a.blk0[s + 1]) ++s;
  const nslam_adam_seg& sg = a.seg[s];
  const float step = *sg.step;
  const auto coef = [&] { return adam_coef(a.b1, a.b2, a.eps, sg.lr, step); };
  if (sg.n_live) {  // stride the live rows (the same per-row update as the one-pass path)
    nslam_adam_seg live = sg;
    live.n = *sg.n_live < sg.n ? *sg.n_live : sg.n;
    live.n_live = nullptr;
    const int64_t need = adam_segment_blocks<kAdamItems>(live, kAdamThreads);
    const int64_t assigned = a.blk0[s + 1] - a.blk0[s];
    for (int64_t lb = b - a.blk0[s]; lb < need; lb += assigned)
      adam_segment_block<kAdamItems>(live, coef, lb, a.zero_grad, (int)threadIdx.x, kAdamThreads);
  } else {
    adam_segment_block<kAdamItems>(sg, coef, b - a.blk0[s], a.zero_grad, (int)threadIdx.x, kAdamThreads);
  }
  if (a.ticket) {
    // Every workgroup read its segment's step count at its start (the value was consumed long
    // before this point), so once all of them have drawn a ticket no read is outstanding and the
    // last one may advance every count and re-arm the ticket for the next launch.  The next
    // launch is a later kernel: its reads see these stores across the kernel boundary.
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (tk == gridDim.x - 1) {
        for (int k = 0; k < a.nseg; ++k) *a.seg[k].step += 1.f;
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// Without a ticket, every segment's step advances after the update kernel in its own single-wave
// launch (stream order makes it see all reads of the old count).  The ticket path above needs no
// release fence: the last workgroup reads nothing the other workgroups wrote (only the ticket, an
// atomic), and the counts it stores are read by later kernels only, across the kernel boundary.
__global__ __launch_bounds__(64) void k_adam_steps(AdamArgs a) {
  if (threadIdx.x < (unsigned)a.nseg) *a.seg[threadIdx.x].step += 1.f;
}

// ------------------------------------------------------------------------------------------
// sparse gradient exchange (ray-sharded mapping)
// ------------------------------------------------------------------------------------------
// Only the frustum-selected rows of a grid gradient reach Adam (Mapper.py:314-333,394-401), so
// only they are summed across ranks: pack them (+ the dense decoder gradients) into one buffer,
// all-reduce it, unpack.  One float4 (rows) or float (tail) per thread; pure HBM copy.
template <bool PACK>
__global__ __launch_bounds__(256) void k_rows_xfer(float* __restrict__ grid, const int32_t* __restrict__ rows,
                                                   int64_t n_rows, int q, float* __restrict__ tail, int64_t n_tail,
                                                   float* __restrict__ buf) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nv = n_rows * q;
  if (e < nv) {
    const int64_t ri = e / q, part = e - ri * q;
    f32x4* gp = reinterpret_cast<f32x4*>(grid + ((int64_t)rows[ri] * q + part) * 4);
    f32x4* bp = reinterpret_cast<f32x4*>(buf + e * 4);
    if (PACK)
      *bp = *gp;
    else
      *gp = *bp;
  } else if (e - nv < n_tail) {
    const int64_t t = e - nv;
    if (PACK)
      buf[nv * 4 + t] = tail[t];
    else
      tail[t] = buf[nv * 4 + t];
  }
}

int rows_xfer(bool pack, float* grid, const int32_t* rows, int64_t n_rows, int32_t row_len, float* tail,
              int64_t n_tail, float* buf, void* stream) {
  if (n_rows < 0 || n_tail < 0 || row_len <= 0 || row_len % 4) return NSLAM_EINVAL;
  if ((n_rows > 0 && (!grid || !rows)) || (n_tail > 0 && !tail) || (n_rows + n_tail > 0 && !buf)) return NSLAM_EINVAL;
  if (n_rows > 0 && ((((uintptr_t)grid) | ((uintptr_t)buf)) & 15)) return NSLAM_EINVAL;
  const int64_t work = n_rows * (row_len / 4) + n_tail;
  if (work == 0) return NSLAM_OK;
  if ((work + 255) / 256 >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  const dim3 g((unsigned)((work + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (pack)
    hipLaunchKernelGGL(k_rows_xfer<true>, g, dim3(256), 0, s, grid, rows, n_rows, row_len / 4, tail, n_tail, buf);
  else
    hipLaunchKernelGGL(k_rows_xfer<false>, g, dim3(256), 0, s, grid, rows, n_rows, row_len / 4, tail, n_tail, buf);
  return hip_status();
}

}  // namespace

extern "C" int nslam_rows_pack(const float* grid, const int32_t* rows, int64_t n_rows, int32_t row_len,
                               const float* tail, int64_t n_tail, float* out, void* stream) {
  return rows_xfer(true, const_cast<float*>(grid), rows, n_rows, row_len, const_cast<float*>(tail), n_tail, out,
                   stream);
}

extern "C" int nslam_rows_unpack(const float* in, const int32_t* rows, int64_t n_rows, int32_t row_len, float* grid,
                                 float* tail, int64_t n_tail, void* stream) {
  return rows_xfer(false, grid, rows, n_rows, row_len, tail, n_tail, const_cast<float*>(in), stream);
}

extern "C" int nslam_gather_rays(const nslam_frame* frames, int32_t n_frames, int64_t n_per, const int64_t* pix,
                                 int32_t H, int32_t W, int32_t h0, int32_t h1, int32_t w0, int32_t w1, float fx,
                                 float fy, float cx, float cy, const double* bound_lo, const double* bound_hi,
                                 float* rays_o, float* rays_d, float* gt_depth, float* gt_color, uint8_t* keep,
                                 const nslam_draw* draw, int64_t* n_kept, void* stream) {
  if (!frames || n_frames <= 0 || n_frames > NSLAM_MAX_FRAMES || n_per < 0) return NSLAM_EINVAL;
  if (H <= 0 || W <= 0 || h0 < 0 || w0 < 0 || h1 > H || w1 > W || h1 <= h0 || w1 <= w0) return NSLAM_EINVAL;
  if ((bound_lo == nullptr) != (bound_hi == nullptr)) return NSLAM_EINVAL;
  const int64_t n = (int64_t)n_frames * n_per;
  if (n == 0) return NSLAM_OK;
  if ((!pix && !draw) || !rays_o || !rays_d || !gt_depth || !gt_color) return NSLAM_EINVAL;
  if (!pix && (!draw->counter || !draw->ticket)) return NSLAM_EINVAL;
  if (!pix && (draw->world < 1 || draw->rank < 0 || draw->rank >= draw->world)) return NSLAM_EINVAL;
  if (!pix && draw->gt_max && !draw->gt_max_key) return NSLAM_EINVAL;
  GatherArgs a{};
  for (int f = 0; f < n_frames; ++f) {
    if (!frames[f].depth || !frames[f].color || (!frames[f].c2w && !frames[f].cam)) return NSLAM_EINVAL;
    a.fr[f] = frames[f];
  }
  a.nf = n_frames;
  a.n_per = n_per;
  a.n = n;
  a.pix = pix;
  a.W = W;
  a.h0 = h0;
  a.w0 = w0;
  a.ww = w1 - w0;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.use_bound = bound_lo != nullptr;
  for (int k = 0; k < 3 && a.use_bound; ++k) {
    a.lo[k] = bound_lo[k];
    a.hi[k] = bound_hi[k];
  }
  a.ro = rays_o;
  a.rd = rays_d;
  a.gd = gt_depth;
  a.gc = gt_color;
  a.keep = keep;
  if (!pix) {
    a.draw = *draw;
  } else {
    a.draw = nslam_draw{};
    a.draw.world = 1;
  }
  a.wn = (int64_t)(h1 - h0) * (w1 - w0);
  a.n_kept = n_kept;
  hipLaunchKernelGGL(k_gather_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_adam_step(const nslam_adam_seg* segs, int32_t n_segs, float beta1, float beta2, float eps,
                               int32_t zero_grad, uint32_t* ticket, void* stream) {
  if (!segs || n_segs <= 0 || n_segs > NSLAM_ADAM_MAX_SEGS) return NSLAM_EINVAL;
  AdamArgs a{};
  int64_t blocks = 0;
  for (int s = 0; s < n_segs; ++s) {
    const nslam_adam_seg& g = segs[s];
    if (g.n < 0 || !g.step || (g.n > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq))) return NSLAM_EINVAL;
    a.seg[s] = g;
    a.blk0[s] = blocks;
    if (g.rows) {
      if (g.row_len <= 0 || g.row_len % 4 || g.row_len / 4 > kAdamThreads) return NSLAM_EINVAL;
      const uintptr_t al = (uintptr_t)g.param | (uintptr_t)g.grad | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq;
      if (al & 15) return NSLAM_EINVAL;
    }
    const int64_t nb = adam_segment_blocks<kAdamItems>(g, kAdamThreads);
    blocks += g.n_live ? (nb < kLiveBlocks ? nb : kLiveBlocks) : nb;
  }
  a.blk0[n_segs] = blocks;
  a.nseg = n_segs;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.zero_grad = zero_grad;
  a.ticket = ticket;
  if (blocks == 0) return NSLAM_EINVAL;  // every segment empty: nothing would advance the steps
  if (blocks >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(kAdamThreads), 0, s, a);
  if (!ticket) hipLaunchKernelGGL(k_adam_steps, dim3(1), dim3(64), 0, s, a);
  return hip_status();
}
