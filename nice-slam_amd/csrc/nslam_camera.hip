// nslam_camera.hip — the camera chain of tracking (Tracker.optimize_cam_in_batch) and bundle adjustment
// (Mapper.optimize_map's camera tensors) on gfx950:
//   k_cam_grad_parts / k_cam_grad_batch : d loss / d camera 7-vector from the d/dpts buffers (one camera /
//                                         every camera of the window), optionally with the camera's Adam
//                                         step, the loss sum and the best-pose update as a tail;
//   k_cam_pose / k_cam_pose_batch       : get_camera_from_tensor (cam_pose_one, nslam_dev.h);
//   k_cam_vector_batch                  : get_tensor_from_camera;
//   k_loss_sum_best                     : the iteration's loss in a fixed order and the best-pose update.
// All of it is small latency-bound work: float64 sums in a fixed order, so every call gives the same bits.
#include <math.h>

#include "nslam_dev.h"

namespace {

// ------------------------------------------------------------------------------------------
// Camera gradient of a tracking iteration (include/nslam.h nslam_cam_grad*)
// ------------------------------------------------------------------------------------------
constexpr int kCamThreads = 1024;

// The epilogue of the camera gradient (one thread): g_R = A·R, the quaternion VJP of
// quad2rotation, and the translation part.  red[k][0], k < 12: Σ g (k < 3) and A (k = 3..11).
__device__ void cam_grad_epilogue(const float* __restrict__ cam, const float* __restrict__ c2w, const double (*red)[kCamThreads / 64],
                                  float* __restrict__ g_cam, float* __restrict__ g_lds = nullptr) {
  struct Ax {
    const float* cam;
    const float* c2w;
    float* g_cam;
  } a{cam, c2w, g_cam};
  double A[9], R[9], gR[9];
  for (int k = 0; k < 9; ++k) A[k] = red[3 + k][0];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = a.c2w[4 * i + j];
  for (int i = 0; i < 3; ++i)  // g_R = A · R
    for (int j = 0; j < 3; ++j) gR[3 * i + j] = A[3 * i + 0] * R[j] + A[3 * i + 1] * R[3 + j] + A[3 * i + 2] * R[6 + j];
  // quad2rotation (common.py:150-159): R = I + s P(q), q = (w, x, y, z) = indices 0..3.
  // G[a][b] = Σ_ij gR_ij M_ij,ab with the ±1 terms of each entry of P.
  double G[4][4] = {};
  const double* g = gR;
  G[2][2] -= g[0]; G[3][3] -= g[0];
  G[1][2] += g[1]; G[3][0] -= g[1];
  G[1][3] += g[2]; G[2][0] += g[2];
  G[1][2] += g[3]; G[3][0] += g[3];
  G[1][1] -= g[4]; G[3][3] -= g[4];
  G[2][3] += g[5]; G[1][0] -= g[5];
  G[1][3] += g[6]; G[2][0] -= g[6];
  G[2][3] += g[7]; G[1][0] += g[7];
  G[1][1] -= g[8]; G[2][2] -= g[8];
  double q[4], qq = 0.0;
  for (int k = 0; k < 4; ++k) {
    q[k] = a.cam[k];
    qq += q[k] * q[k];
  }
  const double s = 2.0 / qq;
  double Hq[4], qHq = 0.0;
  for (int i = 0; i < 4; ++i) {
    double h = 0.0;
    for (int j = 0; j < 4; ++j) h += (G[i][j] + G[j][i]) * q[j];
    Hq[i] = h;
    qHq += q[i] * h;
  }
  float gc[7];
  for (int i = 0; i < 4; ++i) gc[i] = (float)(s * Hq[i] - 0.5 * s * s * qHq * q[i]);
  for (int k = 0; k < 3; ++k) gc[4 + k] = (float)red[k][0];
  for (int k = 0; k < 7; ++k) a.g_cam[k] = gc[k];
  if (g_lds)
    for (int k = 0; k < 7; ++k) g_lds[k] = gc[k];
}

// One camera's gradient from up to four d/dpts buffers (the frozen decoders' shares, summed per point in
// buffer order: what torch adds in front of the kernel would do, bit for bit) over up to kCamParts
// workgroups; each writes its 12 partial sums to ws, the last to arrive (ticket) adds them in workgroup
// order and runs the epilogue (agent-scope release / acquire around the ticket).  A launch of one
// workgroup (nslam_cam_grad; up to kCamThreads points of the others) touches neither ws nor ticket.
constexpr int kCamParts = 32;
struct CamPartsArgs {
  const float* cam;
  const float* c2w;
  const double* gp[4];
  int32_t nbuf;
  const double* z;
  const float* rd;
  int64_t n;
  int32_t S;
  float* g_cam;
  double* ws;  // [kCamParts][12]
  uint32_t* ticket;
  nslam_cam_tail tail;  // ABI v23 (nslam_cam_grad_step): the camera's Adam step, loss and best pose
  int32_t has_tail;
  // nslam_cam_grad_step_lr2: the quaternion's own rate (elements 0..3; nslam_cam_grad_step passes tail.lr)
  // and whether the best pose is the camera as read at kernel entry (the reference's seperate_LR loop)
  float lr_quat;
  int32_t best_before;
};

// ABI v23: what follows a tracking iteration's camera gradient, in the workgroup that formed it (all its
// threads): the loss sum (k_loss_sum_best's fixed-order tree over its first kTailSum threads: the same
// value), Adam on the 7-vector (adam_coef / adam_one, one element per thread: k_adam's element update, bit
// for bit), the step count, and the best-pose update with the stepped camera.  The camera, its Adam state,
// the step count and the best loss are loaded before the tree (their latency hides behind it); thread 0's
// epilogue left g_cam in g_lds, published by the tree's barriers.  Every read of *step / *best_loss is
// issued before those barriers, so thread 0 may replace them after.  nslam_cam_grad_step_lr2: elements 0..3
// step with a.lr_quat, and with a.best_before the best pose receives the camera loaded above, before the step.
constexpr int kTailSum = 256;
__device__ void cam_tail(const CamPartsArgs& a, const float* g_lds) {
  const nslam_cam_tail& t = a.tail;
  __shared__ double s[kTailSum];
  const int k = threadIdx.x;
  float p = 0.f, m = 0.f, v = 0.f, stp = 0.f;
  double bl = 0.0;
  if (k < 7) {
    p = t.cam[k];
    m = t.exp_avg[k];
    v = t.exp_avg_sq[k];
    stp = *t.step;
    if (t.best_loss) bl = *t.best_loss;
  }
  if (k < kTailSum) {
    double acc = 0.0;
    for (int64_t i = k; i < t.n_rays; i += kTailSum) acc += t.ray_loss[i];
    s[k] = acc;
  }
  __syncthreads();
  for (int w = kTailSum / 2; w > 0; w >>= 1) {
    if (k < w) s[k] += s[k + w];
    __syncthreads();
  }
  if (k >= 7) return;
  const double l = s[0];
  const bool better = t.best_loss && l < bl;  // (NaN: not better, as torch's comparison)
  const float p_before = p;
  const AdamCoef c = adam_coef(t.beta1, t.beta2, t.eps, k < 4 ? a.lr_quat : t.lr, stp);
  adam_one(p, g_lds[k], m, v, c);
  t.cam[k] = p;
  t.exp_avg[k] = m;
  t.exp_avg_sq[k] = v;
  if (better) t.best[k] = a.best_before ? p_before : p;
  if (k == 0) {
    *t.step = stp + 1.f;
    *t.loss_out = l;
    if (better) *t.best_loss = l;
  }
}

// workgroup wg of nwg of one camera's gradient (k_cam_grad_parts: the whole grid; k_cam_grad_batch: the
// x extent of the grid row of camera blockIdx.y).  One point per thread per step (coalesced g_pts rows):
// g_t = Σ g and A = Σ_r g_d,r d_rᵀ, which is linear in the points, = Σ_p (z_p g_p) d_r(p)ᵀ; double
// partials, wave shuffles, then LDS.
__device__ __forceinline__ void cam_grad_parts_body(const CamPartsArgs& a, unsigned wg, unsigned nwg) {
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  const int np = (int)(a.n * a.S);  // 3*np < 2^31 (checked by every entry point): 32-bit g_pts offsets
  for (int p = wg * kCamThreads + threadIdx.x; p < np; p += nwg * kCamThreads) {
    const int r = p / a.S;
    const double zs = a.z[p];
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double v = a.gp[0][p * 3 + k];
      for (int b = 1; b < a.nbuf; ++b) v = v + a.gp[b][p * 3 + k];
      g[k] = v;
      acc[k] += v;
    }
    const double d0 = a.rd[r * 3], d1 = a.rd[r * 3 + 1], d2 = a.rd[r * 3 + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double gz = zs * g[i];
      acc[3 + 3 * i] += gz * d0;
      acc[4 + 3 * i] += gz * d1;
      acc[5 + 3 * i] += gz * d2;
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
  __shared__ double red[12][kCamThreads / 64];
  __shared__ float g_tail[7];
  float* const g_lds = a.has_tail ? g_tail : nullptr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) red[k][wave] = acc[k];
  }
  __syncthreads();
  if (nwg == 1) {  // one workgroup: no partials to publish, no hand-over
    if (threadIdx.x < 12) {  // fixed-order sum over the waves: deterministic
      double t = 0.0;
      for (int w = 0; w < kCamThreads / 64; ++w) t += red[threadIdx.x][w];
      red[threadIdx.x][0] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) cam_grad_epilogue(a.cam, a.c2w, red, a.g_cam, g_lds);
    if (a.has_tail) cam_tail(a, g_lds);
    return;
  }
  if (threadIdx.x < 12) {  // fixed-order sum over the waves, published as this workgroup's partial
    double t = 0.0;
    for (int w = 0; w < kCamThreads / 64; ++w) t += red[threadIdx.x][w];
    a.ws[wg * 12 + threadIdx.x] = t;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    red[0][0] = tk == nwg - 1 ? 1.0 : 0.0;  // "I am last", through the one LDS array
  }
  __syncthreads();
  if (red[0][0] == 0.0) return;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next call
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < 12)  // the workgroups' partials in workgroup order: deterministic
    for (unsigned w = 0; w < nwg; ++w) t += a.ws[w * 12 + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 12) red[threadIdx.x][0] = t;
  __syncthreads();
  if (threadIdx.x == 0) cam_grad_epilogue(a.cam, a.c2w, red, a.g_cam, g_lds);
  if (a.has_tail) cam_tail(a, g_lds);
}

__global__ __launch_bounds__(kCamThreads) void k_cam_grad_parts(CamPartsArgs a) { cam_grad_parts_body(a, blockIdx.x, gridDim.x); }

// ABI v19: every bundle-adjustment camera of the window in one launch (grid row blockIdx.y = camera)
struct CamBatchArgs {
  const float* cams;
  const float* c2w;
  int64_t c2w_stride;
  int64_t r0[NSLAM_MAX_FRAMES];  // first ray of each camera's slice
  int64_t n_per;
  const double* gp[4];
  int32_t nbuf;
  const double* z;
  const float* rd;
  int32_t S;
  float* g_cam;
  double* ws;
  uint32_t* tickets;
};

__global__ __launch_bounds__(kCamThreads) void k_cam_grad_batch(CamBatchArgs b) {
  const int k = (int)blockIdx.y;
  int64_t r0 = 0;
#pragma unroll
  for (int i = 0; i < NSLAM_MAX_FRAMES; ++i)  // selects, not a dynamic index into the by-value argument
    if (i == k) r0 = b.r0[i];
  CamPartsArgs a{};
  a.cam = b.cams + 7 * k;
  a.c2w = b.c2w + b.c2w_stride * k;
  const int64_t p0 = r0 * b.S;
#pragma unroll
  for (int i = 0; i < 4; ++i) a.gp[i] = i < b.nbuf ? b.gp[i] + p0 * 3 : nullptr;
  a.nbuf = b.nbuf;
  a.z = b.z + p0;
  a.rd = b.rd + r0 * 3;
  a.n = b.n_per;
  a.S = b.S;
  a.g_cam = b.g_cam + 7 * k;
  a.ws = b.ws + (int64_t)k * kCamParts * 12;
  a.ticket = b.tickets + k;
  cam_grad_parts_body(a, blockIdx.x, gridDim.x);
}

// what nslam_cam_grad_parts, _step and _batch check alike: the d/dpts buffers, the per-ray inputs and the
// kernel's 32-bit p*3+k index into a g_pts buffer (3*points < 2^31)
int cam_parts_check(const double* const* g_pts, int32_t n_parts, const double* z_vals, const float* rays_d,
                    int64_t n_rays, int32_t n_samples) {
  if (n_rays < 0 || n_samples <= 0 || n_parts < 1 || n_parts > 4 || !g_pts) return NSLAM_EINVAL;
  if (n_rays > 0 && (!z_vals || !rays_d)) return NSLAM_EINVAL;
  for (int b = 0; b < n_parts; ++b)
    if (!g_pts[b]) return NSLAM_EINVAL;
  if (n_rays * (int64_t)n_samples * 3 >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  return NSLAM_OK;
}

// workgroups of one camera's gradient: one per kCamThreads points, 1..kCamParts
unsigned cam_grad_workgroups(int64_t n_rays, int32_t n_samples) {
  const int64_t wg = (n_rays * (int64_t)n_samples + kCamThreads - 1) / kCamThreads;
  return (unsigned)(wg < 1 ? 1 : (wg > kCamParts ? kCamParts : wg));
}

int cam_grad_parts_launch(const float* cam, const float* c2w, const double* const* g_pts, int32_t n_parts,
                          const double* z_vals, const float* rays_d, int64_t n_rays, int32_t n_samples, float* g_cam,
                          double* ws, uint32_t* ticket, const nslam_cam_tail* tail, float lr_quat, int32_t best_before,
                          void* stream) {
  if (!cam || !c2w || !g_cam || !ticket || !ws) return NSLAM_EINVAL;
  if (const int rc = cam_parts_check(g_pts, n_parts, z_vals, rays_d, n_rays, n_samples)) return rc;
  CamPartsArgs a{};
  a.cam = cam;
  a.c2w = c2w;
  for (int b = 0; b < n_parts; ++b) a.gp[b] = g_pts[b];
  a.nbuf = n_parts;
  a.z = z_vals;
  a.rd = rays_d;
  a.n = n_rays;
  a.S = n_samples;
  a.g_cam = g_cam;
  a.ws = ws;
  a.ticket = ticket;
  if (tail) {
    a.tail = *tail;
    a.has_tail = 1;
    a.lr_quat = lr_quat;
    a.best_before = best_before;
  }
  hipLaunchKernelGGL(k_cam_grad_parts, dim3(cam_grad_workgroups(n_rays, n_samples)), dim3(kCamThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

}  // namespace

// ABI v8 entry point: the one-workgroup launch of k_cam_grad_parts over a single d/dpts buffer, which reads
// neither a workspace nor a ticket
extern "C" int nslam_cam_grad(const float* cam, const float* c2w, const double* g_pts, const double* z_vals,
                              const float* rays_d, int64_t n_rays, int32_t n_samples, float* g_cam, void* stream) {
  if (!cam || !c2w || !g_cam || n_rays < 0 || n_samples <= 0) return NSLAM_EINVAL;
  if (n_rays > 0 && (!g_pts || !z_vals || !rays_d)) return NSLAM_EINVAL;
  if (n_rays * (int64_t)n_samples * 3 >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  CamPartsArgs a{};
  a.cam = cam;
  a.c2w = c2w;
  a.gp[0] = g_pts;
  a.nbuf = 1;
  a.z = z_vals;
  a.rd = rays_d;
  a.n = n_rays;
  a.S = n_samples;
  a.g_cam = g_cam;
  hipLaunchKernelGGL(k_cam_grad_parts, dim3(1), dim3(kCamThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_cam_grad_parts(const float* cam, const float* c2w, const double* const* g_pts, int32_t n_parts,
                                    const double* z_vals, const float* rays_d, int64_t n_rays, int32_t n_samples,
                                    float* g_cam, double* ws, uint32_t* ticket, void* stream) {
  return cam_grad_parts_launch(cam, c2w, g_pts, n_parts, z_vals, rays_d, n_rays, n_samples, g_cam, ws, ticket, nullptr,
                               0.f, 0, stream);
}

namespace {
int cam_tail_check(const nslam_cam_tail* tail) {
  if (!tail || !tail->cam || !tail->exp_avg || !tail->exp_avg_sq || !tail->step || !tail->loss_out) return NSLAM_EINVAL;
  if (tail->n_rays < 0 || (tail->n_rays > 0 && !tail->ray_loss) || (tail->best_loss && !tail->best)) return NSLAM_EINVAL;
  return NSLAM_OK;
}
}  // namespace

extern "C" int nslam_cam_grad_step(const nslam_cam_tail* tail, const float* c2w, const double* const* g_pts,
                                   int32_t n_parts, const double* z_vals, const float* rays_d, int64_t n_rays,
                                   int32_t n_samples, float* g_cam, double* ws, uint32_t* ticket, void* stream) {
  if (const int rc = cam_tail_check(tail)) return rc;
  return cam_grad_parts_launch(tail->cam, c2w, g_pts, n_parts, z_vals, rays_d, n_rays, n_samples, g_cam, ws, ticket,
                               tail, tail->lr, 0, stream);
}

// The reference's seperate_LR camera loop (Tracker.py:202-247) on the same kernel: two Adam groups over one
// 7-vector are one elementwise Adam with a per-element rate, and its candidate is the camera before the step.
extern "C" int nslam_cam_grad_step_lr2(const nslam_cam_tail_lr2* tail, const float* c2w, const double* const* g_pts,
                                       int32_t n_parts, const double* z_vals, const float* rays_d, int64_t n_rays,
                                       int32_t n_samples, float* g_cam, double* ws, uint32_t* ticket, void* stream) {
  if (!tail) return NSLAM_EINVAL;
  if (const int rc = cam_tail_check(&tail->tail)) return rc;
  return cam_grad_parts_launch(tail->tail.cam, c2w, g_pts, n_parts, z_vals, rays_d, n_rays, n_samples, g_cam, ws,
                               ticket, &tail->tail, tail->lr_quat, tail->best_before_step != 0, stream);
}

extern "C" int nslam_cam_grad_batch(const float* cams, const float* c2w, int64_t c2w_stride, int32_t n_cams,
                                    const int64_t* ray_begin, int64_t n_rays_per, const double* const* g_pts,
                                    int32_t n_parts, const double* z_vals, const float* rays_d, int64_t n_rays,
                                    int32_t n_samples, float* g_cam, double* ws, uint32_t* tickets, void* stream) {
  if (!cams || !c2w || !g_cam || !ws || !tickets || !ray_begin || n_cams < 1 || n_cams > NSLAM_MAX_FRAMES)
    return NSLAM_EINVAL;
  if (c2w_stride < 12 || n_rays_per < 0) return NSLAM_EINVAL;
  // every slice inside the batch (the kernel reads exactly [ray_begin, ray_begin + n_rays_per) of it)
  for (int k = 0; k < n_cams; ++k)
    if (ray_begin[k] < 0 || ray_begin[k] + n_rays_per > n_rays) return NSLAM_EINVAL;
  if (const int rc = cam_parts_check(g_pts, n_parts, z_vals, rays_d, n_rays, n_samples)) return rc;
  CamBatchArgs b{};
  b.cams = cams;
  b.c2w = c2w;
  b.c2w_stride = c2w_stride;
  for (int k = 0; k < n_cams; ++k) b.r0[k] = ray_begin[k];
  b.n_per = n_rays_per;
  for (int i = 0; i < n_parts; ++i) b.gp[i] = g_pts[i];
  b.nbuf = n_parts;
  b.z = z_vals;
  b.rd = rays_d;
  b.S = n_samples;
  b.g_cam = g_cam;
  b.ws = ws;
  b.tickets = tickets;
  hipLaunchKernelGGL(k_cam_grad_batch, dim3(cam_grad_workgroups(n_rays_per, n_samples), (unsigned)n_cams),
                     dim3(kCamThreads), 0, reinterpret_cast<hipStream_t>(stream), b);
  return hip_status();
}

// ------------------------------------------------------------------------------------------
// pose <-> camera 7-vector
// ------------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(64) void k_cam_pose(const float* __restrict__ cam, float* __restrict__ c2w) {
  if (threadIdx.x == 0) cam_pose_one(cam, c2w);
}

__global__ __launch_bounds__(64) void k_cam_pose_batch(const float* __restrict__ cams, float* __restrict__ c2w,
                                                       int64_t stride, int n) {
  if ((int)threadIdx.x < n) cam_pose_one(cams + 7 * threadIdx.x, c2w + stride * threadIdx.x);
}

// get_tensor_from_camera (common.py:179-201) as common.camera_tensors restates it on the device: rotation →
// quaternion (w,x,y,z) by the trace / largest-diagonal branch rule in float64, normalised, w >= 0, then T;
// rounded to float32 once.  NaN compares false (the last branch, as torch.where's) and survives the clamp.
__device__ __forceinline__ void cam_vector_one(const float* __restrict__ M, float* __restrict__ out,
                                               float* __restrict__ out2) {
  const double r00 = M[0], r01 = M[1], r02 = M[2], r10 = M[4], r11 = M[5], r12 = M[6];
  const double r20 = M[8], r21 = M[9], r22 = M[10];
  const double tr = (r00 + r11) + r22;
  auto root = [](double x) { return 2.0 * sqrt(x < 0.0 ? 0.0 : x); };
  double q[4];
  if (tr > 0.0) {
    const double s = root(tr + 1.0);
    q[0] = 0.25 * s; q[1] = (r21 - r12) / s; q[2] = (r02 - r20) / s; q[3] = (r10 - r01) / s;
  } else if (r00 > r11 && r00 > r22) {
    const double s = root(((1.0 + r00) - r11) - r22);
    q[0] = (r21 - r12) / s; q[1] = 0.25 * s; q[2] = (r01 + r10) / s; q[3] = (r02 + r20) / s;
  } else if (r11 > r22) {
    const double s = root(((1.0 + r11) - r00) - r22);
    q[0] = (r02 - r20) / s; q[1] = (r01 + r10) / s; q[2] = 0.25 * s; q[3] = (r12 + r21) / s;
  } else {
    const double s = root(((1.0 + r22) - r00) - r11);
    q[0] = (r10 - r01) / s; q[1] = (r02 + r20) / s; q[2] = (r12 + r21) / s; q[3] = 0.25 * s;
  }
  const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] = q[i] / nrm;
  const bool flip = q[0] < 0.0;
  float v[7];
  for (int i = 0; i < 4; ++i) v[i] = (float)(flip ? -q[i] : q[i]);
  v[4] = M[3]; v[5] = M[7]; v[6] = M[11];
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  if (out2)
    for (int i = 0; i < 7; ++i) out2[i] = v[i];
}

__global__ __launch_bounds__(64) void k_cam_vector_batch(const float* __restrict__ c2w, int64_t stride, int n,
                                                         float* __restrict__ cams, float* __restrict__ cams2) {
  const int k = threadIdx.x;
  if (k < n) cam_vector_one(c2w + stride * k, cams + 7 * k, cams2 ? cams2 + 7 * k : nullptr);
}

// the loss of a camera iteration (fixed-order sum over one workgroup) and, optionally, the best-pose update
constexpr int kSumThreads = 256;
__global__ __launch_bounds__(kSumThreads) void k_loss_sum_best(const double* __restrict__ rl, int64_t n,
                                                              double* __restrict__ out, double* __restrict__ best_loss,
                                                              const float* __restrict__ cam, float* __restrict__ best,
                                                              int nc) {
  __shared__ double s[kSumThreads];
  double t = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kSumThreads) t += rl[i];
  s[threadIdx.x] = t;
  __syncthreads();
  for (int w = kSumThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  const double l = s[0];
  if (threadIdx.x == 0) *out = l;
  if (!best_loss) return;
  if (!(l < *best_loss)) return;  // (NaN: not better, as torch's comparison)
  __syncthreads();                // (every thread has read *best_loss before it is replaced)
  if ((int)threadIdx.x < nc) best[threadIdx.x] = cam[threadIdx.x];
  if (threadIdx.x == 0) *best_loss = l;
}

}  // namespace

extern "C" int nslam_cam_pose(const float* cam, float* c2w, void* stream) {
  if (!cam || !c2w) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_cam_pose, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), cam, c2w);
  return hip_status();
}

extern "C" int nslam_cam_pose_batch(const float* cams, float* c2w, int64_t c2w_stride, int32_t n, void* stream) {
  if (!cams || !c2w || n < 1 || n > 64 || c2w_stride < 12) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_cam_pose_batch, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), cams, c2w,
                     c2w_stride, (int)n);
  return hip_status();
}

extern "C" int nslam_cam_vector_batch(const float* c2w, int64_t c2w_stride, int32_t n, float* cams, float* cams_copy,
                                      void* stream) {
  if (!c2w || !cams || n < 1 || n > 64 || c2w_stride < 12) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_cam_vector_batch, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), c2w, c2w_stride,
                     (int)n, cams, cams_copy);
  return hip_status();
}

extern "C" int nslam_loss_sum_best(const double* ray_loss, int64_t n_rays, double* loss_out, double* best_loss,
                                   const float* cam, float* best, int32_t n, void* stream) {
  if (!loss_out || n_rays < 0 || (n_rays > 0 && !ray_loss)) return NSLAM_EINVAL;
  if (best_loss && (!cam || !best || n < 1 || n > 64)) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_loss_sum_best, dim3(1), dim3(kSumThreads), 0, reinterpret_cast<hipStream_t>(stream), ray_loss,
                     n_rays, loss_out, best_loss, cam, best, (int)n);
  return hip_status();
}
