// nslam_query_multi.hip — ABI v10 nslam_query_bwd_decoders (the mask-only backward of several decoders
// in one launch, k_dec_bwd_multi in nslam_query_bwd.h) and ABI v16 nslam_color_wgrad (the colour
// decoder's parameter gradients, k_color_wgrad in nslam_color_wgrad.hip).  Its own translation unit:
// the multi-decoder kernel instantiates every decoder's backward tile.
#include "nslam_query_bwd.h"

using namespace nslamq;

extern "C" int nslam_query_bwd_decoders(const nslam_query_cfg* cfg, int32_t dec_mask, const double* pts,
                                        int64_t n_pts, const float* g_raw, double* const* g_pts, void* stream) {
  const int rc = check_cfg(cfg, true);
  if (rc) return rc;
  if (dec_mask <= 0 || dec_mask > 15) return NSLAM_EINVAL;
  if (check_points(cfg, pts, n_pts, g_raw != nullptr)) return NSLAM_EINVAL;
  if (cfg->need_pts_grad && n_pts > 0 && !g_pts) return NSLAM_EINVAL;
  MultiDecArgs m{};
  for (int d = 0; d < 4; ++d) {
    if (!((dec_mask >> d) & 1)) continue;
    if (!stage_uses(cfg->stage, d)) return NSLAM_EINVAL;
    // parameter gradients are not formed here (the colour decoder's: nslam_color_wgrad)
    if (cfg->dgrad[d].base) return NSLAM_EUNSUPPORTED;
    if (cfg->need_pts_grad && n_pts > 0 && !g_pts[d]) return NSLAM_EINVAL;
    m.dec[m.ndec] = d;
    m.gp[m.ndec] = cfg->need_pts_grad ? g_pts[d] : nullptr;
    ++m.ndec;
  }
  if (n_pts > 0 && !cfg->saved_masks) return NSLAM_EUNSUPPORTED;
  if (n_pts == 0) return NSLAM_OK;
  const int64_t tiles = (n_pts + 31) / 32;
  const int64_t groups = (tiles + kWavesBwd - 1) / kWavesBwd;
  QueryKArgs a{*cfg, pts, n_pts, nullptr, g_raw, nullptr};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(groups * m.ndec)), block(64 * kWavesBwd);
  if (cfg->need_pts_grad)
    hipLaunchKernelGGL((k_dec_bwd_multi<true>), grid, block, 0, s, a, m);
  else
    hipLaunchKernelGGL((k_dec_bwd_multi<false>), grid, block, 0, s, a, m);
  return hip_status();
}

// ------------------------------------------------------------------------------------------
// Live-point lists: for each decoder, the points with at least one frustum-selected corner in its grid
// (slot >= 0), ascending.  With a compacted grid gradient (nslam_grid.slot) the mask-only mapping backward
// has no other output than the scatter into selected rows, so every other point is work its result
// does not need.  Three launches, deterministic, no cross-workgroup waiting:
//   k_live_flags  one thread per point: the kernels' own load_point + grid_corners (so liveness is what
//                 resolve_corners sees), a 64-point ballot per wave and a count per 256-point block;
//   k_live_scan   one workgroup per decoder: exclusive scan of the block counts (in place), n_live;
//   k_live_emit   one thread per point: block offset + ballot popcounts = its position in the list.
// ------------------------------------------------------------------------------------------
namespace {
constexpr int kLiveBlock = 256;  // points per workgroup of the flag / emit kernels (4 waves)

struct LiveArgs {
  int ndec;
  int dec[4];
  int32_t* idx[4];
  int64_t* n[4];
};
struct LiveWs {
  uint64_t* ballot;  // [ndec][nwaves]
  uint32_t* count;   // [ndec][nblocks]: block counts, then their exclusive prefix sums
  int64_t nwaves, nblocks;
};

__global__ __launch_bounds__(kLiveBlock) void k_live_flags(QueryKArgs a, LiveArgs m, LiveWs w) {
  __shared__ uint32_t wc[kLiveBlock / 64];
  const int part = (int)blockIdx.y;
  const int dec = part == 0 ? m.dec[0] : part == 1 ? m.dec[1] : part == 2 ? m.dec[2] : m.dec[3];
  const int64_t idx = (int64_t)blockIdx.x * kLiveBlock + threadIdx.x;
  const Pt q = load_point(a, idx);
  const nslam_grid& gr = a.c.grid[dec];
  bool live = q.valid;
  if (gr.slot) {
    Corners cr;
    grid_corners(cr, gr, q);
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k)  // (an out-of-range corner has row 0 and weight exactly 0: never live)
      any = any || (((cr.ok >> k) & 1u) && gr.slot[cr.row[k]] >= 0);
    live = live && any;
  }
  const uint64_t b = __ballot(live);
  const int wave = wave_id();
  if ((threadIdx.x & 63) == 0) {
    w.ballot[(size_t)part * w.nwaves + (size_t)blockIdx.x * (kLiveBlock / 64) + wave] = b;
    wc[wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x == 0) w.count[(size_t)part * w.nblocks + blockIdx.x] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
}

__global__ __launch_bounds__(256) void k_live_scan(LiveArgs m, LiveWs w) {
  __shared__ uint32_t sh[256];
  const int part = (int)blockIdx.x;
  int64_t* nout = part == 0 ? m.n[0] : part == 1 ? m.n[1] : part == 2 ? m.n[2] : m.n[3];
  uint32_t* c = w.count + (size_t)part * w.nblocks;
  const int t = (int)threadIdx.x;
  uint32_t carry = 0;
  for (int64_t base = 0; base < w.nblocks; base += 256) {
    const int64_t i = base + t;
    const uint32_t v = i < w.nblocks ? c[i] : 0u;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // Hillis-Steele inclusive scan of the chunk
      const uint32_t add = t >= d ? sh[t - d] : 0u;
      __syncthreads();
      sh[t] += add;
      __syncthreads();
    }
    if (i < w.nblocks) c[i] = carry + sh[t] - v;
    carry += sh[255];
    __syncthreads();
  }
  if (t == 0) *nout = (int64_t)carry;
}

__global__ __launch_bounds__(kLiveBlock) void k_live_emit(int64_t n, LiveArgs m, LiveWs w) {
  const int part = (int)blockIdx.y;
  int32_t* out = part == 0 ? m.idx[0] : part == 1 ? m.idx[1] : part == 2 ? m.idx[2] : m.idx[3];
  const int64_t idx = (int64_t)blockIdx.x * kLiveBlock + threadIdx.x;
  const int wave = wave_id(), lane = threadIdx.x & 63;
  const uint64_t* bw = w.ballot + (size_t)part * w.nwaves + (size_t)blockIdx.x * (kLiveBlock / 64);
  uint32_t pos = w.count[(size_t)part * w.nblocks + blockIdx.x];
  for (int v = 0; v < wave; ++v) pos += (uint32_t)__popcll(bw[v]);
  const uint64_t b = bw[wave];
  if (!((b >> lane) & 1)) return;  // (a set bit is a valid point: idx < n)
  pos += (uint32_t)__popcll(b & ((uint64_t(1) << lane) - 1));
  if (idx < n && (int64_t)pos < n) out[pos] = (int32_t)idx;
}

inline int64_t live_nblocks(int64_t n) { return (n + kLiveBlock - 1) / kLiveBlock; }
inline size_t live_ws_bytes(int64_t n) {
  const int64_t nb = live_nblocks(n);
  return n > 0 ? (size_t)4 * ((size_t)nb * (kLiveBlock / 64) * 8 + (size_t)nb * 4) : 0;
}
}  // namespace

extern "C" size_t nslam_live_points_workspace_size(int64_t n_pts) { return live_ws_bytes(n_pts); }

extern "C" int nslam_live_points(const nslam_query_cfg* cfg, int32_t dec_mask, const double* pts, int64_t n_pts,
                                 int32_t* const* live_idx, int64_t* const* n_live, void* ws, size_t ws_bytes,
                                 void* stream) {
  const int rc = check_cfg(cfg, true);
  if (rc) return rc;
  if (dec_mask <= 0 || dec_mask > 15 || !live_idx || !n_live) return NSLAM_EINVAL;
  if (check_points(cfg, pts, n_pts, true, /*index32=*/true)) return NSLAM_EINVAL;  // (the lists are int32)
  LiveArgs m{};
  for (int d = 0; d < 4; ++d) {
    if (!((dec_mask >> d) & 1)) continue;
    if (!stage_uses(cfg->stage, d)) return NSLAM_EINVAL;
    if (!n_live[d] || (n_pts > 0 && !live_idx[d])) return NSLAM_EINVAL;
    m.dec[m.ndec] = d;
    m.idx[m.ndec] = live_idx[d];
    m.n[m.ndec] = n_live[d];
    ++m.ndec;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (n_pts == 0) {
    for (int i = 0; i < m.ndec; ++i)
      if (hipMemsetAsync(m.n[i], 0, sizeof(int64_t), s) != hipSuccess) return hip_status();
    return NSLAM_OK;
  }
  if (!ws || ws_bytes < live_ws_bytes(n_pts) || (((uintptr_t)ws) & 7) != 0) return NSLAM_EWORKSPACE;
  LiveWs w;
  w.nblocks = live_nblocks(n_pts);
  w.nwaves = w.nblocks * (kLiveBlock / 64);
  w.ballot = reinterpret_cast<uint64_t*>(ws);
  w.count = reinterpret_cast<uint32_t*>(w.ballot + (size_t)4 * w.nwaves);
  QueryKArgs a{*cfg, pts, n_pts, nullptr, nullptr, nullptr};
  const dim3 grid((unsigned)w.nblocks, (unsigned)m.ndec);
  hipLaunchKernelGGL(k_live_flags, grid, dim3(kLiveBlock), 0, s, a, m, w);
  hipLaunchKernelGGL(k_live_scan, dim3((unsigned)m.ndec), dim3(256), 0, s, m, w);
  hipLaunchKernelGGL(k_live_emit, grid, dim3(kLiveBlock), 0, s, n_pts, m, w);
  return hip_status();
}

// The mask-only mapping backward of nslam_query_bwd_decoders over each decoder's live points only.
extern "C" int nslam_query_bwd_decoders_live(const nslam_query_cfg* cfg, int32_t dec_mask, const double* pts,
                                             int64_t n_pts, const float* g_raw, const int32_t* const* live_idx,
                                             const int64_t* const* n_live, void* stream) {
  const int rc = check_cfg(cfg, true);
  if (rc) return rc;
  if (dec_mask <= 0 || dec_mask > 15 || !live_idx || !n_live) return NSLAM_EINVAL;
  if (check_points(cfg, pts, n_pts, g_raw != nullptr, /*index32=*/true)) return NSLAM_EINVAL;
  if (cfg->need_pts_grad) return NSLAM_EUNSUPPORTED;  // d/dpts is needed for every point
  MultiDecArgs m{};
  for (int d = 0; d < 4; ++d) {
    if (!((dec_mask >> d) & 1)) continue;
    if (!stage_uses(cfg->stage, d)) return NSLAM_EINVAL;
    if (cfg->dgrad[d].base) return NSLAM_EUNSUPPORTED;
    if (!n_live[d] || (n_pts > 0 && !live_idx[d])) return NSLAM_EINVAL;
    m.dec[m.ndec] = d;
    m.live[m.ndec] = live_idx[d];
    m.nlive[m.ndec] = n_live[d];
    ++m.ndec;
  }
  if (n_pts > 0 && !cfg->saved_masks) return NSLAM_EUNSUPPORTED;
  if (n_pts == 0) return NSLAM_OK;
  const int64_t tiles = (n_pts + 31) / 32;
  const int64_t groups = (tiles + kWavesBwd - 1) / kWavesBwd;
  QueryKArgs a{*cfg, pts, n_pts, nullptr, g_raw, nullptr};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(groups * m.ndec)), block(64 * kWavesBwd);
  hipLaunchKernelGGL((k_dec_bwd_multi<false, true>), grid, block, 0, s, a, m);
  return hip_status();
}

// ABI v16: the colour decoder's parameter gradients of a colour-stage backward, from the forward's
// activation tape and ReLU masks and the cotangent g_raw — independent of the lean backward that
// forms the colour grid's gradient (nslam_query_bwd_decoders), so the two may run concurrently.
extern "C" int nslam_color_wgrad(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, const float* g_raw,
                                 void* ws, size_t ws_bytes, void* stream) {
  const int rc = check_cfg(cfg, true);
  if (rc) return rc;
  if (cfg->stage != NSLAM_STAGE_COLOR || n_pts < 0) return NSLAM_EINVAL;
  if (!cfg->dgrad[NSLAM_DEC_COLOR].base || cfg->dgrad[NSLAM_DEC_COLOR].count <= 0) return NSLAM_EUNSUPPORTED;
  if (n_pts > 0 && !cw_tape_path(cfg)) return NSLAM_EUNSUPPORTED;
  if (check_points(cfg, pts, n_pts, g_raw != nullptr)) return NSLAM_EINVAL;
  if (n_pts == 0) return NSLAM_OK;
  if (!ws || ws_bytes < dec_ws_bytes(cfg, NSLAM_DEC_COLOR, n_pts)) return NSLAM_EWORKSPACE;
  QueryKArgs a{*cfg, pts, n_pts, nullptr, g_raw, nullptr};
  return launch_color_wgrad(a, reinterpret_cast<float*>(ws), reinterpret_cast<hipStream_t>(stream));
}
