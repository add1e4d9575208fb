// nslam_query.hip — C-ABI entry points of the fused point query (include/nslam.h): forward
// launches (the forward kernels: nslam_query_fwd.h), backward dispatch (the per-decoder backward
// launchers are compiled in nslam_query_dec.hip), the slab reduction of the parameter gradients,
// workspace / tape / mask sizes and the pack layout.
#include <string.h>

#include "nslam_query_fwd.h"
#include "nslam_query_host.h"

using namespace nslamq;

extern "C" int nslam_query_fwd(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, float* raw,
                               void* stream) {
  const int rc = check_cfg(cfg, false);
  if (rc) return rc;
  if (check_points(cfg, pts, n_pts, raw != nullptr)) return NSLAM_EINVAL;
  if (n_pts == 0) return NSLAM_OK;
  QueryKArgs a{*cfg, pts, n_pts, raw, nullptr, nullptr};
  const int64_t tiles = (n_pts + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (cfg->stage) {
    case NSLAM_STAGE_COARSE: hipLaunchKernelGGL(k_query_fwd<NSLAM_STAGE_COARSE>, grid, block, 0, s, a); break;
    case NSLAM_STAGE_MIDDLE: hipLaunchKernelGGL(k_query_fwd<NSLAM_STAGE_MIDDLE>, grid, block, 0, s, a); break;
    case NSLAM_STAGE_FINE: hipLaunchKernelGGL(k_query_fwd<NSLAM_STAGE_FINE>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(k_query_fwd<NSLAM_STAGE_COLOR>, grid, block, 0, s, a); break;
  }
  return hip_status();
}

extern "C" size_t nslam_query_fwd_workspace_size(const nslam_query_cfg* cfg, int64_t n_pts) {
  if (!cfg || n_pts <= 0 || cfg->stage < NSLAM_STAGE_FINE || cfg->stage > NSLAM_STAGE_COLOR) return 0;
  return (((size_t)n_pts * sizeof(float) + 255) & ~(size_t)255) + 256;  // the middle occupancy + 256 reserved
}

// The <STAGE, TAPE> instantiation of the decoder-parallel forward kernel K for cfg: the fine stage, or the
// colour stage with / without the activation tape (local to nslam_query_fwd_ws)
#define COLOR_KERNEL(K) (cfg->act_tape ? K<NSLAM_STAGE_COLOR, true> : K<NSLAM_STAGE_COLOR, false>)
#define STAGE_KERNEL(K) (cfg->stage == NSLAM_STAGE_FINE ? K<NSLAM_STAGE_FINE, false> : COLOR_KERNEL(K))

extern "C" int nslam_query_fwd_ws(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, float* raw, void* ws,
                                  size_t ws_bytes, void* stream) {
  const size_t need = nslam_query_fwd_workspace_size(cfg, n_pts);
  if (need == 0) return nslam_query_fwd(cfg, pts, n_pts, raw, stream);  // coarse / middle: one decoder
  const int rc = check_cfg(cfg, false);
  if (rc) return rc;
  // One kernel serves this entry point (one-wave workgroups per decoder and tile), so cfg->fwd_variant
  // and NSLAM_FWD_MODE only name it: default / units.  A retired or misspelt value is an error, not a
  // silent fallback: it must not run a kernel other than the one asked for.
  static const bool env_ok = [] {
    const char* e = getenv("NSLAM_FWD_MODE");
    return !e || !*e || !strcmp(e, "units");
  }();
  if (cfg->fwd_variant != NSLAM_FWD_DEFAULT && cfg->fwd_variant != NSLAM_FWD_UNITS) return NSLAM_EINVAL;
  if (!env_ok) return NSLAM_EINVAL;
  if (!ws || ws_bytes < need) return NSLAM_EWORKSPACE;
  if (check_points(cfg, pts, n_pts, raw != nullptr) || (((uintptr_t)raw) & 15)) return NSLAM_EINVAL;
  QueryKArgs a{*cfg, pts, n_pts, raw, nullptr, nullptr};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* occ = reinterpret_cast<float*>(ws);  // the middle occupancy [n_pts] (the 256 bytes after it: reserved)
  const int64_t units = (n_pts + 31) / 32 * (cfg->stage == NSLAM_STAGE_COLOR ? 3 : 2);
  hipLaunchKernelGGL(STAGE_KERNEL(k_query_fwd_units), dim3((unsigned)units), dim3(64), 0, s, a, occ);
  if (!cfg->defer_occ)  // else the consumer adds ws on read (nslam_loss_cfg.occ_add)
    hipLaunchKernelGGL(k_occ_combine, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, s, raw, occ, n_pts);
  return hip_status();
}
#undef STAGE_KERNEL
#undef COLOR_KERNEL

// base[j] += sum_b slab[b][j].  A workgroup owns 64 parameters; lane (r, c) of a wave reads the
// float4 c of slab r of every 64th slab group, so the 16 waves x 4 lane rows keep 64 slab streams
// in flight per workgroup (~count/64 workgroups fill the chip; a wave load is 4 x 256-B
// segments).  The 64 partials are combined in LDS in a fixed order: deterministic.
// Defined here once for the library: the decoder launchers (nslam_query_dec.hip) and launch_color_wgrad
// reach it through slab_reduce (nslam_query_host.h).
namespace nslamq {
constexpr int kReduceWaves = 16;
__global__ __launch_bounds__(64 * kReduceWaves) void k_slab_reduce(const float* __restrict__ slab, int64_t nslab,
                                                                   int acc_floats, int count,
                                                                   float* __restrict__ base) {
  __shared__ f32x4 part[kReduceWaves * 4][16];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int c = lane & 15, r = wave * 4 + (lane >> 4);  // r: slab stream 0..63
  const int j = (blockIdx.x * 16 + c) * 4;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (j < count) {
    const float* p = slab + j;
    int64_t b = r;
    for (; b + 64 < nslab; b += 128) {
      s0 += *reinterpret_cast<const f32x4*>(p + b * acc_floats);
      s1 += *reinterpret_cast<const f32x4*>(p + (b + 64) * acc_floats);
    }
    if (b < nslab) s0 += *reinterpret_cast<const f32x4*>(p + b * acc_floats);
  }
  part[r][c] = s0 + s1;
  __syncthreads();
  if (threadIdx.x < 16 && j < count) {
    f32x4 t = part[0][c];
#pragma unroll 8
    for (int k = 1; k < kReduceWaves * 4; ++k) t += part[k][c];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e < count) base[j + e] += t[e];
  }
}

int slab_reduce(const nslam_dec_grad& dg, float* slab, bool folded, int64_t nslab, int64_t blocks, int acc,
                hipStream_t s) {
  const int64_t n = folded ? blocks : nslab;
  const int stride = folded ? acc * kWavesBwd : acc;
  const int64_t nblk = (dg.count + 63) / 64;
  hipLaunchKernelGGL(k_slab_reduce, dim3((unsigned)nblk), dim3(64 * kReduceWaves), 0, s, slab, n, stride,
                     (int)dg.count, dg.base);
  return hip_status();
}
}  // namespace nslamq

extern "C" int nslam_query_bwd_decoder(const nslam_query_cfg* cfg, int32_t dec, int32_t accumulate_pts,
                                       const double* pts, int64_t n_pts, const float* g_raw, double* g_pts, void* ws,
                                       size_t ws_bytes, void* stream) {
  const int rc = check_cfg(cfg, true);
  if (rc) return rc;
  if (dec < 0 || dec > 3 || !stage_uses(cfg->stage, dec)) return NSLAM_EINVAL;
  if (check_points(cfg, pts, n_pts, g_raw != nullptr)) return NSLAM_EINVAL;
  if (cfg->need_pts_grad && n_pts > 0 && !g_pts) return NSLAM_EINVAL;
  if (n_pts == 0) return NSLAM_OK;
  if (cfg->dgrad[dec].base && cfg->dgrad[dec].count <= 0) return NSLAM_EUNSUPPORTED;
  const size_t need = dec_ws_bytes(cfg, dec, n_pts);
  if (ws_bytes < need || (need > 0 && !ws)) return NSLAM_EWORKSPACE;
  QueryKArgs a{*cfg, pts, n_pts, nullptr, g_raw, g_pts};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* slab = reinterpret_cast<float*>(ws);
  const bool first = !accumulate_pts;
  switch (dec) {
    case NSLAM_DEC_COARSE: return dispatch_dec_bwd<NSLAM_DEC_COARSE>(a, first, slab, s);
    case NSLAM_DEC_MIDDLE: return dispatch_dec_bwd<NSLAM_DEC_MIDDLE>(a, first, slab, s);
    case NSLAM_DEC_FINE: return dispatch_dec_bwd<NSLAM_DEC_FINE>(a, first, slab, s);
    default: return dispatch_dec_bwd<NSLAM_DEC_COLOR>(a, first, slab, s);
  }
}

extern "C" size_t nslam_query_bwd_decoder_workspace_size(const nslam_query_cfg* cfg, int32_t dec, int64_t n_pts) {
  if (!cfg || dec < 0 || dec > 3 || n_pts <= 0) return 0;
  return dec_ws_bytes(cfg, dec, n_pts);
}

extern "C" size_t nslam_query_tape_size(int64_t n_pts) {
  if (n_pts <= 0) return 0;
  return (size_t)((n_pts + 31) / 32) * kTapeFloats * sizeof(float);
}

extern "C" size_t nslam_query_saved_size(int64_t n_pts) {
  if (n_pts <= 0) return 0;
  return (size_t)4 * ((n_pts + 31) / 32) * 5 * 64 * sizeof(uint16_t);
}

extern "C" size_t nslam_query_bwd_workspace_size(const nslam_query_cfg* cfg, int64_t n_pts) {
  if (!cfg || n_pts <= 0) return 0;
  return bwd_ws_bytes(cfg, n_pts);
}

extern "C" int nslam_query_bwd(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, const float* g_raw,
                               double* g_pts, void* ws, size_t ws_bytes, void* stream) {
  const int rc = check_cfg(cfg, true);
  if (rc) return rc;
  if (check_points(cfg, pts, n_pts, g_raw != nullptr)) return NSLAM_EINVAL;
  if (cfg->need_pts_grad && n_pts > 0 && !g_pts) return NSLAM_EINVAL;
  if (n_pts == 0) return NSLAM_OK;
  for (int d = 0; d < 4; ++d)
    if (cfg->dgrad[d].base && cfg->dgrad[d].count <= 0)
      return NSLAM_EUNSUPPORTED;
  if (ws_bytes < bwd_ws_bytes(cfg, n_pts) || (bwd_ws_bytes(cfg, n_pts) > 0 && !ws)) return NSLAM_EWORKSPACE;
  QueryKArgs a{*cfg, pts, n_pts, nullptr, g_raw, g_pts};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* slab = reinterpret_cast<float*>(ws);
  int r = NSLAM_OK;
  switch (cfg->stage) {
    case NSLAM_STAGE_COARSE:
      r = dispatch_dec_bwd<NSLAM_DEC_COARSE>(a, true, slab, s);
      break;
    case NSLAM_STAGE_MIDDLE:
      r = dispatch_dec_bwd<NSLAM_DEC_MIDDLE>(a, true, slab, s);
      break;
    case NSLAM_STAGE_FINE:
      r = dispatch_dec_bwd<NSLAM_DEC_MIDDLE>(a, true, slab, s);
      if (!r) r = dispatch_dec_bwd<NSLAM_DEC_FINE>(a, false, slab, s);
      break;
    default:
      r = dispatch_dec_bwd<NSLAM_DEC_MIDDLE>(a, true, slab, s);
      if (!r) r = dispatch_dec_bwd<NSLAM_DEC_FINE>(a, false, slab, s);
      if (!r) r = dispatch_dec_bwd<NSLAM_DEC_COLOR>(a, false, slab, s);
      break;
  }
  return r;
}

extern "C" int nslam_pack_layout(int kind, int nc, int32_t* out, int n) {
  if (!out || n < 4) return NSLAM_EINVAL;
  if (kind == 0) {
    if (nc != 1 && nc != 2) return NSLAM_EINVAL;
    const XyzPack L{nc};
    out[0] = L.total();
    out[1] = L.V();
    out[2] = L.nf();
    out[3] = L.nfrag() - L.nf();
  } else if (kind == 1) {
    const NoXyzPack L;
    out[0] = L.total();
    out[1] = L.V();
    out[2] = L.nf();
    out[3] = L.nfrag() - L.nf();
  } else {
    return NSLAM_EINVAL;
  }
  return 4;
}

#ifdef NSLAM_PHASES
extern "C" int nslam_debug_phases(unsigned long long* out, int64_t n) {
  if (n > (int64_t)5 * kPhaseWaves * 16) n = (int64_t)5 * kPhaseWaves * 16;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), (size_t)n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
#if defined(NSLAM_PHASES) || defined(NSLAM_TIMELINE)
// per-wave timeline {start, end, HW_ID | XCC_ID << 32, tag} of slots 0 forward, 1 mask-only bwd, 2 wgrad
extern "C" int nslam_debug_timeline(unsigned long long* out, int64_t n) {
  if (n > (int64_t)3 * kTlWaves * 4) n = (int64_t)3 * kTlWaves * 4;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl), (size_t)n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
