#pragma once
// nslam_query_core.h — the device building blocks every translation unit of the fused point query
// shares.  The query, for gfx950: normalise → trilinear gather (channels-last grids) → Fourier
// embedding → tiny MLP decoders on MFMA (v_mfma_f32_32x32x2_f32) → stage combiner → OOB logit, and its
// backward.  Its files, by who needs what:
//   nslam_query_core.h     (here) kernel arguments, the per-point context, the Fourier embedding, the
//                          phase / timeline instrumentation, the saved ReLU masks and the activation
//                          tape, and the decoders' forward chains xyz_forward / noxyz_forward (the
//                          recompute backward runs them too) — every query translation unit
//   nslam_query_fwd.h      the forward kernels — nslam_query.hip only
//   nslam_query_bwd.h      the backward chains, tiles, kernels and their launchers, over
//   nslam_query_scatter.h  the grid-gradient scatter walk — nslam_query_dec.hip (once per decoder) and
//                          nslam_query_multi.hip
//   nslam_query_host.h     argument checks, workspace sizing and the cross-unit declarations; host code
//                          only — every query translation unit
//
// Replaces, per point: Renderer.eval_points (src/utils/Renderer.py:23-61), NICE.forward
// (src/conv_onet/models/decoder.py:312-342), MLP / MLP_no_xyz forward (decoder.py:177-203,
// 262-274), sample_grid_feature (decoder.py:168-175, F.grid_sample) and the autograd backward of
// all of them (Tracker.py:125, Mapper.py:503).
//
// Work decomposition: one wave = one tile of 32 points.  Each lane pair (l, l+32) owns one point;
// the half h = l>>5 gathers/holds the 16 feature channels F(r,h) of that point (nslam_dev.h).
#include "nslam_dev.h"

// Everything lives in a named namespace: the per-decoder backward launchers are explicitly
// instantiated in their own translation units (nslam_query_dec.hip, built once per decoder) so the
// library compiles in parallel; the API translation unit (nslam_query.hip) only declares them
// (nslam_query_host.h).
namespace nslamq {

struct QueryKArgs {
  nslam_query_cfg c;
  const double* pts;
  int64_t n;
  float* raw;          // fwd output [n][4]
  const float* g_raw;  // bwd input  [n][4]
  double* g_pts;       // bwd output [n][3]
};

// ------------------------------------------------------------------------------------------
// per-point context
// ------------------------------------------------------------------------------------------
struct Pt {
  double p[3];
  float x[3];  // p.float() (decoder.py:189)
  bool valid;
  bool inside;
};

__device__ __forceinline__ Pt load_point(const QueryKArgs& a, int64_t idx) {
  Pt q;
  q.valid = idx < a.n;
  const int64_t i = q.valid ? idx : 0;  // invalid tail lanes compute on a real point, write nothing
  if (a.c.rays_o) {  // pts = rays_o + rays_d * z (float64, Renderer.py:172-174); host checks n < 2^31
    const uint32_t r = (uint32_t)i / (uint32_t)a.c.n_samples;
    const double z = a.c.z_vals[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) q.p[k] = (double)a.c.rays_o[r * 3 + k] + (double)a.c.rays_d[r * 3 + k] * z;
  } else {
    q.p[0] = a.pts[i * 3 + 0];
    q.p[1] = a.pts[i * 3 + 1];
    q.p[2] = a.pts[i * 3 + 2];
  }
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q.x[k] = (float)q.p[k];
    in = in && (q.p[k] < a.c.bound_hi[k]) && (q.p[k] > a.c.bound_lo[k]);  // Renderer.py:43-46
  }
  q.inside = in;
  return q;
}

__device__ __forceinline__ void grid_corners(Corners& cr, const nslam_grid& g, const Pt& q) {
  float nc3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) nc3[k] = norm_coord(q.p[k], g.lo[k], g.hi[k]);
  make_corners(cr, nc3, g.dims);
}

// ------------------------------------------------------------------------------------------
// Fourier embedding (decoder.py:26-30): block b, reg r of lane (h,p) is dim k = 32b + F(r,h)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float fourier_arg(const float x[3], float b0, float b1, float b2) {
  return fmaf(x[2], b2, fmaf(x[1], b1, x[0] * b0));
}

// G: B is in global memory (else LDS or generic); see as_global
template <bool COS, bool G = false>
__device__ __forceinline__ f32x16 emb_tile(const float* __restrict__ B, const float x[3], int b, int lane) {
  const int h = lane >> 5;
  f32x16 e;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = 32 * b + 8 * i + 4 * h;
    const f32x4 B0 = G ? *as_global(reinterpret_cast<const f32x4*>(B + k)) : *reinterpret_cast<const f32x4*>(B + k);
    const f32x4 B1 = G ? *as_global(reinterpret_cast<const f32x4*>(B + 96 + k))
                       : *reinterpret_cast<const f32x4*>(B + 96 + k);
    const f32x4 B2 = G ? *as_global(reinterpret_cast<const f32x4*>(B + 192 + k))
                       : *reinterpret_cast<const f32x4*>(B + 192 + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = fourier_arg(x, B0[j], B1[j], B2[j]);
      e[4 * i + j] = COS ? fcos(t) : fsin(t);
    }
  }
  return e;
}

// A wave's LDS scratch is wave-private: ordering LDS writes before other lanes' reads of the same wave needs
// only the wave's own LDS counter drained (and a compiler memory barrier), not a workgroup barrier.
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Phase timing (debug build only, make phases): lane 0 of each backward wave records s_memtime
// at marks 0..15 of its tile into g_phase[decoder][wave][16].
#ifdef NSLAM_PHASES
constexpr int kPhaseWaves = 1 << 15;
// slots: 0 forward, 1..3 decoder backward, 4 k_color_wgrad (per wave: cycles in prod / cons / hand-over)
__device__ unsigned long long g_phase[5 * kPhaseWaves * 16];  // one-TU phases build only
#define PHASE(dec, k)                                                                                     \
  do {                                                                                                    \
    const int64_t w_ = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                     \
    if ((threadIdx.x & 63) == 0 && w_ < kPhaseWaves)                                                      \
      g_phase[((size_t)(dec) * kPhaseWaves + w_) * 16 + (k)] = __builtin_amdgcn_s_memtime();              \
  } while (0)
#else
#define PHASE(dec, k) \
  do {                \
  } while (0)
#endif
// Timeline (make phases, or make timeline: the marks below only, so the kernels keep their production
// register allocation — the phase marks cost the forward 88 VGPRs and its third wave per SIMD): per
// wave of kernel slot k (0 forward, 1 mask-only backward, 2 k_color_wgrad) {start, end} of
// s_memrealtime (100 MHz, one clock for all XCDs), HW_ID | XCC_ID << 32, and a tag
#if defined(NSLAM_PHASES) || defined(NSLAM_TIMELINE)
constexpr int kTlWaves = 1 << 15;
__device__ unsigned long long g_tl[3 * kTlWaves * 4];
__device__ __forceinline__ void tl_mark(int slot, int end, long long tag) {
  const int64_t w_ = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) != 0 || w_ >= kTlWaves) return;
  unsigned long long* o = g_tl + ((size_t)slot * kTlWaves + w_) * 4;
  o[end] = __builtin_amdgcn_s_memrealtime();
  if (!end) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID
    const unsigned xcc = __builtin_amdgcn_s_getreg((15 << 11) | 20);  // HW_REG_XCC_ID
    o[2] = (unsigned long long)hw | ((unsigned long long)(xcc & 15) << 32);
    o[3] = (unsigned long long)tag;
  }
}
#define TL(slot, end, tag) tl_mark(slot, end, tag)
#else
#define TL(slot, end, tag) \
  do {                     \
  } while (0)
#endif

// ReLU masks saved by the forward: [decoder][tile][layer][64 lanes] uint16 (one 128-B row per layer)
__device__ __forceinline__ uint16_t* mask_slot(const QueryKArgs& a, int dec, int64_t tile) {
  const int64_t ntiles = (a.n + 31) / 32;
  return a.c.saved_masks + ((size_t)dec * ntiles + tile) * 5 * 64;
}
__device__ __forceinline__ void save_masks(const QueryKArgs& a, int dec, int64_t tile, const uint32_t m[5],
                                           int lane) {
  if (!a.c.saved_masks) return;
  uint16_t* s = mask_slot(a, dec, tile);
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i * 64 + lane] = (uint16_t)m[i];
}
__device__ __forceinline__ void load_masks(const QueryKArgs& a, int dec, int64_t tile, uint32_t m[5], int lane) {
  const uint16_t* s = mask_slot(a, dec, tile);
#pragma unroll
  for (int i = 0; i < 5; ++i) m[i] = s[i * 64 + lane];
}
// The masks of point idx, lane half h, wherever the forward's tiling put them (a live-point tile gathers
// its points from many source tiles): a per-lane tile and lane instead of the wave's.
__device__ __forceinline__ void load_masks_at(const QueryKArgs& a, int dec, int64_t idx, int h, uint32_t m[5]) {
  const uint16_t* s = mask_slot(a, dec, idx >> 5) + ((int)(idx & 31) | (h << 5));
#pragma unroll
  for (int i = 0; i < 5; ++i) m[i] = s[i * 64];
}

// Activation tape of the colour decoder (ABI v9 nslam_query_cfg.act_tape): the forward stores the
// post-ReLU hidden tiles h0..h4 of every tile (C layout) and the weight-gradient backward reads them
// instead of recomputing the decoder (it needs them as the inputs of dW; Mapper.py:503).
constexpr int kTapeFloats = 5 * 16 * 64;  // per tile: h0..h4
// Layout [tile][layer][register r][64 lanes] float: every store / load instruction moves 256 B
// contiguous, and no 4-register grouping of the tile is needed (a float4 layout cost the forward
// ~30 VGPRs of copies).
// Point-major: layer i of a tile is [32 points][32 features], the layout of the weight-gradient
// MFMA's B operand (K = points), so the backward streams it from global memory with no LDS
// transpose.  The forward stores registers 4k..4k+3 of lane (p, h) — features 8k+4h..+3, i.e.
// F(r, h) — as one 16-B store at [p][8k+4h].
__device__ __forceinline__ void tape_store(float* __restrict__ t, int i, const f32x16& v, int lane) {
  const int p = lane & 31, h = lane >> 5;
  __attribute__((address_space(1))) f32x4* q =
      reinterpret_cast<__attribute__((address_space(1))) f32x4*>(as_global_w(t) + i * 1024 + p * 32 + 4 * h);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[2 * k] = f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
}

// ------------------------------------------------------------------------------------------
// MLP with Fourier embedding (decoder.py:177-203): forward
//   layer-3's embedding product is formed right after layer 0, so the 48-register embedding
//   dies early (the MFMA work is unchanged).
// ------------------------------------------------------------------------------------------
// fc_c.i: the feature blocks' share of layer i's input (decoder.py:195-197)
template <int NC>
__device__ __forceinline__ f32x16 fc_branch(const float* __restrict__ pk, const XyzPack& L, int i,
                                            const f32x16 (&cin)[NC], int lane) {
  f32x16 z = vec_tile_g(pk + L.BiasC(i), lane);
#pragma unroll
  for (int c = 0; c < NC; ++c) gemm_acc(z, pk + L.FC(i, c) * NSLAM_FRAG, cin[c], lane);
  return z;
}

// (the decoder's vector section — biases, output rows, Fourier B — is read from global memory here;
// the decoder-parallel forward's chain with an LDS copy of it is xyz_forward_pf, nslam_query_fwd.h)
template <int NC, bool KEEP, bool TAPE = false>
__device__ __forceinline__ f32x16 xyz_forward(const float* __restrict__ pk, const f32x16 (&cin)[NC],
                                              const float x[3], int lane, uint32_t m[5], f32x16* hs,
                                              float* __restrict__ tape = nullptr) {
  const XyzPack L{NC};
  f32x16 a = vec_tile_g(pk + L.Bias(0), lane);
  f32x16 a3 = vec_tile_g(pk + L.Bias(3), lane);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const f32x16 e = emb_tile<false, true>(pk + L.FB(), x, b, lane);
    gemm_acc(a, pk + (L.L0() + b) * NSLAM_FRAG, e, lane);
    gemm_acc(a3, pk + (L.L3() + b) * NSLAM_FRAG, e, lane);
  }
  m[0] = mask16(a);
  f32x16 h = relu16(a) + fc_branch<NC>(pk, L, 0, cin, lane);
  if (KEEP) hs[0] = h;
  if (TAPE) tape_store(tape, 0, h, lane);
  a = vec_tile_g(pk + L.Bias(1), lane);
  gemm_acc(a, pk + L.L1() * NSLAM_FRAG, h, lane);
  m[1] = mask16(a);
  h = relu16(a) + fc_branch<NC>(pk, L, 1, cin, lane);
  if (KEEP) hs[1] = h;
  if (TAPE) tape_store(tape, 1, h, lane);
  a = vec_tile_g(pk + L.Bias(2), lane);
  gemm_acc(a, pk + L.L2() * NSLAM_FRAG, h, lane);
  m[2] = mask16(a);
  h = relu16(a) + fc_branch<NC>(pk, L, 2, cin, lane);
  if (KEEP) hs[2] = h;
  if (TAPE) tape_store(tape, 2, h, lane);
  gemm_acc(a3, pk + (L.L3() + 3) * NSLAM_FRAG, h, lane);
  m[3] = mask16(a3);
  h = relu16(a3) + fc_branch<NC>(pk, L, 3, cin, lane);
  if (KEEP) hs[3] = h;
  if (TAPE) tape_store(tape, 3, h, lane);
  a = vec_tile_g(pk + L.Bias(4), lane);
  gemm_acc(a, pk + L.L4() * NSLAM_FRAG, h, lane);
  m[4] = mask16(a);
  h = relu16(a) + fc_branch<NC>(pk, L, 4, cin, lane);
  if (TAPE) tape_store(tape, 4, h, lane);
  return h;
}

// dh += the caller's cotangent of h4 (ABI v17 nslam_query_cfg.g_h4; row = this lane's point, [32] floats,
// NULL: none): feature F(r, h) of register r = 4i + j is float 8i + 4h + j of the row
__device__ __forceinline__ void add_gh4(f32x16& dh, const float* __restrict__ row, int lane) {
  if (!row) return;
  const gptr_t<f32x4> p = as_global(reinterpret_cast<const f32x4*>(row + 4 * (lane >> 5)));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 v = p[2 * i];
#pragma unroll
    for (int j = 0; j < 4; ++j) dh[4 * i + j] += v[j];
  }
}

// ------------------------------------------------------------------------------------------
// MLP_no_xyz (coarse, decoder.py:262-274): forward
// ------------------------------------------------------------------------------------------
template <bool KEEP>
__device__ __forceinline__ f32x16 noxyz_forward(const float* __restrict__ pk, const f32x16& c, int lane,
                                                uint32_t m[5], f32x16* hs) {
  const NoXyzPack L;
  f32x16 a = vec_tile_g(pk + L.Bias(0), lane);
  gemm_acc(a, pk + L.L0() * NSLAM_FRAG, c, lane);
  f32x16 a3 = vec_tile_g(pk + L.Bias(3), lane);
  gemm_acc(a3, pk + L.L3() * NSLAM_FRAG, c, lane);
  m[0] = mask16(a);
  f32x16 h = relu16(a);
  if (KEEP) hs[0] = h;
  a = vec_tile_g(pk + L.Bias(1), lane);
  gemm_acc(a, pk + L.L1() * NSLAM_FRAG, h, lane);
  m[1] = mask16(a);
  h = relu16(a);
  if (KEEP) hs[1] = h;
  a = vec_tile_g(pk + L.Bias(2), lane);
  gemm_acc(a, pk + L.L2() * NSLAM_FRAG, h, lane);
  m[2] = mask16(a);
  h = relu16(a);
  if (KEEP) hs[2] = h;
  gemm_acc(a3, pk + (L.L3() + 1) * NSLAM_FRAG, h, lane);
  m[3] = mask16(a3);
  h = relu16(a3);
  if (KEEP) hs[3] = h;
  a = vec_tile_g(pk + L.Bias(4), lane);
  gemm_acc(a, pk + L.L4() * NSLAM_FRAG, h, lane);
  m[4] = mask16(a);
  return relu16(a);
}

}  // namespace nslamq
