#pragma once
// nslam_query_fwd.h — the forward kernels of the fused point query: the pipelined gathers, the decoder
// chain with its vector section in LDS (xyz_forward_pf), the per-decoder units, and k_query_fwd (one wave
// runs a tile's whole stage), k_query_fwd_units (the decoder-parallel forward of nslam_query_fwd_ws: one
// wave per decoder and tile, the same values bit for bit) and k_occ_combine.
// Included by nslam_query.hip only (the file map: nslam_query_core.h).
#include "nslam_query_core.h"

namespace nslamq {

// The trilinear cell of a point in one grid, corners formed on demand (make_corners' rows and weights,
// the same arithmetic): 10 values per lane instead of a Corners struct's 8 rows + 8 weights.
struct LazyCell {
  int row0, nx, nxy;
  float f0[3], f1[3];
  bool hi_ok[3];
  __device__ __forceinline__ LazyCell(const nslam_grid& g, const Pt& q) {
    const int n[3] = {g.dims[2], g.dims[1], g.dims[0]};  // x→W, y→H, z→D
    int i0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float gm;
      const float u = unnorm_clip(norm_coord(q.p[a], g.lo[a], g.hi[a]), n[a], gm);
      const float fl = floorf(u);
      i0[a] = (int)fl;
      f1[a] = u - fl;
      f0[a] = (float)(i0[a] + 1) - u;
      hi_ok[a] = (i0[a] + 1) <= n[a] - 1;
    }
    nx = n[0];
    nxy = n[1] * n[0];
    row0 = (i0[2] * n[1] + i0[1]) * n[0] + i0[0];
  }
  // corner k's row (0 when out of range) and weight (exactly 0 when out of range)
  __device__ __forceinline__ int row(int k, float& w) const {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const bool ok = (!dx || hi_ok[0]) && (!dy || hi_ok[1]) && (!dz || hi_ok[2]);
    const float wr = ((dx ? f1[0] : f0[0]) * (dy ? f1[1] : f0[1])) * (dz ? f1[2] : f0[2]);
    w = ok ? wr : 0.f;
    return (row0 + dz * nxy + dy * nx + dx) & -(int)ok;  // (a select, not a branch)
  }
};

// Two trilinear gathers (the fine decoder's fine and middle features, decoder.py:184-187) software-
// pipelined corner by corner: corner k + 1's rows of both grids are loaded while corner k is summed, so
// 16 row loads per lane are in flight and no corner waits for a full round trip after the previous one.
// Each feature sums its corners in gather_tile's order (the same values).
__device__ __forceinline__ void gather_pair(const nslam_grid& gA, const nslam_grid& gB, const Pt& q, int lane,
                                            f32x16& accA, f32x16& accB) {
  const int h = lane >> 5;
  const LazyCell A(gA, q), B(gB, q);
  accA = zero16();
  accB = zero16();
  auto load = [&](const LazyCell& L, const float* data, int k, f32x4 (&v)[4], float& w) {
    const gptr_t<f32x4> rp =
        as_global(reinterpret_cast<const f32x4*>(data + (size_t)(uint32_t)L.row(k, w) * NSLAM_C_DIM + 4 * h));
    v[0] = rp[0];
    v[1] = rp[2];
    v[2] = rp[4];
    v[3] = rp[6];
  };
  f32x4 va[4], vb[4];
  float wa, wb;
  load(A, gA.data, 0, va, wa);
  load(B, gB.data, 0, vb, wb);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f32x4 na[4], nb[4];
    float nwa = 0.f, nwb = 0.f;
    if (k < 7) {
      load(A, gA.data, k + 1, na, nwa);
      load(B, gB.data, k + 1, nb, nwb);
    }
    __builtin_amdgcn_sched_barrier(0);  // the next corner's loads are issued before this one is summed
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      accA[j] += va[0][j] * wa;
      accA[4 + j] += va[1][j] * wa;
      accA[8 + j] += va[2][j] * wa;
      accA[12 + j] += va[3][j] * wa;
      accB[j] += vb[0][j] * wb;
      accB[4 + j] += vb[1][j] * wb;
      accB[8 + j] += vb[2][j] * wb;
      accB[12 + j] += vb[3][j] * wb;
    }
    if (k < 7) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        va[i] = na[i];
        vb[i] = nb[i];
      }
      wa = nwa;
      wb = nwb;
    }
  }
}

// xyz_forward of the decoder-parallel forward (vs: the vector section's LDS copy), its 15 (NC = 1) or 20
// (NC = 2) GEMMs as a FragPipe: each weight fragment is loaded while the previous GEMM runs, so no GEMM
// waits for its fragment's L2 round trip.  The same products in the same order as xyz_forward.
// (phases build: marks MK .. MK + 3 after the embedding GEMMs, layers 1-2, layer 3 and layer 4)
template <int NC, bool TAPE, int MK = 5>
__device__ __forceinline__ f32x16 xyz_forward_pf(const float* __restrict__ pk, const f32x16 (&cin)[NC],
                                                 const float x[3], int lane, uint32_t m[5],
                                                 float* __restrict__ tape, const float* vs) {
  const XyzPack L{NC};
  FragPipe fp(pk, L.L0(), lane);
  f32x16 a = vec_tile(vs + (L.Bias(0) - L.V()), lane);
  f32x16 a3 = vec_tile(vs + (L.Bias(3) - L.V()), lane);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const f32x16 e = emb_tile<false, false>(vs + (L.FB() - L.V()), x, b, lane);
    fp.gemm(a, e, L.L3() + b);
    fp.gemm(a3, e, b < 2 ? L.L0() + b + 1 : L.FC(0, 0));
  }
  PHASE(0, MK);
  // fc_c.i (cin) with the next layer's first fragment after it
  auto fc = [&](int i, int next) {
    f32x16 z = vec_tile(vs + (L.BiasC(i) - L.V()), lane);
#pragma unroll
    for (int c = 0; c < NC; ++c) fp.gemm(z, cin[c], c + 1 < NC ? L.FC(i, c + 1) : next);
    return z;
  };
  m[0] = mask16(a);
  f32x16 h = relu16(a) + fc(0, L.L1());
  if (TAPE) tape_store(tape, 0, h, lane);
  a = vec_tile(vs + (L.Bias(1) - L.V()), lane);
  fp.gemm(a, h, L.FC(1, 0));
  m[1] = mask16(a);
  h = relu16(a) + fc(1, L.L2());
  if (TAPE) tape_store(tape, 1, h, lane);
  a = vec_tile(vs + (L.Bias(2) - L.V()), lane);
  fp.gemm(a, h, L.FC(2, 0));
  m[2] = mask16(a);
  h = relu16(a) + fc(2, L.L3() + 3);
  if (TAPE) tape_store(tape, 2, h, lane);
  PHASE(0, MK + 1);
  fp.gemm(a3, h, L.FC(3, 0));
  m[3] = mask16(a3);
  h = relu16(a3) + fc(3, L.L4());
  if (TAPE) tape_store(tape, 3, h, lane);
  PHASE(0, MK + 2);
  a = vec_tile(vs + (L.Bias(4) - L.V()), lane);
  fp.gemm(a, h, L.FC(4, 0));
  m[4] = mask16(a);
  h = relu16(a) + fc(4, -1);
  if (TAPE) tape_store(tape, 4, h, lane);
  PHASE(0, MK + 3);
  return h;
}

// output_linear row j: sum_f Wo[j][f] h4[f] + bo[j]  (complete in both halves)
__device__ __forceinline__ float out_row(const float* __restrict__ Wo, const float* __restrict__ bo, int j,
                                         const f32x16& h4, int lane) {
  const f32x16 w = vec_tile(Wo + 32 * j, lane);
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += w[r] * h4[r];
  return (s + xor32(s)) + bo[j];
}

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
template <int STAGE>
__global__ __launch_bounds__(256, 2) void k_query_fwd(QueryKArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave_id();
  if (tile * 32 >= a.n) return;  // wave-uniform
  const int h = lane >> 5;
  const Pt q = load_point(a, tile * 32 + (lane & 31));
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t m[5];
  if (STAGE == NSLAM_STAGE_COARSE) {
    Corners cr;
    grid_corners(cr, a.c.grid[NSLAM_DEC_COARSE], q);
    const f32x16 c = gather_tile(a.c.grid[NSLAM_DEC_COARSE].data, cr, lane);
    const float* pk = a.c.packed[NSLAM_DEC_COARSE];
    const NoXyzPack L;
    const f32x16 h4 = noxyz_forward<false>(pk, c, lane, m, nullptr);
    save_masks(a, NSLAM_DEC_COARSE, tile, m, lane);
    out[3] = out_row(pk + L.Wo(), pk + L.Bo(), 0, h4, lane);
  } else {
    Corners cr;
    grid_corners(cr, a.c.grid[NSLAM_DEC_MIDDLE], q);
    const f32x16 cm[1] = {gather_tile(a.c.grid[NSLAM_DEC_MIDDLE].data, cr, lane)};
    {
      const float* pk = a.c.packed[NSLAM_DEC_MIDDLE];
      const XyzPack L{1};
      const f32x16 h4 = xyz_forward<1, false>(pk, cm, q.x, lane, m, nullptr);
      save_masks(a, NSLAM_DEC_MIDDLE, tile, m, lane);
      out[3] = out_row(pk + L.Wo(), pk + L.Bo(), 0, h4, lane);
    }
    if (STAGE >= NSLAM_STAGE_FINE) {
      grid_corners(cr, a.c.grid[NSLAM_DEC_FINE], q);
      const f32x16 cf[2] = {gather_tile(a.c.grid[NSLAM_DEC_FINE].data, cr, lane), cm[0]};
      const float* pk = a.c.packed[NSLAM_DEC_FINE];
      const XyzPack L{2};
      const f32x16 h4 = xyz_forward<2, false>(pk, cf, q.x, lane, m, nullptr);
      save_masks(a, NSLAM_DEC_FINE, tile, m, lane);
      out[3] = out_row(pk + L.Wo(), pk + L.Bo(), 0, h4, lane) + out[3];  // fine_occ + middle_occ
    }
    if (STAGE == NSLAM_STAGE_COLOR) {
      grid_corners(cr, a.c.grid[NSLAM_DEC_COLOR], q);
      const f32x16 cc[1] = {gather_tile(a.c.grid[NSLAM_DEC_COLOR].data, cr, lane)};
      const float* pk = a.c.packed[NSLAM_DEC_COLOR];
      const XyzPack L{1};
      f32x16 h4;
      if (a.c.act_tape)
        h4 = xyz_forward<1, false, true>(pk, cc, q.x, lane, m, nullptr, a.c.act_tape + tile * kTapeFloats);
      else
        h4 = xyz_forward<1, false>(pk, cc, q.x, lane, m, nullptr);
      save_masks(a, NSLAM_DEC_COLOR, tile, m, lane);
#pragma unroll
      for (int j = 0; j < 3; ++j) out[j] = out_row(pk + L.Wo(), pk + L.Bo(), j, h4, lane);
    }
  }
  if (!q.inside) out[3] = 100.f;  // Renderer.py:57
  if (h == 0 && q.valid) {
    f32x4 v;
    v[0] = out[0];
    v[1] = out[1];
    v[2] = out[2];
    v[3] = out[3];
    *reinterpret_cast<f32x4*>(a.raw + (tile * 32 + (lane & 31)) * 4) = v;
  }
}

// One decoder of the decoder-parallel forward for this wave's tile (vec: the decoder's vector section in
// LDS): gather, chain, masks and the decoder's share of the output.
__device__ __forceinline__ void fwd_part_middle(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx, int lane,
                                                float* __restrict__ occ_mid, const float* vec) {
  const int h = lane >> 5;
  uint32_t m[5];
  Corners cr;
  grid_corners(cr, a.c.grid[NSLAM_DEC_MIDDLE], q);
  PHASE(0, 2);
  const f32x16 cm[1] = {gather_tile(a.c.grid[NSLAM_DEC_MIDDLE].data, cr, lane)};
  PHASE(0, 3);
  const float* pk = a.c.packed[NSLAM_DEC_MIDDLE];
  const XyzPack L{1};
  const f32x16 h4 = xyz_forward_pf<1, false>(pk, cm, q.x, lane, m, nullptr, vec);
  save_masks(a, NSLAM_DEC_MIDDLE, tile, m, lane);
  float o = out_row(vec + (L.Wo() - L.V()), vec + (L.Bo() - L.V()), 0, h4, lane);
  if (!q.inside) o = 100.f;
  if (h == 0 && q.valid) occ_mid[idx] = o;
}

template <int STAGE>
__device__ __forceinline__ void fwd_part_fine(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx, int lane,
                                              const float* vec) {
  // the fine decoder also reads the middle feature (decoder.py:184-187)
  const int h = lane >> 5;
  uint32_t m[5];
  PHASE(0, 2);
  f32x16 cf[2];
  gather_pair(a.c.grid[NSLAM_DEC_FINE], a.c.grid[NSLAM_DEC_MIDDLE], q, lane, cf[0], cf[1]);
  PHASE(0, 3);
  const float* pk = a.c.packed[NSLAM_DEC_FINE];
  const XyzPack L{2};
  const f32x16 h4 = xyz_forward_pf<2, false>(pk, cf, q.x, lane, m, nullptr, vec);
  save_masks(a, NSLAM_DEC_FINE, tile, m, lane);
  float o = out_row(vec + (L.Wo() - L.V()), vec + (L.Bo() - L.V()), 0, h4, lane);
  if (!q.inside) o = 0.f;
  if (h == 0 && q.valid) {
    if (STAGE == NSLAM_STAGE_COLOR) {
      a.raw[idx * 4 + 3] = o;
    } else {
      f32x4 v = {0.f, 0.f, 0.f, o};
      *reinterpret_cast<f32x4*>(a.raw + idx * 4) = v;
    }
  }
}

// the colour decoder (TAPE: its hidden activations go to the activation tape as well)
template <bool TAPE>
__device__ __forceinline__ void fwd_part_color(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx, int lane,
                                               const float* vec) {
  const int h = lane >> 5;
  uint32_t m[5];
  Corners cr;
  grid_corners(cr, a.c.grid[NSLAM_DEC_COLOR], q);
  PHASE(0, 10);
  const f32x16 cc[1] = {gather_tile(a.c.grid[NSLAM_DEC_COLOR].data, cr, lane)};
  PHASE(0, 11);
  const float* pk = a.c.packed[NSLAM_DEC_COLOR];
  const XyzPack L{1};
  float* tp = TAPE ? a.c.act_tape + tile * kTapeFloats : nullptr;
  const f32x16 h4 = xyz_forward_pf<1, TAPE, 12>(pk, cc, q.x, lane, m, tp, vec);
  save_masks(a, NSLAM_DEC_COLOR, tile, m, lane);
  float o[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) o[j] = out_row(vec + (L.Wo() - L.V()), vec + (L.Bo() - L.V()), j, h4, lane);
  if (h == 0 && q.valid) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.raw[idx * 4 + j] = o[j];
  }
}

// Decoder-parallel forward (fine and colour stages), one wave per workgroup: unit u = blockIdx is one
// decoder of one 32-point tile — [0, T) fine (two gathers, 20 GEMMs: the heaviest, dispatched first),
// [T, 2T) middle, [2T, 3T) colour — so a launch has 2-3x the waves of k_query_fwd and every wave a
// fraction of its serial MFMA / gather chain.  With one-wave workgroups the dispatcher refills every
// wave slot the moment its wave exits, so the launch balances itself over the SIMDs
// (tools/probes/wave_timeline.py, profiles/r05_*).  Each decoder writes its share:
//   middle: occ_mid[p] = inside ? middle_occ : 100
//   fine:   raw[p][3]  = inside ? fine_occ : 0     (fine stage: the whole row)
//   colour: raw[p][0..2]
// and k_occ_combine (or the loss kernel, defer_occ) then forms raw[p][3] = fine_occ + middle_occ
// (decoder.py:331-334, the reference's operand order) — exactly 100 outside the bound (0 + 100;
// Renderer.py:57).
// (The staging loop of the vector section and the part -> decoder dispatch are written out in the kernel:
// behind __forceinline__ helpers the compiler allocates it 168 VGPRs instead of 160 and schedules it
// differently, profiles/query_split_resources.txt.)
#ifndef NSLAM_UNITS_LB
#define NSLAM_UNITS_LB 3  // waves per SIMD the units kernel's register budget allows (4: <= 128 VGPRs)
#endif
constexpr int kVecFloats = 744;  // XyzPack vector section (740) rounded to float4s
template <int STAGE, bool TAPE>
__global__ __launch_bounds__(64, NSLAM_UNITS_LB) void k_query_fwd_units(QueryKArgs a, float* __restrict__ occ_mid) {
  const int64_t ntiles = (a.n + 31) / 32;
  const int64_t u = blockIdx.x;
  const int j = u < ntiles ? 0 : u < 2 * ntiles ? 1 : 2;  // dispatch slot
  const int part = j == 0 ? 1 : (j == 1 ? 0 : 2);
  const int64_t tile = u - j * ntiles;
  TL(0, 0, part);
  // this unit's decoder vector section (biases, output rows, Fourier B), read by every layer
  __shared__ __attribute__((aligned(16))) float vsec[kVecFloats];
  {
    const int d = part == 0 ? NSLAM_DEC_MIDDLE : part == 1 ? NSLAM_DEC_FINE : NSLAM_DEC_COLOR;
    const float* src = a.c.packed[d] + XyzPack{d == NSLAM_DEC_FINE ? 2 : 1}.V();
    for (int i = threadIdx.x; i < 740; i += 64) vsec[i] = src[i];
    __syncthreads();
  }
  const int lane = threadIdx.x;
  const int64_t idx = tile * 32 + (lane & 31);
  const Pt q = load_point(a, idx);
  if (part == 1) {
    fwd_part_fine<STAGE>(a, q, tile, idx, lane, vsec);
  } else if (part == 0) {
    fwd_part_middle(a, q, tile, idx, lane, occ_mid, vsec);
  } else if (STAGE == NSLAM_STAGE_COLOR) {
    fwd_part_color<TAPE>(a, q, tile, idx, lane, vsec);
  }
  TL(0, 1, 0);
}

static __global__ __launch_bounds__(256) void k_occ_combine(float* __restrict__ raw, const float* __restrict__ occ_mid,
                                                     int64_t n) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n) raw[p * 4 + 3] = raw[p * 4 + 3] + occ_mid[p];
}

}  // namespace nslamq
