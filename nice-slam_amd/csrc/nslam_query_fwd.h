#pragma once
// nslam_query_fwd.h — the forward kernels of the fused point query: the pipelined gathers, the decoder
// chain with its vector section in LDS (xyz_forward_pf), the per-decoder units, and k_query_fwd (one wave
// runs a tile's whole stage), k_query_fwd_parts / k_query_fwd_units / k_query_fwd_pc (the decoder-parallel
// forwards of nslam_query_fwd_ws: ABI v18 fwd_variant, bit-identical) and k_occ_combine.
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

// gather_tile's trilinear feature with all 8 corners' row loads issued together (one round trip of memory
// latency instead of a corner-by-corner pipeline's 8), summed in gather_tile's corner order (the same
// values).  For a wave with nothing else in registers (the producer of k_query_fwd_pc).
__device__ __forceinline__ f32x16 gather_wide(const nslam_grid& g, const Pt& q, int lane) {
  const int h = lane >> 5;
  const LazyCell A(g, q);
  f32x16 acc = zero16();
  f32x4 v[8][4];
  float w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const gptr_t<f32x4> rp =
        as_global(reinterpret_cast<const f32x4*>(g.data + (size_t)(uint32_t)A.row(k, w[k]) * NSLAM_C_DIM + 4 * h));
    v[k][0] = rp[0];
    v[k][1] = rp[2];
    v[k][2] = rp[4];
    v[k][3] = rp[6];
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] += v[k][0][j] * w[k];
      acc[4 + j] += v[k][1][j] * w[k];
      acc[8 + j] += v[k][2][j] * w[k];
      acc[12 + j] += v[k][3][j] * w[k];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  return acc;
}

// xyz_forward of the decoder-parallel forward (vs: the vector section's LDS copy), its 15 (NC = 1) or 20
// (NC = 2) GEMMs as a FragPipe: each weight fragment is loaded while the previous GEMM runs, so no GEMM
// waits for its fragment's L2 round trip.  The same products in the same order as xyz_forward.
// (phases build: marks MK .. MK + 3 after the embedding GEMMs, layers 1-2, layer 3 and layer 4)
// (E(b): embedding block b — sin(x B_b) formed here, or handed over by a producer wave, k_query_fwd_pc)
template <int NC, bool TAPE, int MK = 5, class EmbFn>
__device__ __forceinline__ f32x16 xyz_forward_pf_e(const float* __restrict__ pk, const f32x16 (&cin)[NC],
                                                   const EmbFn& E, int lane, uint32_t m[5],
                                                   float* __restrict__ tape, const float* vs) {
  const XyzPack L{NC};
  FragPipe fp(pk, L.L0(), lane);
  f32x16 a = vec_tile(vs + (L.Bias(0) - L.V()), lane);
  f32x16 a3 = vec_tile(vs + (L.Bias(3) - L.V()), lane);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const f32x16 e = E(b);
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
template <int NC, bool TAPE, int MK = 5>
__device__ __forceinline__ f32x16 xyz_forward_pf(const float* __restrict__ pk, const f32x16 (&cin)[NC],
                                                 const float x[3], int lane, uint32_t m[5],
                                                 float* __restrict__ tape, const float* vs) {
  const XyzPack L{NC};
  return xyz_forward_pf_e<NC, TAPE, MK>(
      pk, cin, [&](int b) { return emb_tile<false, false>(vs + (L.FB() - L.V()), x, b, lane); }, lane, m, tape, vs);
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

// One decoder of the decoder-parallel forward for this wave's tile.
// the middle decoder's chain and output for this wave's tile from its gathered feature cm
__device__ __forceinline__ void fwd_middle_chain(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx,
                                                 int lane, float* __restrict__ occ_mid, const float* vec,
                                                 const f32x16& cm) {
  const int h = lane >> 5;
  uint32_t m[5];
  const float* pk = a.c.packed[NSLAM_DEC_MIDDLE];
  const XyzPack L{1};
  const f32x16 cms[1] = {cm};
  const f32x16 h4 = xyz_forward_pf<1, false>(pk, cms, q.x, lane, m, nullptr, vec);
  save_masks(a, NSLAM_DEC_MIDDLE, tile, m, lane);
  float o = out_row(vec + (L.Wo() - L.V()), vec + (L.Bo() - L.V()), 0, h4, lane);
  if (!q.inside) o = 100.f;
  if (h == 0 && q.valid) occ_mid[idx] = o;
}
__device__ __forceinline__ void fwd_part_middle(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx, int lane,
                                                float* __restrict__ occ_mid, const float* vec) {
  Corners cr;
  grid_corners(cr, a.c.grid[NSLAM_DEC_MIDDLE], q);
  PHASE(0, 2);
  const f32x16 cm = gather_tile(a.c.grid[NSLAM_DEC_MIDDLE].data, cr, lane);
  PHASE(0, 3);
  fwd_middle_chain(a, q, tile, idx, lane, occ_mid, vec, cm);
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

// the colour decoder's chain (+ activation tape) and outputs for this wave's tile from its feature cc
template <bool TAPE>
__device__ __forceinline__ void fwd_color_chain(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx,
                                                int lane, const float* vec, const f32x16& cc) {
  const int h = lane >> 5;
  uint32_t m[5];
  const float* pk = a.c.packed[NSLAM_DEC_COLOR];
  const XyzPack L{1};
  float* tp = TAPE ? a.c.act_tape + tile * kTapeFloats : nullptr;
  const f32x16 ccs[1] = {cc};
  const f32x16 h4 = xyz_forward_pf<1, TAPE, 12>(pk, ccs, q.x, lane, m, tp, vec);
  save_masks(a, NSLAM_DEC_COLOR, tile, m, lane);
  float o[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) o[j] = out_row(vec + (L.Wo() - L.V()), vec + (L.Bo() - L.V()), j, h4, lane);
  if (h == 0 && q.valid) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.raw[idx * 4 + j] = o[j];
  }
}
template <bool TAPE>
__device__ __forceinline__ void fwd_part_color(const QueryKArgs& a, const Pt& q, int64_t tile, int64_t idx, int lane,
                                               const float* vec) {
  Corners cr;
  grid_corners(cr, a.c.grid[NSLAM_DEC_COLOR], q);
  PHASE(0, 10);
  const f32x16 cc = gather_tile(a.c.grid[NSLAM_DEC_COLOR].data, cr, lane);
  PHASE(0, 11);
  fwd_color_chain<TAPE>(a, q, tile, idx, lane, vec, cc);
}

// Decoder-parallel forward (fine and colour stages): each workgroup evaluates ONE part for its 4
// tiles, so a launch has 2-3x the waves of k_query_fwd and every wave a fraction of the serial
// MFMA/gather chain.  Parts are interleaved over blockIdx (heavy and light workgroups mix on
// every CU).  NPARTS = 3 (colour stage): middle | fine | colour; NPARTS = 2: fine stage middle |
// fine, or colour stage (middle then colour) | fine — fewer, balanced waves (3000 at room0) that
// fit the chip's wave slots in one round.
//   middle: occ_mid[p] = inside ? middle_occ : 100
//   fine:   raw[p][3]  = inside ? fine_occ : 0     (fine stage: the whole row)
//   colour: raw[p][0..2]
// and k_occ_combine (or the loss kernel, defer_occ) then forms raw[p][3] = fine_occ + middle_occ
// (decoder.py:331-334, the reference's operand order) — exactly 100 outside the bound (0 + 100;
// Renderer.py:57).
// (The staging loop of the vector section and the part -> decoder dispatch are written out in each of
// the parts, units and pc kernels: behind shared __forceinline__ helpers the compiler allocates
// k_query_fwd_units 168 VGPRs instead of 160 and schedules it differently.)
#ifndef NSLAM_FWD_LB
#define NSLAM_FWD_LB 2  // min waves per SIMD (experiments: 3..5 trade VGPRs for occupancy)
#endif
constexpr int kVecFloats = 744;  // XyzPack vector section (740) rounded to float4s
template <int STAGE, int NPARTS, bool TAPE>
__global__ __launch_bounds__(256, NSLAM_FWD_LB) void k_query_fwd_parts(QueryKArgs a, float* __restrict__ occ_mid) {
  const int part = (int)(blockIdx.x % NPARTS);
  const int lane = threadIdx.x & 63;
  TL(0, 0, part);
  // The part's decoder vector sections (biases, output rows, Fourier B: ~3 KiB each) are read by
  // every layer of every wave: an LDS copy per workgroup turns ~90 global loads per wave into
  // ds_reads.  Part 0 of the 2-part colour forward evaluates middle then colour: two copies.
  __shared__ __attribute__((aligned(16))) float vsec[2][kVecFloats];
  {
    const int d0 = part == 0 ? NSLAM_DEC_MIDDLE : part == 1 ? NSLAM_DEC_FINE : NSLAM_DEC_COLOR;
    const int nc0 = d0 == NSLAM_DEC_FINE ? 2 : 1;
    const float* src0 = a.c.packed[d0] + XyzPack{nc0}.V();
    const bool two = NPARTS == 2 && STAGE == NSLAM_STAGE_COLOR && part == 0;
    const float* src1 = two ? a.c.packed[NSLAM_DEC_COLOR] + XyzPack{1}.V() : nullptr;
    for (int i = threadIdx.x; i < 740; i += 256) {
      vsec[0][i] = src0[i];
      if (two) vsec[1][i] = src1[i];
    }
    __syncthreads();
  }
  const int64_t tile = (int64_t)(blockIdx.x / NPARTS) * 4 + wave_id();
  if (tile * 32 >= a.n) return;  // wave-uniform
  const int64_t idx = tile * 32 + (lane & 31);
  PHASE(0, 0);
  const Pt q = load_point(a, idx);
  PHASE(0, 1);
  if (NPARTS == 2 && STAGE == NSLAM_STAGE_COLOR) {
    if (part == 0) {
      fwd_part_middle(a, q, tile, idx, lane, occ_mid, vsec[0]);
      fwd_part_color<TAPE>(a, q, tile, idx, lane, vsec[1]);
    } else {
      fwd_part_fine<STAGE>(a, q, tile, idx, lane, vsec[0]);
    }
  } else if (part == 0) {
    fwd_part_middle(a, q, tile, idx, lane, occ_mid, vsec[0]);
  } else if (part == 1) {
    fwd_part_fine<STAGE>(a, q, tile, idx, lane, vsec[0]);
  } else if (STAGE == NSLAM_STAGE_COLOR) {
    fwd_part_color<TAPE>(a, q, tile, idx, lane, vsec[0]);
  }
  PHASE(0, 9);
  TL(0, 1, 0);
}

// Decoder-parallel forward, one wave per workgroup: unit u = blockIdx is one decoder of one 32-point
// tile — [0, T) fine (two gathers, 20 GEMMs: the heaviest, dispatched first), [T, 2T) middle, [2T, 3T)
// colour — with the same per-decoder code and outputs as k_query_fwd_parts.  With one-wave workgroups
// the dispatcher refills every wave slot the moment its wave exits, so the launch balances itself over
// the SIMDs (k_query_fwd_parts' 4-wave workgroups of middle-then-colour waves left the SIMDs that drew
// two of them running ~25 us after the others: tools/probes/wave_timeline.py, profiles/r05_*).
#ifndef NSLAM_UNITS_LB
#define NSLAM_UNITS_LB 3  // waves per SIMD the units kernel's register budget allows (4: <= 128 VGPRs)
#endif
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

// ------------------------------------------------------------------------------------------
// Producer / consumer forward (round 5): the decoder-tile units of k_query_fwd_units, but each unit's
// work split between two kinds of wave of one persistent workgroup per CU, so every SIMD holds both at
// once and its MFMA pipe (consumers) and VALU / memory pipes (producers) run side by side:
//   producer waves (4, one per SIMD): the unit's points, trilinear gathers (gather_wide)
//     and Fourier embedding sin(x B_b) — exactly the units kernel's arithmetic — into an LDS slot, in
//     the register layout (16 floats per lane per tile: one conflict-free ds_write_b128 per quad);
//   consumer waves (8, two per SIMD): read a full slot into registers (3 embedding tiles + NC feature
//     tiles), hand the slot back at once, then run the decoder's GEMM chain (xyz_forward_pf_e: the same
//     products in the same order), masks, activation tape and outputs.
// Slots form a ring of kPcSlots: position k (the CU's k-th unit) lives in slot k % kPcSlots; its
// producer waits until position k - kPcSlots was read (pc_free), fills the slot and publishes k
// (pc_full); its consumer waits for k, reads, releases.  Producers and consumers take positions from
// two LDS counters in order, so the CU's waves balance among themselves; CU g owns the global units
// g, g + G, g + 2G, ... (fine units first: the heaviest).  Every wave leaves when the counter passes
// the CU's unit count, and every position below it is produced and consumed exactly once, so the
// grid drains.  Flags are LDS words written after an explicit lgkmcnt(0) (the slot's data is in LDS
// before the flag is) and polled with s_sleep.
constexpr int kPcCons = 8, kPcProd = 4, kPcWaves = kPcCons + kPcProd;  // consumers: 2 per SIMD
constexpr int kPcSlots = 7;
constexpr int kPcTileF = 1024;                   // one register tile: 16 floats x 64 lanes
constexpr int kPcSlotF = 5 * kPcTileF + 4;       // emb 0-2, features 3-4, header {unit, inside lo, hi}
static_assert((kPcSlotF * 4) % 16 == 0, "slots stay 16-B aligned");

__device__ __forceinline__ void pc_put(float* __restrict__ t, const f32x16& v, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<f32x4*>(t + i * 256 + lane * 4) = f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
}
__device__ __forceinline__ f32x16 pc_get(const float* __restrict__ t, int lane) {
  f32x16 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(t + i * 256 + lane * 4);
    v[4 * i] = q[0];
    v[4 * i + 1] = q[1];
    v[4 * i + 2] = q[2];
    v[4 * i + 3] = q[3];
  }
  return v;
}
// LDS flag words (workgroup-visible): a store after every earlier LDS access of this wave has completed;
// a poll whose value orders every later LDS access of this wave after it
__device__ __forceinline__ void pc_flag_store(int* p, int v) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (bounded: a wait that never ends — a broken invariant; one unit's hand-over takes microseconds — traps
// after ~2^24 polls (~0.5 s) instead of letting the wave go on with a slot it does not own: the launch
// fails loudly, the caller's next HIP call reports the error, and nothing is silently corrupted)
__device__ __forceinline__ void pc_flag_wait(const int* p, int v) {
  [[maybe_unused]] const unsigned long long t0 = TL_NOW();
  for (int it = 0;; ++it) {
    const int x = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (x == v) break;
    if (it == (1 << 24)) __builtin_trap();
    __builtin_amdgcn_s_sleep(1);
  }
  TL_ADD(0, TL_NOW() - t0);  // (timeline build: the wave's waiting time)
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ int pc_take(int* ctr, int lane) {
  int k = 0;
  if (lane == 0) k = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return __builtin_amdgcn_readfirstlane(k);
}

// The producer's share of unit (part, tile) into slot sl: features (part 1: fine and middle), the
// embedding of the part's decoder and the inside ballot — the units kernel's arithmetic
template <int STAGE>
__device__ __forceinline__ void pc_produce(const QueryKArgs& a, int part, int64_t tile, int64_t unit, int lane,
                                           const float* vs, float* __restrict__ sl, int* full, int* freed, int k,
                                           int s) {
  const int64_t idx = tile * 32 + (lane & 31);
  const Pt q = load_point(a, idx);
  // the grids by opaque indices: their constants (extents, scales; float64) are formed per unit —
  // hoisted out of the producer loop they would pin (and spill) registers for all of it
  int gi = part == 1 ? NSLAM_DEC_FINE : part == 0 ? NSLAM_DEC_MIDDLE : NSLAM_DEC_COLOR, gm = NSLAM_DEC_MIDDLE;
  asm volatile("" : "+s"(gi), "+s"(gm));
  // the slot first (position k - kPcSlots has been read out of it); then every tile is stored as soon as
  // it is formed — the features, then the embedding blocks one at a time — so at most one tile and the
  // loads of one gather are in registers
  pc_flag_wait(freed + s, k - kPcSlots);
  [[maybe_unused]] const unsigned long long tg0 = TL_NOW();
  pc_put(sl + 3 * kPcTileF, gather_wide(a.c.grid[gi], q, lane), lane);
  if (part == 1) {
    __builtin_amdgcn_sched_barrier(0);
    pc_put(sl + 4 * kPcTileF, gather_wide(a.c.grid[gm], q, lane), lane);
  }
  TL_ADD1(0, TL_NOW() - tg0);  // (timeline build: the producer's gather time)
  const uint64_t in = __ballot(q.inside);
  const float* B = vs + (XyzPack{1}.FB() - XyzPack{1}.V());  // (the same offset for NC = 2)
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    __builtin_amdgcn_sched_barrier(0);
    pc_put(sl + b * kPcTileF, emb_tile<false, false>(B, q.x, b, lane), lane);
  }
  if (lane == 0) {
    int* hd = reinterpret_cast<int*>(sl + 5 * kPcTileF);
    hd[0] = (int)unit;
    hd[1] = (int)(uint32_t)in;
    hd[2] = (int)(uint32_t)(in >> 32);
  }
  pc_flag_store(full + s, k);
}

template <int STAGE, bool TAPE>
__global__ __launch_bounds__(64 * kPcWaves, 1) void k_query_fwd_pc(QueryKArgs a, float* __restrict__ occ_mid) {
  constexpr int NP = STAGE == NSLAM_STAGE_COLOR ? 3 : 2;
  __shared__ __attribute__((aligned(16))) float vsec[3][kVecFloats];
  __shared__ __attribute__((aligned(16))) float slots[kPcSlots * kPcSlotF];
  __shared__ int full[kPcSlots], freed[kPcSlots], ctr[2];
  {
    const float* s0 = a.c.packed[NSLAM_DEC_MIDDLE] + XyzPack{1}.V();
    const float* s1 = a.c.packed[NSLAM_DEC_FINE] + XyzPack{2}.V();
    const float* s2 = NP == 3 ? a.c.packed[NSLAM_DEC_COLOR] + XyzPack{1}.V() : nullptr;
    for (int i = threadIdx.x; i < 740; i += 64 * kPcWaves) {
      vsec[0][i] = s0[i];
      vsec[1][i] = s1[i];
      if (NP == 3) vsec[2][i] = s2[i];
    }
    if (threadIdx.x < kPcSlots) {
      full[threadIdx.x] = -1;
      freed[threadIdx.x] = (int)threadIdx.x - kPcSlots;
    }
    if (threadIdx.x < 2) ctr[threadIdx.x] = 0;
    __syncthreads();
  }
  const int64_t ntiles = (a.n + 31) / 32;
  const int64_t U = ntiles * NP, G = gridDim.x, g = blockIdx.x;
  const int K = (int)((U - g + G - 1) / G);  // this CU's units (the launch has G <= U)
  const int w = wave_id(), lane0 = threadIdx.x & 63;
  TL(0, 0, w >= kPcCons);
  if (w >= kPcCons) {  // producer
    for (;;) {
      const int k = pc_take(&ctr[0], lane0);
      if (k >= K) break;  // wave-uniform
      // lane-derived addresses re-formed per unit (no hoisting)
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      const int64_t u = g + (int64_t)k * G;
      const int part = u < ntiles ? 1 : u < 2 * ntiles ? 0 : 2;
      const int64_t tile = u - (part == 1 ? 0 : part == 0 ? ntiles : 2 * ntiles);
      const int s = k % kPcSlots;
      pc_produce<STAGE>(a, part, tile, u, lane, vsec[part == 0 ? 0 : part == 1 ? 1 : 2], slots + s * kPcSlotF,
                        full, freed, k, s);
    }
  } else {  // consumer
    for (;;) {
      const int k = pc_take(&ctr[1], lane0);
      if (k >= K) break;  // wave-uniform
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      const int s = k % kPcSlots;
      const float* sl = slots + s * kPcSlotF;
      pc_flag_wait(full + s, k);
      const int* hd = reinterpret_cast<const int*>(sl + 5 * kPcTileF);
      const int64_t u = __builtin_amdgcn_readfirstlane(hd[0]);
      const uint32_t inw = (uint32_t)hd[1 + (lane >> 5)];
      const bool inside = (inw >> (lane & 31)) & 1u;
      const int part = u < ntiles ? 1 : u < 2 * ntiles ? 0 : 2;
      const int64_t tile = u - (part == 1 ? 0 : part == 0 ? ntiles : 2 * ntiles);
      const int64_t idx = tile * 32 + (lane & 31);
      const bool valid = idx < a.n;
      const int h = lane >> 5;
      // the embedding tiles are read where the chain uses them (one at a time in registers); the slot is
      // handed back once the last one is in registers (the features are read into registers first)
      const auto E = [&](int b) {
        const f32x16 v = pc_get(sl + b * kPcTileF, lane);
        if (b == 2) pc_flag_store(freed + s, k);
        return v;
      };
      uint32_t m[5];
      if (part == 1) {
        const f32x16 cf[2] = {pc_get(sl + 3 * kPcTileF, lane), pc_get(sl + 4 * kPcTileF, lane)};
        const XyzPack L{2};
        const float* vs = vsec[1];
        const f32x16 h4 = xyz_forward_pf_e<2, false, 5>(a.c.packed[NSLAM_DEC_FINE], cf, E, lane, m, nullptr, vs);
        save_masks(a, NSLAM_DEC_FINE, tile, m, lane);
        float o = out_row(vs + (L.Wo() - L.V()), vs + (L.Bo() - L.V()), 0, h4, lane);
        if (!inside) o = 0.f;
        if (h == 0 && valid) {
          if (STAGE == NSLAM_STAGE_COLOR) {
            a.raw[idx * 4 + 3] = o;
          } else {
            f32x4 v = {0.f, 0.f, 0.f, o};
            *reinterpret_cast<f32x4*>(a.raw + idx * 4) = v;
          }
        }
      } else if (part == 0) {
        const f32x16 cm[1] = {pc_get(sl + 3 * kPcTileF, lane)};
        const XyzPack L{1};
        const float* vs = vsec[0];
        const f32x16 h4 = xyz_forward_pf_e<1, false, 5>(a.c.packed[NSLAM_DEC_MIDDLE], cm, E, lane, m, nullptr, vs);
        save_masks(a, NSLAM_DEC_MIDDLE, tile, m, lane);
        float o = out_row(vs + (L.Wo() - L.V()), vs + (L.Bo() - L.V()), 0, h4, lane);
        if (!inside) o = 100.f;
        if (h == 0 && valid) occ_mid[idx] = o;
      } else if (STAGE == NSLAM_STAGE_COLOR) {
        const f32x16 cc[1] = {pc_get(sl + 3 * kPcTileF, lane)};
        const XyzPack L{1};
        const float* vs = vsec[2];
        float* tp = TAPE ? a.c.act_tape + tile * kTapeFloats : nullptr;
        const f32x16 h4 = xyz_forward_pf_e<1, TAPE, 12>(a.c.packed[NSLAM_DEC_COLOR], cc, E, lane, m, tp, vs);
        save_masks(a, NSLAM_DEC_COLOR, tile, m, lane);
        float o[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = out_row(vs + (L.Wo() - L.V()), vs + (L.Bo() - L.V()), j, h4, lane);
        if (h == 0 && valid) {
#pragma unroll
          for (int j = 0; j < 3; ++j) a.raw[idx * 4 + j] = o[j];
        }
      }
    }
  }
  TL(0, 1, 0);
}

static __global__ __launch_bounds__(256) void k_occ_combine(float* __restrict__ raw, const float* __restrict__ occ_mid,
                                                     int64_t n) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n) raw[p * 4 + 3] = raw[p * 4 + 3] + occ_mid[p];
}

}  // namespace nslamq
