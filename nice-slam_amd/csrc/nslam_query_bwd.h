#pragma once
// nslam_query_bwd.h — the backward of the fused point query: parameter-gradient slabs and the LDS
// transposes of the weight gradients, the decoders' backward chains (xyz_backward / noxyz_backward
// after a recompute, *_saved from the forward's ReLU masks), one tile's backward (dec_bwd_tile), the
// kernels k_dec_bwd (one decoder) and k_dec_bwd_multi (several mask-only decoders in one launch) and the
// per-decoder launchers (dispatch_dec_bwd).
// Included by nslam_query_dec.hip (once per decoder: its k_dec_bwd instantiations) and
// nslam_query_multi.hip (the file map: nslam_query_core.h).
#include "nslam_query_host.h"
#include "nslam_query_scatter.h"

namespace nslamq {

// Parameter-gradient slab of one wave, addressed as a raw buffer: every update is a buffer store
// (or load + store) with the lane-dependent part of the offset in a VGPR and the uniform part
// (parameter block, row) in soffset, so the ~350 updates per tile cost one address VGPR per block.
// A slab address is owned by one lane of one wave, so no atomics: WG == 1 (a wave's only tile)
// stores, WG == 2 (waves walking several tiles over a zeroed slab) read-modify-writes; both are
// per-lane program-ordered.
struct Slab {
  __amdgpu_buffer_rsrc_t r;
};

__device__ __forceinline__ Slab make_slab(float* base, int floats) {
  return Slab{__builtin_amdgcn_make_buffer_rsrc(base, 0, floats * 4, 0x00020000)};
}

template <int WG>
__device__ __forceinline__ void put(const Slab& A, int lane_off, int uni_off, float v) {
  // the b32 intrinsics move raw bits (unsigned): bit-cast, never convert
  if (WG == 2) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(A.r, lane_off * 4, uni_off * 4, 0));
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), A.r, lane_off * 4, uni_off * 4, 0);
}

// dW[o][kofs + k] += sum_p sa[p][o] * sx[p][k]   for k < kvalid   (dW at slab offset base)
template <int WG>
__device__ __forceinline__ void dw_block_img(const Slab& A, int base, int ldk, int kofs, int kvalid,
                                             const float* __restrict__ sa, const float* __restrict__ sx, int lane) {
  const int h = lane >> 5, j = lane & 31;
  f32x16 acc = zero16();
#pragma unroll
  for (int s = 0; s < 16; ++s) acc = mfma32(sa[(2 * s + h) * TPITCH + j], sx[(2 * s + h) * TPITCH + j], acc);
  if (j < kvalid) {
    const int lo = 4 * h * ldk + j;  // fidx(r, h) = (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
    for (int r = 0; r < 16; ++r) put<WG>(A, lo, base + ((r & 3) + 8 * (r >> 2)) * ldk + kofs, acc[r]);
  }
}
// the same with the input side as a B-operand stream in registers (tape_bop): no sx image
template <int WG>
__device__ __forceinline__ void dw_block_bop(const Slab& A, int base, int ldk, int kofs, int kvalid,
                                             const float* __restrict__ sa, const f32x16& bx, int lane) {
  const int h = lane >> 5, j = lane & 31;
  f32x16 acc = zero16();
#pragma unroll
  for (int s = 0; s < 16; ++s) acc = mfma32(sa[(2 * s + h) * TPITCH + j], bx[s], acc);
  if (j < kvalid) {
    const int lo = 4 * h * ldk + j;
#pragma unroll
    for (int r = 0; r < 16; ++r) put<WG>(A, lo, base + ((r & 3) + 8 * (r >> 2)) * ldk + kofs, acc[r]);
  }
}
template <int WG>
__device__ __forceinline__ void dw_block(const Slab& A, int base, int ldk, int kofs, int kvalid, const Scratch& S,
                                         int lane) {
  dw_block_img<WG>(A, base, ldk, kofs, kvalid, S.sA, S.sX, lane);
}

// db[o] += sum_p sa[p][o]
template <int WG>
__device__ __forceinline__ void db_vec_img(const Slab& A, int base, const float* __restrict__ sa, int lane) {
  const int h = lane >> 5, o = lane & 31;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) s += sa[(2 * t + h) * TPITCH + o];
  s += xor32(s);
  if (h == 0) put<WG>(A, o, base, s);
}
template <int WG>
__device__ __forceinline__ void db_vec(const Slab& A, int base, const Scratch& S, int lane) {
  db_vec_img<WG>(A, base, S.sA, lane);
}

// sA <- d ; then per input tile: sX <- x ; dW += ...
__device__ __forceinline__ void wg_begin(const f32x16& d, const Scratch& S, int lane) { tstore(S.sA, d, lane); }
template <int WG>
__device__ __forceinline__ void wg_block(const Slab& A, int base, int ldk, int kofs, int kvalid, const f32x16& x,
                                         const Scratch& S, int lane) {
  tstore(S.sX, x, lane);
  lds_sync();
  dw_block<WG>(A, base, ldk, kofs, kvalid, S, lane);
  lds_sync();
}
template <int WG>
__device__ __forceinline__ void wg_end(const Slab& A, int base, const Scratch& S, int lane) {
  lds_sync();
  db_vec<WG>(A, base, S, lane);
  lds_sync();
}

// ------------------------------------------------------------------------------------------
// MLP with Fourier embedding: backward (forward recomputed first).
//   gall[GOFS + j], j < NOUT : cotangents of the decoder outputs (per point, both halves)
//   dc : out, d/d(feature block 0) (C layout);  gx : out, d/dx through the embedding (if EMBG)
// Parameter gradients (WG) go through LDS transposes + MFMA over the 32 points and are added
// with atomics shaped as two 128-B row segments.
// ------------------------------------------------------------------------------------------
template <int NC, int WG>
__device__ __forceinline__ void fc_bwd(const float* __restrict__ pk, const XyzPack& L, int i,
                                       const f32x16 (&cin)[NC], const f32x16& dh, const nslam_dec_grad& dg,
                                       const Slab& A, const Scratch& S, int lane, f32x16& dc) {
  gemm_acc(dc, pk + L.FCT(i) * NSLAM_FRAG, dh, lane);  // dz_i = dh_i
  if (WG) {
    wg_begin(dh, S, lane);
#pragma unroll
    for (int c = 0; c < NC; ++c) wg_block<WG>(A, dg.wc[i], 32 * NC, 32 * c, 32, cin[c], S, lane);
    wg_end<WG>(A, dg.bc[i], S, lane);
  }
}

template <int NC, int NOUT, int GOFS, int WG, bool EMBG>
__device__ __forceinline__ void xyz_backward(const float* __restrict__ pk, const f32x16 (&cin)[NC],
                                             const float x[3], const float (&gall)[4], const nslam_dec_grad& dg,
                                             const Slab& A, const Scratch& S, int lane, f32x16& dc, float gx[3],
                                             const float* gh4 = nullptr) {
  const XyzPack L{NC};
  [[maybe_unused]] constexpr int DEC_ = NOUT == 3 ? 3 : (NC == 2 ? 2 : 1);
  const int h = lane >> 5;
  uint32_t m[5];
  f32x16 hs[4];
  const f32x16 h4 = xyz_forward<NC, WG != 0>(pk, cin, x, lane, m, hs);
  PHASE(DEC_, 4);

  // output layer: dh4 = Wo^T g
  f32x16 dh = zero16();
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    const f32x16 w = vec_tile_g(pk + L.Wo() + 32 * j, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] += w[r] * gall[GOFS + j];
  }
  add_gh4(dh, gh4, lane);
  if (WG) {
    tstore(S.sX, h4, lane);
    lds_sync();
    const int f = lane & 31;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int p = 2 * t + h;
        s += S.gtab[p * 4 + GOFS + j] * S.sX[p * TPITCH + f];
      }
      s += xor32(s);
      if (h == 0) put<WG>(A, f, dg.wo + 32 * j, s);
      if (lane == 0) {
        float sb = 0.f;
        for (int p = 0; p < 32; ++p) sb += S.gtab[p * 4 + GOFS + j];
        put<WG>(A, 0, dg.bo + j, sb);
      }
    }
    if (WG == 1 && GOFS + NOUT < 4 && GOFS == 0) {  // colour: output row 3 is never used, store zeros
#pragma unroll
      for (int j = NOUT; j < 4; ++j) {
        if (h == 0) put<1>(A, f, dg.wo + 32 * j, 0.f);
        if (lane == 0) put<1>(A, 0, dg.bo + j, 0.f);
      }
    }
    lds_sync();
  }
  dc = zero16();
  const float* FB = pk + L.FB();
  PHASE(DEC_, 5);

  // layer 4
  fc_bwd<NC, WG>(pk, L, 4, cin, dh, dg, A, S, lane, dc);
  f32x16 da = apply_mask(dh, m[4]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[4], 32, 0, 32, hs[3], S, lane);
    wg_end<WG>(A, dg.b[4], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + L.L4T() * NSLAM_FRAG, da, lane);
  PHASE(DEC_, 6);
  // layer 3 (input = [emb | h2])
  fc_bwd<NC, WG>(pk, L, 3, cin, dh, dg, A, S, lane, dc);
  const f32x16 da3 = apply_mask(dh, m[3]);
  if (WG) {
    wg_begin(da3, S, lane);
#pragma unroll
    for (int b = 0; b < 3; ++b)
      wg_block<WG>(A, dg.w[3], 125, 32 * b, b < 2 ? 32 : 29, emb_tile<false, true>(FB, x, b, lane), S, lane);
    wg_block<WG>(A, dg.w[3], 125, 93, 32, hs[2], S, lane);
    wg_end<WG>(A, dg.b[3], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + (L.L3T() + 3) * NSLAM_FRAG, da3, lane);
  PHASE(DEC_, 7);
  // layer 2
  fc_bwd<NC, WG>(pk, L, 2, cin, dh, dg, A, S, lane, dc);
  da = apply_mask(dh, m[2]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[2], 32, 0, 32, hs[1], S, lane);
    wg_end<WG>(A, dg.b[2], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + L.L2T() * NSLAM_FRAG, da, lane);
  PHASE(DEC_, 8);
  // layer 1
  fc_bwd<NC, WG>(pk, L, 1, cin, dh, dg, A, S, lane, dc);
  da = apply_mask(dh, m[1]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[1], 32, 0, 32, hs[0], S, lane);
    wg_end<WG>(A, dg.b[1], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + L.L1T() * NSLAM_FRAG, da, lane);
  PHASE(DEC_, 9);
  // layer 0 (input = emb)
  fc_bwd<NC, WG>(pk, L, 0, cin, dh, dg, A, S, lane, dc);
  da = apply_mask(dh, m[0]);
  if (WG) {
    wg_begin(da, S, lane);
#pragma unroll
    for (int b = 0; b < 3; ++b)
      wg_block<WG>(A, dg.w[0], 93, 32 * b, b < 2 ? 32 : 29, emb_tile<false, true>(FB, x, b, lane), S, lane);
    wg_end<WG>(A, dg.b[0], S, lane);
  }

  PHASE(DEC_, 10);
  // Fourier features: de_b = L3T_b da3 + L0T_b da0 ; G = de * cos(theta)
  gx[0] = gx[1] = gx[2] = 0.f;
  if (EMBG) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      f32x16 de = zero16();
      gemm_acc(de, pk + (L.L3T() + b) * NSLAM_FRAG, da3, lane);
      gemm_acc(de, pk + (L.L0T() + b) * NSLAM_FRAG, da, lane);
      const f32x16 cs = emb_tile<true, true>(FB, x, b, lane);
      f32x16 G;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 32 * b + 8 * i + 4 * h;
        const f32x4 B0 = *as_global(reinterpret_cast<const f32x4*>(FB + k));
        const f32x4 B1 = *as_global(reinterpret_cast<const f32x4*>(FB + 96 + k));
        const f32x4 B2 = *as_global(reinterpret_cast<const f32x4*>(FB + 192 + k));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gk = de[4 * i + j] * cs[4 * i + j];
          G[4 * i + j] = gk;
          gx[0] += gk * B0[j];
          gx[1] += gk * B1[j];
          gx[2] += gk * B2[j];
        }
      }
      if (WG) {  // dB[j][k] += sum_p x_j[p] G[k][p]
        tstore(S.sA, G, lane);
        lds_sync();
        const int jj = lane & 31;
        const int jc = jj < 3 ? jj : 0;
        f32x16 acc = zero16();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const int p = 2 * s + h;
          const float xv = jj < 3 ? S.xtab[p * 3 + jc] : 0.f;
          acc = mfma32(S.sA[p * TPITCH + jj], xv, acc);
        }
        if (jj < 3) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = 32 * b + fidx(r, h);
            if (k < NSLAM_EMB) put<WG>(A, jj * NSLAM_EMB + 4 * h, dg.B + 32 * b + (r & 3) + 8 * (r >> 2), acc[r]);
          }
        }
        lds_sync();
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[k] += xor32(gx[k]);
  }
  PHASE(DEC_, 11);
}

// MLP_no_xyz (coarse, decoder.py:262-274): backward (noxyz_forward recomputed first)
template <int WG>
__device__ __forceinline__ void noxyz_backward(const float* __restrict__ pk, const f32x16& c, float g,
                                               const nslam_dec_grad& dg, const Slab& A, const Scratch& S, int lane,
                                               f32x16& dc) {
  const NoXyzPack L;
  const int h = lane >> 5;
  uint32_t m[5];
  f32x16 hs[4];
  const f32x16 h4 = noxyz_forward<WG != 0>(pk, c, lane, m, hs);
  f32x16 dh;
  {
    const f32x16 w = vec_tile_g(pk + L.Wo(), lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] = w[r] * g;
  }
  if (WG) {
    tstore(S.sX, h4, lane);
    lds_sync();
    const int f = lane & 31;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int p = 2 * t + h;
      s += S.gtab[p * 4 + 3] * S.sX[p * TPITCH + f];
    }
    s += xor32(s);
    if (h == 0) put<WG>(A, f, dg.wo, s);
    if (lane == 0) {
      float sb = 0.f;
      for (int p = 0; p < 32; ++p) sb += S.gtab[p * 4 + 3];
      put<WG>(A, 0, dg.bo, sb);
    }
    lds_sync();
  }
  dc = zero16();
  // layer 4
  f32x16 da = apply_mask(dh, m[4]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[4], 32, 0, 32, hs[3], S, lane);
    wg_end<WG>(A, dg.b[4], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + L.L4T() * NSLAM_FRAG, da, lane);
  // layer 3 (input = [c | h2])
  da = apply_mask(dh, m[3]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[3], 64, 0, 32, c, S, lane);
    wg_block<WG>(A, dg.w[3], 64, 32, 32, hs[2], S, lane);
    wg_end<WG>(A, dg.b[3], S, lane);
  }
  gemm_acc(dc, pk + L.L3T() * NSLAM_FRAG, da, lane);
  dh = zero16();
  gemm_acc(dh, pk + (L.L3T() + 1) * NSLAM_FRAG, da, lane);
  // layer 2
  da = apply_mask(dh, m[2]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[2], 32, 0, 32, hs[1], S, lane);
    wg_end<WG>(A, dg.b[2], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + L.L2T() * NSLAM_FRAG, da, lane);
  // layer 1
  da = apply_mask(dh, m[1]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[1], 32, 0, 32, hs[0], S, lane);
    wg_end<WG>(A, dg.b[1], S, lane);
  }
  dh = zero16();
  gemm_acc(dh, pk + L.L1T() * NSLAM_FRAG, da, lane);
  // layer 0 (input = c)
  da = apply_mask(dh, m[0]);
  if (WG) {
    wg_begin(da, S, lane);
    wg_block<WG>(A, dg.w[0], 32, 0, 32, c, S, lane);
    wg_end<WG>(A, dg.b[0], S, lane);
  }
  gemm_acc(dc, pk + L.L0T() * NSLAM_FRAG, da, lane);
}

// ------------------------------------------------------------------------------------------
// Backward from saved ReLU masks (decoders without parameter gradients): no forward recompute,
// no embedding sin, no feature gather.  dh_4 = Wo^T g; for i = 4..0: dc += FCT_i dh_i and
// dh_{i-1} = L_iT mask_i(dh_i) (layer 3 through its hidden block); EMBG adds d/dx through the
// Fourier features from mask_3(dh_3) and mask_0(dh_0).
// ------------------------------------------------------------------------------------------
// TR: dc is formed transposed (lane (c, h) register r = channel c of point F(r, h); gemm_acc_t), the
// layout the lean scatter walk consumes without an LDS transpose (only without EMBG: coord_grad
// reads the C layout)
// img (EMBG; the d/dpts mask-only kernels): the caller's scatter image — dc, complete before the Fourier
// backward, is stored there (tstore layout) and does not hold 16 registers through it (the caller's
// scatter reads it there; its coordinate gradient reads it back: tload)
template <int NC, int NOUT, int GOFS, bool EMBG, bool TR = false>
__device__ __forceinline__ void xyz_backward_saved(const float* __restrict__ pk, const uint32_t m[5],
                                                   const float x[3], const float (&gall)[4], int lane, f32x16& dc,
                                                   float gx[3], const float* gh4 = nullptr,
                                                   float* __restrict__ img = nullptr) {
  static_assert(!(TR && EMBG), "d/dpts needs dc in the C layout");
  const XyzPack L{NC};
  const int h = lane >> 5;
  f32x16 dh = zero16();
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    const f32x16 w = vec_tile_g(pk + L.Wo() + 32 * j, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] += w[r] * gall[GOFS + j];
  }
  add_gh4(dh, gh4, lane);
  dc = zero16();
  gemm_acc_tr<TR>(dc, pk + L.FCT(4) * NSLAM_FRAG, dh, lane);
  f32x16 da = apply_mask(dh, m[4]);
  dh = zero16();
  gemm_acc(dh, pk + L.L4T() * NSLAM_FRAG, da, lane);
  gemm_acc_tr<TR>(dc, pk + L.FCT(3) * NSLAM_FRAG, dh, lane);
  const f32x16 da3 = apply_mask(dh, m[3]);
  dh = zero16();
  gemm_acc(dh, pk + (L.L3T() + 3) * NSLAM_FRAG, da3, lane);
  gemm_acc_tr<TR>(dc, pk + L.FCT(2) * NSLAM_FRAG, dh, lane);
  da = apply_mask(dh, m[2]);
  dh = zero16();
  gemm_acc(dh, pk + L.L2T() * NSLAM_FRAG, da, lane);
  gemm_acc_tr<TR>(dc, pk + L.FCT(1) * NSLAM_FRAG, dh, lane);
  da = apply_mask(dh, m[1]);
  dh = zero16();
  gemm_acc(dh, pk + L.L1T() * NSLAM_FRAG, da, lane);
  gemm_acc_tr<TR>(dc, pk + L.FCT(0) * NSLAM_FRAG, dh, lane);
  gx[0] = gx[1] = gx[2] = 0.f;
  if (EMBG) {
    da = apply_mask(dh, m[0]);
    if (img) {
      tstore(img, dc, lane);
      asm volatile("" ::: "memory");  // (read back after the scatter, not kept in registers meanwhile)
    }
    const float* FB = pk + L.FB();
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      f32x16 de = zero16();
      gemm_acc(de, pk + (L.L3T() + b) * NSLAM_FRAG, da3, lane);
      gemm_acc(de, pk + (L.L0T() + b) * NSLAM_FRAG, da, lane);
      const f32x16 cs = emb_tile<true, true>(FB, x, b, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 32 * b + 8 * i + 4 * h;
        const f32x4 B0 = *as_global(reinterpret_cast<const f32x4*>(FB + k));
        const f32x4 B1 = *as_global(reinterpret_cast<const f32x4*>(FB + 96 + k));
        const f32x4 B2 = *as_global(reinterpret_cast<const f32x4*>(FB + 192 + k));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gk = de[4 * i + j] * cs[4 * i + j];
          gx[0] += gk * B0[j];
          gx[1] += gk * B1[j];
          gx[2] += gk * B2[j];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[k] += xor32(gx[k]);
  }
}

template <bool TR = false>
__device__ __forceinline__ void noxyz_backward_saved(const float* __restrict__ pk, const uint32_t m[5], float g,
                                                     int lane, f32x16& dc) {
  const NoXyzPack L;
  f32x16 dh;
  {
    const f32x16 w = vec_tile_g(pk + L.Wo(), lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] = w[r] * g;
  }
  dc = zero16();
  f32x16 da = apply_mask(dh, m[4]);
  dh = zero16();
  gemm_acc(dh, pk + L.L4T() * NSLAM_FRAG, da, lane);
  da = apply_mask(dh, m[3]);
  gemm_acc_tr<TR>(dc, pk + L.L3T() * NSLAM_FRAG, da, lane);
  dh = zero16();
  gemm_acc(dh, pk + (L.L3T() + 1) * NSLAM_FRAG, da, lane);
  da = apply_mask(dh, m[2]);
  dh = zero16();
  gemm_acc(dh, pk + L.L2T() * NSLAM_FRAG, da, lane);
  da = apply_mask(dh, m[1]);
  dh = zero16();
  gemm_acc(dh, pk + L.L1T() * NSLAM_FRAG, da, lane);
  da = apply_mask(dh, m[0]);
  gemm_acc_tr<TR>(dc, pk + L.L0T() * NSLAM_FRAG, da, lane);
}

// One backward launch per decoder: the decoder's forward is recomputed, its grid gradient is
// scattered, its parameter gradients are accumulated and its share of d/dpts is added into g_pts
// (launches on one stream are ordered and each point is owned by one lane pair: plain
// read-modify-write, no atomics).  With parameter gradients every wave owns a slab of the
// workspace (WG == 1: one tile per wave, slab = tile; WG == 2: a fixed number of waves walk the
// tiles over pre-zeroed slabs) and k_slab_reduce sums the slabs in a fixed order
// (deterministic).  LDS holds only each wave's transpose scratch: LDS float atomics
// (ds_add_f32, one RMW per lane) were the bottleneck of the previous shared-accumulator design.
// (kWavesBwd waves per workgroup, at most kMaxSlabs one-tile slabs: nslam_query_host.h)
constexpr int kScratchFloats = 2 * TILE_FLOATS + 32 * 4 + 32 * 3 + 32 * 8 * 2 + 32;

// lean mapping tile (saved masks, no weight or point gradients): dc transposed, walk without LDS image
constexpr bool lean_tr(int WG, bool PG, bool SAVED) { return SAVED && WG == 0 && !PG; }
// per-wave LDS floats of a backward kernel variant
constexpr int bwd_scratch_floats(int WG, bool PG, bool SAVED) {
  return WG ? kScratchFloats : lean_tr(WG, PG, SAVED) ? kWalkFloats : TILE_FLOATS + kWalkFloats;
}

// LIVE (mask-only mapping tiles): lane p of tile t takes point live[32 t + p] of the decoder's live-point
// list (nslam_live_points: the points with a frustum-selected corner, ascending), nlive entries; lanes past
// the list behave like tail lanes.  Each point's cotangent is its own MFMA column, so it does not depend
// on the tile the point sits in; only the runs the scatter walk merges before its atomics regroup.
template <int DEC, int WG, bool PG, bool FIRST, bool SAVED, bool LIVE = false>
__device__ __forceinline__ void dec_bwd_tile(const QueryKArgs& a, int64_t tile, const Slab& A, const Scratch& S,
                                             int lane, double* __restrict__ gpts, int64_t gbase = 0,
                                             const int32_t* __restrict__ live = nullptr, int64_t nlive = 0) {
  static_assert(!LIVE || (SAVED && WG == 0 && !PG), "live-point tiles: the mask-only mapping backward");
  // gpts: d/dpts of point idx at gpts[(idx - gbase) * 3 + k] (gbase: a tile's LDS staging rows)
  // Every scratch / slab address is a function of the lane only, i.e. invariant across the tile
  // loop; letting LICM hoist the ~300 of them pins (and spills) the register file.  Re-derive
  // them per tile.
  asm volatile("" : "+v"(lane));
  PHASE(DEC, 0);
  const int h = lane >> 5, p = lane & 31;
  int64_t idx = tile * 32 + p;
  if (LIVE) {  // (a.n: an invalid lane; so is an entry that is no point index, whatever the list holds)
    const uint32_t v = idx < nlive ? (uint32_t)live[idx] : 0xffffffffu;
    idx = (int64_t)v < a.n ? (int64_t)v : a.n;
  }
  const Pt q = load_point(a, idx);
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  if (q.valid) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.g_raw + idx * 4);
    g[0] = v[0];
    g[1] = v[1];
    g[2] = v[2];
    g[3] = q.inside ? v[3] : 0.f;  // ret[~mask,3]=100 blocks the occupancy gradient
  }
  if (WG) {
    if (h == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) S.gtab[p * 4 + j] = g[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) S.xtab[p * 3 + j] = q.x[j];
    }
    lds_sync();
  }
  const nslam_grid& gr = a.c.grid[DEC];
  const nslam_dec_grad& dg = a.c.dgrad[DEC];
  const float* pk = a.c.packed[DEC];
  // the colour decoder's h4 cotangent of a direct MLP(color=True) caller (ABI v17), none for tail lanes
  const float* gh4 = (DEC == NSLAM_DEC_COLOR && a.c.g_h4 && q.valid) ? a.c.g_h4 + idx * 32 : nullptr;
  // The weight fragments are loop-invariant across the tile loop; hoisting their ~100 loads out of
  // the loop would pin hundreds of registers.  Launder the base pointer per tile so they stay put.
  asm volatile("" : "+s"(pk));
  PHASE(DEC, 1);
  Corners cr;
  grid_corners(cr, gr, q);
  ScatterCorners scn{};
  if (WG == 0 && gr.grad) scn = resolve_corners(gr.slot, cr, q.valid, lane);
  PHASE(DEC, 2);
  f32x16 dc;
  float gx[3] = {0.f, 0.f, 0.f};
  static_assert(!(SAVED && WG), "weight gradients from saved masks run as k_color_wgrad");
  // the lean mapping chain forms dc transposed for the register-only scatter walk (lean_tr)
  constexpr bool TR = lean_tr(WG, PG, SAVED);
  float* const tab = TR ? S.sA : S.sA + TILE_FLOATS;  // the walk table (after the transpose image if any)
  // d/dpts mask-only tiles (not the coarse decoder's: its chain keeps dc in registers): dc waits in the
  // scatter image while the Fourier backward runs
  constexpr bool IMGDC = SAVED && WG == 0 && PG && DEC != NSLAM_DEC_COARSE;
  float* const img = IMGDC ? S.sA : nullptr;
  if (SAVED) {  // masks from the forward: no recompute (the mask-only chain)
    uint32_t m[5];
    if (LIVE)
      load_masks_at(a, DEC, q.valid ? idx : 0, h, m);
    else
      load_masks(a, DEC, tile, m, lane);
    // the walk table goes to LDS before the chain (its corner rows and weights need no registers
    // through it); the slot loads were issued before the masks, so this waits for nothing extra
    if (WG == 0 && gr.grad) stage_walk_table(tab, scn, cr.cell, lane);
    if (DEC == NSLAM_DEC_COARSE) {
      noxyz_backward_saved<TR>(pk, m, g[3], lane, dc);
    } else if (DEC == NSLAM_DEC_FINE) {
      xyz_backward_saved<2, 1, 3, PG, TR>(pk, m, q.x, g, lane, dc, gx, nullptr, img);
    } else if (DEC == NSLAM_DEC_COLOR) {
      xyz_backward_saved<1, 3, 0, PG, TR>(pk, m, q.x, g, lane, dc, gx, gh4, img);
    } else {
      xyz_backward_saved<1, 1, 3, PG, TR>(pk, m, q.x, g, lane, dc, gx, nullptr, img);
    }
  } else if (DEC == NSLAM_DEC_COARSE) {
    const f32x16 c = gather_tile(gr.data, cr, lane);
    noxyz_backward<WG>(pk, c, g[3], dg, A, S, lane, dc);
  } else if (DEC == NSLAM_DEC_FINE) {
    Corners cm;
    grid_corners(cm, a.c.grid[NSLAM_DEC_MIDDLE], q);
    // the middle feature enters the fine decoder under torch.no_grad (decoder.py:184-187)
    const f32x16 cf[2] = {gather_tile(gr.data, cr, lane), gather_tile(a.c.grid[NSLAM_DEC_MIDDLE].data, cm, lane)};
    xyz_backward<2, 1, 3, WG, PG || WG>(pk, cf, q.x, g, dg, A, S, lane, dc, gx);
  } else {
    const f32x16 c[1] = {gather_tile(gr.data, cr, lane)};
    PHASE(DEC, 3);
    if (DEC == NSLAM_DEC_COLOR)  // the colour decoder's 4th output is overwritten by the combiner
      xyz_backward<1, 3, 0, WG, PG || WG>(pk, c, q.x, g, dg, A, S, lane, dc, gx, gh4);
    else
      xyz_backward<1, 1, 3, WG, PG || WG>(pk, c, q.x, g, dg, A, S, lane, dc, gx);
  }
  PHASE(DEC, 12);
  if (gr.grad) {
    if (WG) {
      scatter_grid_grad_halves(gr.grad, gr.slot, cr, dc, q.valid, S, lane);
    } else {  // walk table: the lean kernels' slot after the transpose image
      scatter_grid_grad_uniform<SAVED, TR, IMGDC>(gr.grad, scn, cr.cell, dc, S.sA, tab, lane);
    }
  }
  PHASE(DEC, 13);
  if (PG) {
    double gp[3] = {(double)gx[0], (double)gx[1], (double)gx[2]};
    if (SAVED && WG == 0) {
      // the corners again (the same arithmetic, so the same values) instead of 27 registers held across
      // the chain; the laundered coordinates keep the compiler from merging the two computations
      Pt q2 = q;
#pragma unroll
      for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(q2.p[k]));
      grid_corners(cr, gr, q2);
    }
    if (IMGDC) {
      lds_sync();  // (the scatter read the image; the reads below are this wave's own stores)
      dc = tload(S.sA, lane);
    }
    coord_grad(gr, cr, dc, lane, gp);
    if (h == 0 && q.valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        gpts[(idx - gbase) * 3 + k] = FIRST ? gp[k] : gpts[(idx - gbase) * 3 + k] + gp[k];
    }
  }
  PHASE(DEC, 14);
}

#ifndef NSLAM_LEAN_LB
#define NSLAM_LEAN_LB 2  // min waves per SIMD of the mask-only kernels (experiments: 3..5)
#endif
template <int DEC, int WG, bool PG, bool FIRST, bool SAVED>
__global__ __launch_bounds__(64 * kWavesBwd, (WG || PG || !SAVED) ? 2 : NSLAM_LEAN_LB) void k_dec_bwd(QueryKArgs a, float* __restrict__ slab,
                                                                 int acc_floats) {
  // per-wave scratch: the scatter needs sA + corner rows/weights; weight gradients add sX and
  // the per-point tables (sizing LDS per variant keeps the lean kernels at 5+ waves/SIMD)
  // (the lean kernels' scatter walk needs only the sA transpose image and its walk table)
  constexpr int kScr = bwd_scratch_floats(WG, PG, SAVED);
  __shared__ __attribute__((aligned(16))) float lds[kWavesBwd * kScr];
  const int lane = threadIdx.x & 63, wave = wave_id();
  float* sc = lds + wave * kScr;
  Scratch S;
  S.sA = sc;
  if (WG) {
    S.sX = sc + TILE_FLOATS;
    S.gtab = sc + 2 * TILE_FLOATS;
    S.xtab = S.gtab + 32 * 4;
    S.crow = reinterpret_cast<int*>(S.xtab + 32 * 3);
    S.cw = reinterpret_cast<float*>(S.crow + 32 * 8);
    S.ccell = reinterpret_cast<int*>(S.cw + 32 * 8);
  } else {
    S.sX = S.gtab = S.xtab = S.cw = nullptr;
    S.crow = S.ccell = nullptr;
  }
  const int64_t ntiles = (a.n + 31) / 32;
  const int64_t w = (int64_t)blockIdx.x * kWavesBwd + wave;
  const Slab A = make_slab(WG ? slab + (size_t)w * acc_floats : slab, WG ? acc_floats : 0);
  if (WG == 0) {  // one tile per wave (grid covers all tiles)
    if (w < ntiles) dec_bwd_tile<DEC, WG, PG, FIRST, SAVED>(a, w, A, S, lane, a.g_pts);
    return;
  }
  if (WG == 1) {  // one tile per wave, then the workgroup folds its waves' slabs into its first one
    if (w < ntiles) dec_bwd_tile<DEC, WG, PG, FIRST, SAVED>(a, w, A, S, lane, a.g_pts);
    // the slabs were just written by this CU (L2-resident): summing them here in wave order (a
    // fixed order: deterministic) leaves k_slab_reduce a quarter of the bytes to read
    __syncthreads();
    const int64_t w0 = (int64_t)blockIdx.x * kWavesBwd;
    const int nv = (int)(ntiles - w0 < kWavesBwd ? ntiles - w0 : kWavesBwd);
    f32x4* s0 = reinterpret_cast<f32x4*>(slab + (size_t)w0 * acc_floats);
    const int q = acc_floats / 4;
    for (int i = threadIdx.x; i < q; i += blockDim.x) {
      f32x4 t = s0[i];
      for (int v = 1; v < nv; ++v) t += s0[(size_t)v * q + i];
      s0[i] = t;
    }
    return;
  }
#pragma nounroll
  for (int64_t tile = w; tile < ntiles; tile += (int64_t)gridDim.x * kWavesBwd)
    dec_bwd_tile<DEC, WG, PG, FIRST, SAVED>(a, tile, A, S, lane, a.g_pts);
}

// Mask-only backward of several decoders in ONE launch (ABI v10 nslam_query_bwd_decoders): the
// decoders' workgroups are interleaved over blockIdx (part = blockIdx % ndec), so frozen decoders
// that would otherwise run as concurrent launches on separate streams (tracking: middle, fine and
// colour; mapping: middle and fine) need no fork / join between streams.  Each part writes its own
// d/dpts buffer gp[part] (no cross-decoder accumulation, no atomics on points).
struct MultiDecArgs {
  int ndec;
  int dec[4];
  double* gp[4];
  // LIVE launches (nslam_query_bwd_decoders_live): each part's live-point list and its device length
  const int32_t* live[4];
  const int64_t* nlive[4];
};
// (a colour decoder with weight gradients runs here as its lean chain too: grid gradient, d/dpts;
// its parameter gradients come from k_color_wgrad, nslam_color_wgrad.hip)
// Register bound of the mapping (no d/dpts) variant: 4 waves/SIMD -> 106 VGPRs (the walk table staged
// before the chain frees its corner registers).  A/B on one box, 3 alternating rounds (r4t): 0.2287 ms
// per iteration at the old 2-wave bound (115 VGPRs), 0.2208 ms at 4, 0.2260 ms at 5 (96 VGPRs: one
// resident round for room0's 4500 waves, but the standalone launch only 1 % shorter than at 4).
#ifndef NSLAM_MULTI_LB
#define NSLAM_MULTI_LB 4
#endif
#ifndef NSLAM_MULTI_PG_LB
#define NSLAM_MULTI_PG_LB 3  // the d/dpts (tracking, bundle adjustment) variant: 163 VGPRs with dc in the
                             // scatter image through the Fourier backward (218 before: 2 waves/SIMD)
#endif
// LIVE: the grid is sized for every point (a captured launch stays valid whatever the lists hold); a wave
// whose tile lies past its part's list exits at once.
template <bool PG, bool LIVE = false>
__global__ __launch_bounds__(64 * kWavesBwd, PG ? NSLAM_MULTI_PG_LB : NSLAM_MULTI_LB) void k_dec_bwd_multi(QueryKArgs a, MultiDecArgs m) {
  static_assert(!(PG && LIVE), "d/dpts is needed for every point");
  constexpr int kScr = bwd_scratch_floats(0, PG, true);
  __shared__ __attribute__((aligned(16))) float lds[kWavesBwd * kScr];
  const int lane = threadIdx.x & 63, wave = wave_id();
  Scratch S;
  S.sA = lds + wave * kScr;
  S.sX = S.gtab = S.xtab = S.cw = nullptr;
  S.crow = S.ccell = nullptr;
  const int part = (int)(blockIdx.x % (unsigned)m.ndec);
  // selects, not a dynamic index into the by-value argument (that would copy it to scratch)
  const int dec = part == 0 ? m.dec[0] : part == 1 ? m.dec[1] : part == 2 ? m.dec[2] : m.dec[3];
  double* gp = part == 0 ? m.gp[0] : part == 1 ? m.gp[1] : part == 2 ? m.gp[2] : m.gp[3];
  const int64_t w = (int64_t)(blockIdx.x / (unsigned)m.ndec) * kWavesBwd + wave;
  const int32_t* live = nullptr;
  int64_t nlive = a.n;
  if (LIVE) {
    live = part == 0 ? m.live[0] : part == 1 ? m.live[1] : part == 2 ? m.live[2] : m.live[3];
    const int64_t* np = part == 0 ? m.nlive[0] : part == 1 ? m.nlive[1] : part == 2 ? m.nlive[2] : m.nlive[3];
    nlive = *np;
    if (nlive > a.n) nlive = a.n;  // (never more entries than the list's capacity)
  }
  const int64_t ntiles = (nlive + 31) / 32;
  if (w >= ntiles) return;
  TL(1, 0, part);
  const Slab A = make_slab(nullptr, 0);
  switch (dec) {
    case NSLAM_DEC_COARSE:
      dec_bwd_tile<NSLAM_DEC_COARSE, 0, PG, true, true, LIVE>(a, w, A, S, lane, gp, 0, live, nlive);
      break;
    case NSLAM_DEC_MIDDLE:
      dec_bwd_tile<NSLAM_DEC_MIDDLE, 0, PG, true, true, LIVE>(a, w, A, S, lane, gp, 0, live, nlive);
      break;
    case NSLAM_DEC_FINE:
      dec_bwd_tile<NSLAM_DEC_FINE, 0, PG, true, true, LIVE>(a, w, A, S, lane, gp, 0, live, nlive);
      break;
    default: dec_bwd_tile<NSLAM_DEC_COLOR, 0, PG, true, true, LIVE>(a, w, A, S, lane, gp, 0, live, nlive); break;
  }
  TL(1, 1, 0);
}

template <int DEC, int WG, bool PG, bool FIRST, bool SAVED = false>
int launch_one(const QueryKArgs& a, float* slab, int acc, int64_t blocks, hipStream_t s) {
  hipLaunchKernelGGL((k_dec_bwd<DEC, WG, PG, FIRST, SAVED>), dim3((unsigned)blocks), dim3(64 * kWavesBwd), 0, s, a,
                     slab, acc);
  return hip_status();
}

template <int DEC, int WG, bool PG>
int launch_dec_bwd(const QueryKArgs& a, bool first, float* slab, hipStream_t s) {
  const int64_t tiles = (a.n + 31) / 32;
  if (WG == 0) {
    const int64_t blocks = (tiles + kWavesBwd - 1) / kWavesBwd;
    if (a.c.saved_masks)
      return first ? launch_one<DEC, 0, PG, true, true>(a, nullptr, 0, blocks, s)
                   : launch_one<DEC, 0, PG, false, true>(a, nullptr, 0, blocks, s);
    return first ? launch_one<DEC, 0, PG, true>(a, nullptr, 0, blocks, s)
                 : launch_one<DEC, 0, PG, false>(a, nullptr, 0, blocks, s);
  }
  const nslam_dec_grad& dg = a.c.dgrad[DEC];
  const int acc = acc_floats_of(dg);
  const int64_t nslab = n_slabs(tiles);
  const int64_t blocks = (nslab + kWavesBwd - 1) / kWavesBwd;
  // the colour decoder's weight gradients from the forward's activation tape when it is there: the
  // lean chain (grid gradient), then k_color_wgrad (which does not read anything the chain wrote)
  constexpr bool kTapeable = DEC == NSLAM_DEC_COLOR && !PG;
  int rc;
  if constexpr (kTapeable) {
    if (cw_tape_path(&a.c)) {
      rc = launch_one<DEC, 0, false, true, true>(a, nullptr, 0, (tiles + kWavesBwd - 1) / kWavesBwd, s);
      return rc ? rc : launch_color_wgrad(a, slab, s);
    }
  }
  if (tiles > max_slabs() && hipMemsetAsync(slab, 0, (size_t)nslab * acc * sizeof(float), s) != hipSuccess)
    return hip_status();
  if (tiles <= max_slabs()) {
    rc = first ? launch_one<DEC, 1, PG, true>(a, slab, acc, blocks, s)
               : launch_one<DEC, 1, PG, false>(a, slab, acc, blocks, s);
  } else {
    rc = first ? launch_one<DEC, 2, PG, true>(a, slab, acc, blocks, s)
               : launch_one<DEC, 2, PG, false>(a, slab, acc, blocks, s);
  }
  if (rc) return rc;
  return slab_reduce(dg, slab, tiles <= max_slabs(), nslab, blocks, acc, s);
}

template <int DEC>
int dispatch_dec_bwd(const QueryKArgs& a, bool first, float* slab, hipStream_t s) {
  const bool wg = a.c.dgrad[DEC].base != nullptr;
  const bool pg = a.c.need_pts_grad != 0;
  if (wg && pg && a.c.saved_masks) {
    // Split instead of the combined kernel (which spills ~100 VGPRs): parameter + grid gradients
    // first, then d/dpts from the saved masks with the grid scatter switched off.
    int rc = launch_dec_bwd<DEC, 1, false>(a, first, slab, s);
    if (rc) return rc;
    QueryKArgs b = a;
    b.c.grid[DEC].grad = nullptr;
    b.c.dgrad[DEC].base = nullptr;
    return launch_dec_bwd<DEC, 0, true>(b, first, nullptr, s);
  }
  if (wg && pg) return launch_dec_bwd<DEC, 1, true>(a, first, slab, s);
  if (wg) return launch_dec_bwd<DEC, 1, false>(a, first, slab, s);
  if (pg) return launch_dec_bwd<DEC, 0, true>(a, first, slab, s);
  return launch_dec_bwd<DEC, 0, false>(a, first, slab, s);
}

}  // namespace nslamq
