#pragma once
// nslam_query_scatter.h — the backward's way from a tile's feature cotangent into the grids: the wave's
// LDS scratch, the grid-gradient scatter (the uniform walk of the mask-only kernels, the per-half walk of
// the weight-gradient kernels) and the coordinate gradient through the trilinear weights.
// Included by nslam_query_bwd.h only (the file map: nslam_query_core.h).
#include "nslam_query_core.h"

namespace nslamq {

// ------------------------------------------------------------------------------------------
// a backward wave's private LDS scratch (transpose images for the weight gradients, scatter tables)
// ------------------------------------------------------------------------------------------
struct Scratch {
  float* sA;    // [32][33] transposed cotangent tile
  float* sX;    // [32][33] transposed input tile
  float* gtab;  // [32][4]  per-point output cotangents
  float* xtab;  // [32][3]  per-point x (float)
  int* crow;    // [32][8]  corner rows (grad slots when the grid gradient is frustum-compacted)
  float* cw;    // [32][8]
  int* ccell;   // [32]     cell of each point (packed lower-corner coordinates): the run-merge key
};

// ------------------------------------------------------------------------------------------
// grid gradient scatter (atomics shaped as two 128-B row segments per wave-instruction) and
// coordinate gradient through the trilinear weights
// ------------------------------------------------------------------------------------------
// Stage a tile's corner rows / weights for the scatter.  With a slot map (ABI v6: frustum-
// compacted grid gradient, Mapper.py:314-333) corner row r accumulates into compact row slot[r];
// corners outside the frustum selection (slot -1) get weight 0, i.e. no atomic: the reference
// never forms their gradient (its optimised tensor is the masked vector, Mapper.py:394-401).
__device__ __forceinline__ void stage_corners(const Corners& cr, const int32_t* __restrict__ slot, bool valid,
                                              const Scratch& S, int lane) {
  if (lane < 32) {
    const int p = lane;
    S.ccell[p] = cr.cell;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int r = cr.row[k];
      float w = valid ? cr.w[k] : 0.f;
      if (slot) {
        r = slot[r];
        if (r < 0) {
          r = 0;
          w = 0.f;
        }
      }
      S.crow[p * 8 + k] = r;
      S.cw[p * 8 + k] = w;
    }
  }
}

// grid-gradient add of one lane's channel
__device__ __forceinline__ void grid_add(float* p, float v) { unsafeAtomicAdd(p, v); }

__device__ __forceinline__ float rdlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// Corners 4h..4h+3 of this lane's point, frustum-slot mapped (slot -1: weight 0, no atomic).
// Issued right after the corners are known, so the slot gathers' latency hides behind the
// decoder backward instead of stalling the scatter.
struct ScatterCorners {
  int rk[4];
  float wk[4];
};
__device__ __forceinline__ ScatterCorners resolve_corners(const int32_t* __restrict__ slot, const Corners& cr,
                                                          bool valid, int lane) {
  const int h = lane >> 5;
  ScatterCorners sc;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = h ? cr.row[4 + i] : cr.row[i];
    float w = valid ? (h ? cr.w[4 + i] : cr.w[i]) : 0.f;
    if (slot) {
      r = slot[r];
      if (r < 0) {
        r = 0;
        w = 0.f;
      }
    }
    sc.rk[i] = r;
    sc.wk[i] = w;
  }
  return sc;
}

// The walk keeps each corner voxel of the current cell in a register chosen by the voxel's own
// coordinate parities, not by its position in the cell: lane half h holds the corners with
// x & 1 == h, register j those with (y & 1) + 2 (z & 1) == j.  Stepping to a neighbouring cell then
// leaves every shared voxel where it is (its running sum simply continues), and only the voxels
// that leave the cell are flushed and their registers cleared — no data moves between registers.
// Walk table of one tile (per wave, kWalkFloats): entry (p, h) holds point p's weights (then its
// frustum rows) of the four corners in lane half h, register order j, so one ds_read_b128 with a
// half-uniform address (an LDS broadcast) fetches them.
constexpr int kWalkFloats = 2 * 32 * 8;
__device__ __forceinline__ void stage_walk_table(float* __restrict__ tab, const ScatterCorners& sc, int cellk,
                                                 int lane) {
  // lane (hz, p) resolved corners 4 hz + i, i = dx + 2 dy, of the cell with lower corner cellk
  const int hz = lane >> 5, p = lane & 31;
  const int px = cellk & 1, py = (cellk >> 10) & 1, pz = (cellk >> 20) & 1;
  float* w = tab + p * 8;
  int* r = reinterpret_cast<int*>(tab + 256) + p * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (((i & 1) ^ px) << 2) | ((i >> 1) ^ py) | ((hz ^ pz) << 1);
    w[e] = sc.wk[i];
    r[e] = sc.rk[i];
  }
}

// Step codes of the walk: every lane evaluates, in parallel before the
// walk, what the step from point p-1's cell to point p's does — bit 8: the cell changes; bit 4 hh + j:
// voxel (hh, j) of the previous cell is kept (a neighbouring-cell step).  The walk itself then
// reads one code per point (v_readlane) instead of deriving the steps' axis deltas and parities on the
// scalar unit point after point (~3k SALU instructions per tile, shared by the CU's waves).
__device__ __forceinline__ int walk_code(int cellk, int lane) {
  const int p = lane & 31;
  const int prev = __shfl(cellk, (lane & 32) | ((p + 31) & 31), 64);  // point p - 1 (same half)
  if (p == 0) return 0x100;        // the first point: nothing accumulated, nothing kept
  if (prev == cellk) return 0;     // the same cell: no step
  const int ax = (cellk & 1023) - (prev & 1023);
  const int ay = ((cellk >> 10) & 1023) - ((prev >> 10) & 1023);
  const int az = (cellk >> 20) - (prev >> 20);
  const int px = prev & 1, py = (prev >> 10) & 1, pz = (prev >> 20) & 1;
  int code = 0x100;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const bool kx = ax == 0 || (ax == 1 && (hh ^ px) == 1) || (ax == -1 && (hh ^ px) == 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int dy = (j & 1) ^ py, dz = (j >> 1) ^ pz;
      const bool ky = ay == 0 || (ay == 1 && dy == 1) || (ay == -1 && dy == 0);
      const bool kz = az == 0 || (az == 1 && dz == 1) || (az == -1 && dz == 0);
      if (kx && ky && kz) code |= 1 << (4 * hh + j);
    }
  }
  return code;
}

// STAGED: the caller wrote the walk table already.  TR: dc arrives transposed (xyz_backward_saved<..., TR>):
// lane (ch, h) holds channel ch of points F(r, h), and one v_permlane32_swap per register hands every
// lane both halves' points — the walk's cotangent columns straight from registers, no LDS image.
template <bool STAGED = false, bool TR = false, bool IMG_READY = false>
__device__ __forceinline__ void scatter_grid_grad_uniform(float* __restrict__ grad, const ScatterCorners& sc,
                                                          int cellk, const f32x16& dc, float* __restrict__ img,
                                                          float* __restrict__ tab, int lane) {
  // Points of a tile are consecutive samples of (mostly) one ray: a voxel's contributions from a
  // run of cells touching it are summed in one register and flushed once (one atomic per voxel per
  // run).  The whole wave walks the tile's 32 points in step (fully unrolled, uniform control
  // flow); lane (h, ch) owns channel ch of its half's four corners, and the two halves hold x-
  // neighbours, i.e. adjacent rows of the channels-last grid, so every flush wave-instruction adds
  // one contiguous 256-B segment (the full-rate shape of a float atomic).  Per point: the cell by
  // v_readlane (it steers the uniform branch), weights and rows by broadcast LDS reads of the walk
  // table, and the cotangent column of channel ch from one LDS transpose of dc.
  const int h = lane >> 5, ch = lane & 31;
  float vlo[16], vhi[16];  // TR: channel ch of point F(r, 0) / F(r, 1)
  if (TR) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // (through a scalar: clang's __builtin_bit_cast of a vector-element lvalue reads element 0)
      const float d = dc[r];
      const unsigned u = __builtin_bit_cast(unsigned, d);
      const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);  // {lower half's, upper half's}
      vlo[r] = __builtin_bit_cast(float, (unsigned)sw[0]);
      vhi[r] = __builtin_bit_cast(float, (unsigned)sw[1]);
    }
  } else if (!IMG_READY) {  // (IMG_READY: the caller's chain left dc in img already)
    tstore(img, dc, lane);
  }
  if (!STAGED) stage_walk_table(tab, sc, cellk, lane);
  lds_sync();
  const f32x4* wt = reinterpret_cast<const f32x4*>(tab) + h;        // (t, h) at wt[2 t]
  const i32x4* rt = reinterpret_cast<const i32x4*>(tab + 256) + h;  // (t, h) at rt[2 t]
  float acc[4], wsum[4];
  int rows[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = 0.f;
    wsum[j] = 0.f;
    rows[j] = 0;
  }
  const int codes = walk_code(cellk, lane);
#pragma unroll
  for (int t = 0; t < 32; ++t) {
    const int code = __builtin_amdgcn_readlane(codes, t);
    // point t = F(r, hh): r = (t & 3) + 4 (t >> 3), hh = (t >> 2) & 1
    const float vc = TR ? (((t >> 2) & 1) ? vhi[(t & 3) + 4 * (t >> 3)] : vlo[(t & 3) + 4 * (t >> 3)])
                        : img[t * TPITCH + ch];
    const f32x4 w = wt[2 * t];
    const i32x4 nr = rt[2 * t];
    if (code & 0x100) {  // wave-uniform: the walk steps to another cell
      const int kb = code >> (4 * h);  // this half's voxels of the previous cell that stay
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool keep = (kb >> j) & 1;
        // one exec-masked flush (both conditions evaluated: no nested branch)
        if ((!keep) & (wsum[j] != 0.f)) grid_add(grad + (size_t)rows[j] * NSLAM_C_DIM + ch, acc[j]);
        acc[j] = keep ? acc[j] : 0.f;
        wsum[j] = keep ? wsum[j] : 0.f;
        rows[j] = nr[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] += w[j] * vc;
      wsum[j] += w[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (wsum[j] != 0.f) grid_add(grad + (size_t)rows[j] * NSLAM_C_DIM + ch, acc[j]);
  lds_sync();
}

// Per-half variant (weight-gradient kernels): half h walks points 16h..16h+15 on its own, every
// flush wave-instruction is one 128-B row segment.  Kept for the register-starved weight-gradient
// kernels, where the uniform variant above coincided with an illegal-address fault in the fine
// decoder's kernel (both runs of tests/test_gpu_parity.py eval fine, r1k and r1l).
__device__ __forceinline__ void scatter_grid_grad_halves(float* __restrict__ grad, const int32_t* __restrict__ slot,
                                                         const Corners& cr, const f32x16& dc, bool valid,
                                                         const Scratch& S, int lane) {
  const int h = lane >> 5, ch = lane & 31;
  tstore(S.sA, dc, lane);
  stage_corners(cr, slot, valid, S, lane);
  lds_sync();
  float acc[8], wsum[8];
  int rows[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    acc[k] = 0.f;
    wsum[k] = 0.f;
    rows[k] = 0;
  }
  int cur = -1;
  for (int t = 0; t < 16; ++t) {
    const int pp = 16 * h + t;
    const int cell = S.ccell[pp];
    if (cell != cur) {
      if (cur >= 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (wsum[k] != 0.f) grid_add(grad + (size_t)rows[k] * NSLAM_C_DIM + ch, acc[k]);
      }
      cur = cell;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        acc[k] = 0.f;
        wsum[k] = 0.f;
        rows[k] = S.crow[pp * 8 + k];
      }
    }
    const float v = S.sA[pp * TPITCH + ch];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float w = S.cw[pp * 8 + k];
      acc[k] += w * v;
      wsum[k] += w;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (wsum[k] != 0.f) grid_add(grad + (size_t)rows[k] * NSLAM_C_DIM + ch, acc[k]);
  lds_sync();
}

__device__ __forceinline__ void coord_grad(const nslam_grid& g, const Corners& cr, const f32x16& dc, int lane,
                                           double gp[3]) {
  float part[3];
  coord_grad_partial(g.data, cr, dc, lane, part);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float gn = (part[k] + xor32(part[k])) * cr.gmul[k];
    gp[k] += ((double)gn * 2.0) / (g.hi[k] - g.lo[k]);
  }
}

}  // namespace nslamq
