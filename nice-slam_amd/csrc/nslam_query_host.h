#pragma once
// nslam_query_host.h — the host side every translation unit of the fused point query shares: argument
// checks, workspace sizing, the slab plan of the parameter gradients, and the declarations of what one
// unit launches for another (the per-decoder backward launchers, k_color_wgrad, k_slab_reduce).  No
// device code.  Included by every query translation unit (the file map: nslam_query_core.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "nslam.h"

namespace nslamq {

struct QueryKArgs;  // nslam_query_core.h

constexpr int kWavesBwd = 4;     // waves per workgroup of the decoder backward kernels
constexpr int kMaxSlabs = 4096;  // WG == 2 above this many tiles

inline bool grid_ok(const nslam_grid& g) {
  // every axis <= 1024: the scatter packs a cell's coordinates into 10 bits each (Corners::cell)
  return g.data && g.dims[0] > 0 && g.dims[1] > 0 && g.dims[2] > 0 && g.dims[0] <= 1024 && g.dims[1] <= 1024 &&
         g.dims[2] <= 1024 && (((uintptr_t)g.data) & 15) == 0;
}

inline int check_cfg(const nslam_query_cfg* c, bool bwd) {
  if (!c || c->stage < 0 || c->stage > 3) return NSLAM_EINVAL;
  const int st = c->stage;
  bool need[4] = {st == NSLAM_STAGE_COARSE, st != NSLAM_STAGE_COARSE, st >= NSLAM_STAGE_FINE,
                  st == NSLAM_STAGE_COLOR};
  for (int d = 0; d < 4; ++d) {
    if (!need[d]) continue;
    if (!grid_ok(c->grid[d]) || !c->packed[d]) return NSLAM_EINVAL;
    if ((((uintptr_t)c->packed[d]) & 15) != 0) return NSLAM_EINVAL;
  }
  if (c->rays_o) {
    if (!c->rays_d || !c->z_vals || c->n_samples <= 0) return NSLAM_EINVAL;
  }
  // the h4 cotangent is read as float4 rows (add_gh4, k_color_wgrad): 16-byte aligned
  if (c->g_h4 && (((uintptr_t)c->g_h4) & 15) != 0) return NSLAM_EINVAL;
  return NSLAM_OK;
}

// The point arguments of an entry point (after check_cfg): a count that is not negative; for a non-empty
// call the points — pts, or the config's ray form — and the per-point rows it reads or writes (rows_ok:
// raw / g_raw is there; an entry point without such a buffer passes true); the ray form indexes points in
// 32 bits (load_point) and takes whole rays.  index32: so does this entry point in pts form (the
// live-point lists are int32).
inline int check_points(const nslam_query_cfg* cfg, const double* pts, int64_t n_pts, bool rows_ok,
                        bool index32 = false) {
  if (n_pts < 0 || (n_pts > 0 && ((!pts && !cfg->rays_o) || !rows_ok))) return NSLAM_EINVAL;
  if ((cfg->rays_o || index32) && n_pts >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  if (cfg->rays_o && n_pts % cfg->n_samples) return NSLAM_EINVAL;
  return NSLAM_OK;
}

inline bool stage_uses(int stage, int dec) {
  switch (stage) {
    case NSLAM_STAGE_COARSE: return dec == NSLAM_DEC_COARSE;
    case NSLAM_STAGE_MIDDLE: return dec == NSLAM_DEC_MIDDLE;
    case NSLAM_STAGE_FINE: return dec == NSLAM_DEC_MIDDLE || dec == NSLAM_DEC_FINE;
    default: return dec != NSLAM_DEC_COARSE;
  }
}

inline int acc_floats_of(const nslam_dec_grad& dg) { return (int)((dg.count + 3) & ~int64_t(3)); }

// ---- the colour decoder's weight gradients (k_color_wgrad, nslam_color_wgrad.hip) ----------------
// With the forward's activation tape and ReLU masks, the colour decoder's backward is two launches that
// need not wait for each other: the lean mask-only chain (grid gradient, d/dpts) and k_color_wgrad, a
// split-K reduction over tile chunks of every weight block (one 8-wave workgroup per chunk; each
// chunk's partial sums fill one slab), then k_slab_reduce over the chunks.  Workspace: the chunk slabs.
#ifndef NSLAM_CW_CHUNKS
#define NSLAM_CW_CHUNKS 256
#endif
constexpr int kCwTargetChunks = NSLAM_CW_CHUNKS;  // one workgroup per CU
struct CwPlan {
  int64_t chunk_tiles;
  int nchunks;
  size_t slab_bytes;
};
inline CwPlan cw_plan(const nslam_dec_grad& dg, int64_t n_pts) {
  CwPlan p;
  const int64_t tiles = (n_pts + 31) / 32;
  p.chunk_tiles = (tiles + kCwTargetChunks - 1) / kCwTargetChunks;
  p.nchunks = (int)((tiles + p.chunk_tiles - 1) / p.chunk_tiles);
  p.slab_bytes = (size_t)p.nchunks * acc_floats_of(dg) * sizeof(float);
  return p;
}
inline bool cw_tape_path(const nslam_query_cfg* c) { return c->act_tape != nullptr && c->saved_masks != nullptr; }
// k_color_wgrad + k_slab_reduce into a.c.dgrad[COLOR] (a.g_raw: the cotangent; ws: the chunk slabs)
int launch_color_wgrad(const QueryKArgs& a, float* ws, hipStream_t s);

// Slab cap: kMaxSlabs, or NSLAM_MAX_SLABS from the environment (tests use it to reach the
// multi-tile read-modify-write mode at small sizes).
inline int64_t max_slabs() {
  const char* e = getenv("NSLAM_MAX_SLABS");
  const long v = e ? strtol(e, nullptr, 10) : 0;
  return v > 0 ? v : kMaxSlabs;
}

// parameter-gradient slabs for a decoder: one per tile up to the cap, else one per launched wave
// (the cap rounded up to whole workgroups), each wave walking tiles with grid stride
inline int64_t n_slabs(int64_t tiles) {
  const int64_t cap = max_slabs();
  return tiles <= cap ? tiles : (cap + kWavesBwd - 1) / kWavesBwd * kWavesBwd;
}

// k_slab_reduce (nslam_query.hip): dg.base[j] += the sum over the slabs, in a fixed order.  WG == 1
// launches leave one folded slab per workgroup (stride kWavesBwd slabs); WG == 2, and k_color_wgrad's
// chunks, one per wave / chunk
int slab_reduce(const nslam_dec_grad& dg, float* slab, bool folded, int64_t nslab, int64_t blocks, int acc,
                hipStream_t s);

inline size_t dec_ws_bytes(const nslam_query_cfg* cfg, int dec, int64_t n_pts) {
  const nslam_dec_grad& dg = cfg->dgrad[dec];
  if (!dg.base || dg.count <= 0) return 0;
  if (dec == NSLAM_DEC_COLOR && cw_tape_path(cfg)) {
    return cw_plan(dg, n_pts).slab_bytes;
  }
  return (size_t)n_slabs((n_pts + 31) / 32) * acc_floats_of(dg) * sizeof(float);
}

inline size_t bwd_ws_bytes(const nslam_query_cfg* cfg, int64_t n_pts) {
  size_t need = 0;
  for (int d = 0; d < 4; ++d) {
    const size_t b = dec_ws_bytes(cfg, d, n_pts);
    need = b > need ? b : need;  // decoders run one after the other on the stream: one region
  }
  return need;
}

// One decoder's backward (nslam_query_bwd.h), instantiated in nslam_query_dec.hip, once per decoder
template <int DEC>
int dispatch_dec_bwd(const QueryKArgs& a, bool first, float* slab, hipStream_t s);
#ifndef NSLAM_QUERY_ONE_TU
extern template int dispatch_dec_bwd<NSLAM_DEC_COARSE>(const QueryKArgs&, bool, float*, hipStream_t);
extern template int dispatch_dec_bwd<NSLAM_DEC_MIDDLE>(const QueryKArgs&, bool, float*, hipStream_t);
extern template int dispatch_dec_bwd<NSLAM_DEC_FINE>(const QueryKArgs&, bool, float*, hipStream_t);
extern template int dispatch_dec_bwd<NSLAM_DEC_COLOR>(const QueryKArgs&, bool, float*, hipStream_t);
#endif

}  // namespace nslamq
