// nslam_mc_fan.h: how a row of nslam_mc_table.h becomes triangles.  Hand-written; shared by the dense extractor
// (nslam_mesh.hip, k_mc_emit) and the block-volume extractor (nslam_tsdf.hip, k_tsdf_mc_emit), so the two cannot
// drift apart.  The generated table stays as tools/gen_mc_table.py writes it.
//
// A row of the table is a fan per loop, from the loop's first vertex: (l0, l1, l2), (l0, l2, l3), ...
// With four crossings in a face of the cell that fan can put a diagonal, even a whole triangle, into the face,
// where the neighbouring cell's fan puts the same one: an edge of four faces, or two triangles on the same three
// vertices.  A vertex of a loop is a valid apex when all its fan diagonals cross the cell's interior, i.e. it
// shares no face of the cell with the vertices two or more steps away (every loop of every case has one).  Every
// loop is fanned from its valid apex with the lowest edge id: a diagonal then belongs to two triangles of its
// own cell and to no other.  Same loops, same triangle count, same winding; and because the choice does not
// depend on where the loop's listing starts or which way it runs, a case and its complement (the same loops,
// reversed) get the same triangles, reversed.
#pragma once
#include <stdint.h>

#include "nslam_mc_table.h"

// edge e = axis * 4 + (a + 2 b) of a cell: the corner that owns it (the offsets (a, b) fill the two other axes
// in ascending order)
__device__ __forceinline__ int edge_owner(int e) {
  const int ax = e >> 2, ea = e & 1, eb = (e >> 1) & 1;
  return ax == 0 ? (ea << 1) | (eb << 2) : ax == 1 ? ea | (eb << 2) : ea | (eb << 1);
}

// the two faces of the cell that edge e lies in, as bits axis * 2 + side
__device__ __forceinline__ int edge_faces(int e) {
  const int ax = e >> 2, o1 = ax == 0 ? 1 : 0, o2 = ax == 2 ? 1 : 2;
  return (1 << (o1 * 2 + (e & 1))) | (1 << (o2 * 2 + ((e >> 1) & 1)));
}

// A loop is held as up to eight 4-bit edge ids.
__device__ __forceinline__ int loop_at(uint32_t loop, int i) { return (loop >> (4 * i)) & 15; }

// The table row of case cs, 12 bits per triangle (three 4-bit edge ids, the -1 padding becomes 15): triangles
// 0 .. 4 in lo, the rest in hi.  The byte loads do not depend on one another, and the walk below stays in
// registers.
struct McRow {
  uint64_t lo;
  uint32_t hi;
};
static_assert(NSLAM_MC_MAX_TRI <= 7, "a packed row holds five triangles in lo and two in hi");

__device__ __forceinline__ McRow row_pack(int cs) {
  const signed char* T = kMcTri[cs];
  McRow r{0, 0};
#pragma unroll
  for (int i = 0; i < 3 * NSLAM_MC_MAX_TRI; ++i) {
    const uint32_t e = (uint32_t)T[i] & 15u;
    if (i < 15)
      r.lo |= (uint64_t)e << (4 * i);
    else
      r.hi |= e << (4 * (i - 15));
  }
  return r;
}

__device__ __forceinline__ uint32_t row_tri(const McRow& r, int t) {
  return (t < 5 ? (uint32_t)(r.lo >> (12 * t)) : r.hi >> (12 * (t - 5))) & 0xfffu;
}

// The loop whose fan starts at triangle tr of a packed row of `rows` triangles: its vertices and their number n;
// returns the row triangle at which the next loop starts.
__device__ __forceinline__ int row_loop(const McRow& r, int rows, int tr, uint32_t& loop, int& n) {
  loop = row_tri(r, tr);
  n = 3;
  int next = tr + 1;
  while (next < rows && n < 8) {
    const uint32_t t = row_tri(r, next);  // continues the fan: same first vertex, starts where the last one ended
    if ((t & 15u) != (loop & 15u) || ((t >> 4) & 15u) != ((loop >> (4 * (n - 1))) & 15u)) break;
    loop |= (t >> 8) << (4 * n);
    ++n;
    ++next;
  }
  return next;
}

// position in the loop of its valid apex with the lowest edge id
__device__ __forceinline__ int loop_apex(uint32_t loop, int n) {
  int best = 0, best_e = 16;
  for (int c = 0; c < n; ++c) {
    const int e = loop_at(loop, c);
    if (e >= best_e) continue;  // the table lists a loop from its lowest edge: mostly decided at c = 0
    bool good = true;
    for (int d = 2; d <= n - 2; ++d) {
      int j = c + d;
      j -= j >= n ? n : 0;
      good = good && (edge_faces(e) & edge_faces(loop_at(loop, j))) == 0;
    }
    if (good) best = c, best_e = e;
  }
  return best;
}

// vertex k (0, 1, 2) of the i-th triangle (1 <= i <= n - 2) of the loop's fan from `apex`, as an edge id
__device__ __forceinline__ int fan_edge(uint32_t loop, int n, int apex, int i, int k) {
  int j = apex + (k == 0 ? 0 : i + k - 1);
  j -= j >= n ? n : 0;
  return loop_at(loop, j);
}
