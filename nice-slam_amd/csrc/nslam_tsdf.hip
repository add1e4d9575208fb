// nslam_tsdf.hip — block-sparse TSDF fusion of depth frames (the volume Mesher.get_bound_from_frames fuses,
// src/utils/Mesher.py:214-279; open3d's ScalableTSDFVolume restated, contract in include/nslam.h):
//   nslam_tsdf_block_range   the box of 16^3-voxel blocks the strided depth samples of K frames reach
//   nslam_tsdf_touch         per block of a dense table, the frames whose samples reach it (a uint32 bit mask)
//   nslam_tsdf_integrate     running-average update of the listed blocks, frames in ascending order
//   nslam_tsdf_mc_count/emit marching cubes over the allocated blocks, neighbours through the table
// Storage is a dense int32 block table over a caller-given box and a pool of blocks in structure-of-arrays
// form; no kernel allocates, every table and pool index is checked before it is used.  Atomics are integer
// min / max / add / or only, so every output is the same from run to run.  The build has -ffp-contract=off:
// the float32 arithmetic below rounds where include/nslam.h says it does.
#include <math.h>

#include "nslam_dev.h"
#include "nslam_mc_fan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kEdge = 16;          // voxels per block edge
constexpr int kVox = 4096;         // voxels per block
constexpr int kSlabs = 4;          // x-slabs (of 256 voxels) per integrate workgroup: 4 workgroups per block
constexpr int64_t kMaxCells = int64_t(1) << 27;
constexpr int32_t kMaxBlock = 1 << 26;  // |block index| bound: 16 * index + 15 fits an int32
constexpr double kClamp = 1073741824.0;  // 2^30: where a far-away sample's block index saturates

inline int64_t blocks_for(int64_t n) { return (n + kThreads - 1) / kThreads; }

struct Box {
  int32_t lo[3], n[3];
  __host__ __device__ int64_t cells() const { return (int64_t)n[0] * n[1] * n[2]; }
};

// the table box [lo, hi) of block indices: non-empty, at most 2^27 cells, indices within +-2^26
int make_box(Box& b, const int32_t* lo, const int32_t* hi) {
  if (!lo || !hi) return NSLAM_EINVAL;
  int64_t cells = 1;
  for (int c = 0; c < 3; ++c) {
    if (hi[c] <= lo[c] || lo[c] < -kMaxBlock || hi[c] > kMaxBlock) return NSLAM_EINVAL;
    const int64_t n = (int64_t)hi[c] - lo[c];
    cells *= n;
    if (cells > kMaxCells) return NSLAM_EINVAL;
    b.lo[c] = lo[c];
    b.n[c] = (int32_t)n;
  }
  return NSLAM_OK;
}

// ------------------------------------------------------------------------------------------------
// passes A and B: the strided depth samples
// ------------------------------------------------------------------------------------------------
struct SampleArgs {
  const float* depth;  // [K][H][W]
  const double* c2w;   // [K][16] row-major, +z forward
  int32_t K, H, W, stride, sh, sw;  // sh x sw samples per frame
  int64_t n;                        // K * sh * sw
  double fx, fy, cx, cy, trunc, B;
  float depth_trunc;
  Box box;
  int32_t* bounds;              // pass A: min x, y, z, max x, y, z
  unsigned long long* counter;  // pass A: valid samples; pass B: samples with a block outside the table
  uint32_t* mask;               // pass B: [cells]
};

__device__ __forceinline__ int32_t block_of(double q) {
  q = floor(q);
  q = q < -kClamp ? -kClamp : (q > kClamp ? kClamp : q);
  return (int32_t)q;
}

// sample i -> its frame and the block range of p -+ trunc per axis; false for an invalid depth (or a
// world point that is not finite)
__device__ __forceinline__ bool sample_blocks(const SampleArgs& a, int64_t i, int32_t& f, int32_t lo[3],
                                              int32_t hi[3]) {
  const int32_t su = (int32_t)(i % a.sw);
  const int64_t r = i / a.sw;
  const int32_t sv = (int32_t)(r % a.sh);
  f = (int32_t)(r / a.sh);
  const int32_t u = su * a.stride, v = sv * a.stride;
  const float d = a.depth[((int64_t)f * a.H + v) * a.W + u];
  if (!(d > 0.f && d <= a.depth_trunc)) return false;
  const double z = (double)d;
  const double x = (((double)u - a.cx) * z) / a.fx, y = (((double)v - a.cy) * z) / a.fy;
  const double* m = a.c2w + 16 * f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double p = ((m[4 * c] * x + m[4 * c + 1] * y) + m[4 * c + 2] * z) + m[4 * c + 3];
    if (!(fabs(p) <= 1.0e300)) return false;
    lo[c] = block_of((p - a.trunc) / a.B);
    hi[c] = block_of((p + a.trunc) / a.B);
  }
  return true;
}

__device__ __forceinline__ int32_t wave_min_i32(int32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

__global__ void k_tsdf_range_init(int32_t* bounds, unsigned long long* counter) {
  if (threadIdx.x < 3) bounds[threadIdx.x] = INT32_MAX;
  else if (threadIdx.x < 6) bounds[threadIdx.x] = INT32_MIN;
  else if (threadIdx.x == 6) *counter = 0ull;
}

__global__ __launch_bounds__(kThreads) void k_tsdf_range(SampleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t f, lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  const bool ok = i < a.n && sample_blocks(a, i, f, lo, hi);
  if (!ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = INT32_MAX, hi[c] = INT32_MIN;
  }
  const uint64_t live = __ballot(ok);
  if (live == 0) return;  // wave-uniform
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = wave_min_i32(lo[c]);
    hi[c] = wave_max_i32(hi[c]);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // thousands of waves share six words: look first (a stale value only costs an atomic it did not need)
      if (lo[c] < __atomic_load_n(a.bounds + c, __ATOMIC_RELAXED)) atomicMin(a.bounds + c, lo[c]);
      if (hi[c] > __atomic_load_n(a.bounds + 3 + c, __ATOMIC_RELAXED)) atomicMax(a.bounds + 3 + c, hi[c]);
    }
    atomicAdd(a.counter, (unsigned long long)__popcll(live));
  }
}

__global__ __launch_bounds__(kThreads) void k_tsdf_touch(SampleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t f = 0, lo[3], hi[3];
  bool outside = false;
  if (i < a.n && sample_blocks(a, i, f, lo, hi)) {
    const uint32_t bit = 1u << f;
    // 2 trunc <= B (checked by the entry point): at most two blocks per axis
    for (int32_t bx = lo[0]; bx <= hi[0]; ++bx)
      for (int32_t by = lo[1]; by <= hi[1]; ++by)
        for (int32_t bz = lo[2]; bz <= hi[2]; ++bz) {
          const int64_t ix = (int64_t)bx - a.box.lo[0], iy = (int64_t)by - a.box.lo[1], iz = (int64_t)bz - a.box.lo[2];
          if (ix < 0 || ix >= a.box.n[0] || iy < 0 || iy >= a.box.n[1] || iz < 0 || iz >= a.box.n[2]) {
            outside = true;
            continue;
          }
          uint32_t* w = a.mask + ((ix * a.box.n[1] + iy) * a.box.n[2] + iz);
          // most samples of a frame find their bit set already: look before the atomic
          if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & bit)) atomicOr(w, bit);
        }
  }
  const uint64_t out = __ballot(outside);
  if (out != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.counter, (unsigned long long)__popcll(out));
}

int sample_args(SampleArgs& a, const float* depth, const double* c2w, int32_t K, int32_t H, int32_t W, double fx,
                double fy, double cx, double cy, int32_t stride, float depth_trunc, double voxel, double trunc) {
  if (!depth || !c2w || K <= 0 || H <= 0 || W <= 0 || stride < 1) return NSLAM_EINVAL;
  if (!(voxel > 0.0) || !(trunc > 0.0) || !(2.0 * trunc <= 16.0 * voxel) || !(voxel <= 1.0e30)) return NSLAM_EINVAL;
  if (!(fx != 0.0) || !(fy != 0.0) || !(depth_trunc > 0.f)) return NSLAM_EINVAL;
  if ((int64_t)H * W >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  a.depth = depth;
  a.c2w = c2w;
  a.K = K;
  a.H = H;
  a.W = W;
  a.stride = stride;
  a.sh = (H + stride - 1) / stride;
  a.sw = (W + stride - 1) / stride;
  a.n = (int64_t)K * a.sh * a.sw;
  if (blocks_for(a.n) >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.trunc = trunc;
  a.B = 16.0 * voxel;
  a.depth_trunc = depth_trunc;
  return NSLAM_OK;
}

// ------------------------------------------------------------------------------------------------
// pass C: integrate
// ------------------------------------------------------------------------------------------------
struct FuseArgs {
  const float* depth;    // [K][H][W]
  const uint8_t* color;  // [K][H][W][3] or NULL
  const float* w2c;      // [K][16]
  int32_t K, H, W;
  float fx, fy, cx, cy, depth_trunc, trunc, inv_trunc;
  double L;
  Box box;
  const int32_t *key, *id;  // [n_list]: table cell and pool id of a touched block
  const uint32_t* mask;     // [n_list]: the frames that touched it
  int64_t n_list, n_pool;
  float *tsdf, *weight, *cpool;  // [n_pool][4096]; cpool: 3 planes, cstride floats apart, or NULL
  int64_t cstride;
};

// One workgroup = kSlabs x-slabs of one block: thread t holds voxels (x, y = t >> 4, z = t & 15) for kSlabs
// consecutive x, so the 64 lanes of a wave read and write 64 consecutive floats of the z-fastest storage.
// The frame loop is uniform over the workgroup (mask, matrices and intrinsics are scalar loads); the voxel
// state stays in registers across it.
__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(FuseArgs a) {
  const int64_t li = blockIdx.x / (kEdge / kSlabs);
  const int part = blockIdx.x % (kEdge / kSlabs);
  const int32_t id = a.id[li], key = a.key[li];
  uint32_t m = a.mask[li];
  if (a.K < 32) m &= (1u << a.K) - 1u;
  if (m == 0 || id < 0 || id >= a.n_pool || key < 0 || key >= a.box.cells()) return;
  m = __builtin_amdgcn_readfirstlane(m);
  const int32_t bz = key % a.box.n[2] + a.box.lo[2], by = (key / a.box.n[2]) % a.box.n[1] + a.box.lo[1];
  const int32_t bx = key / (a.box.n[2] * a.box.n[1]) + a.box.lo[0];
  const int t = threadIdx.x;
  const float py = (float)(((double)(by * kEdge + (t >> 4)) + 0.5) * a.L);
  const float pz = (float)(((double)(bz * kEdge + (t & 15)) + 0.5) * a.L);
  const bool col = a.cpool != nullptr && a.color != nullptr;
  float px[kSlabs], ts[kSlabs], w[kSlabs], c0[kSlabs], c1[kSlabs], c2[kSlabs];
  int64_t at[kSlabs];
#pragma unroll
  for (int j = 0; j < kSlabs; ++j) {
    const int lx = part * kSlabs + j;
    px[j] = (float)(((double)(bx * kEdge + lx) + 0.5) * a.L);
    at[j] = (int64_t)id * kVox + lx * 256 + t;
    ts[j] = a.tsdf[at[j]];
    w[j] = a.weight[at[j]];
    c0[j] = c1[j] = c2[j] = 0.f;
    if (col) {
      c0[j] = a.cpool[at[j]];
      c1[j] = a.cpool[a.cstride + at[j]];
      c2[j] = a.cpool[2 * a.cstride + at[j]];
    }
  }
  const float Wf = (float)a.W - 1e-4f, Hf = (float)a.H - 1e-4f;
  while (m) {
    const int f = __ffs(m) - 1;
    m &= m - 1u;
    const float* M = a.w2c + 16 * f;
    const float* dimg = a.depth + (int64_t)f * a.H * a.W;
    const uint8_t* cimg = col ? a.color + (int64_t)f * a.H * a.W * 3 : nullptr;
#pragma unroll
    for (int j = 0; j < kSlabs; ++j) {
      const float camx = ((M[0] * px[j] + M[1] * py) + M[2] * pz) + M[3];
      const float camy = ((M[4] * px[j] + M[5] * py) + M[6] * pz) + M[7];
      const float camz = ((M[8] * px[j] + M[9] * py) + M[10] * pz) + M[11];
      if (!(camz > 0.f)) continue;
      const float uf = ((camx * a.fx) / camz + a.cx) + 0.5f;
      const float vf = ((camy * a.fy) / camz + a.cy) + 0.5f;
      if (!(uf >= 1e-4f && uf < Wf && vf >= 1e-4f && vf < Hf)) continue;
      const int32_t u = (int32_t)uf, v = (int32_t)vf;  // 0 <= u < W, 0 <= v < H by the test above
      const float d = dimg[(int64_t)v * a.W + u];
      if (!(d > 0.f && d <= a.depth_trunc)) continue;
      const float xn = ((float)u - a.cx) / a.fx, yn = ((float)v - a.cy) / a.fy;
      const float len = sqrtf((xn * xn + yn * yn) + 1.0f);
      const float sdf = (d - camz) * len;
      if (!(sdf > -a.trunc)) continue;
      const float tv = fminf(1.0f, sdf * a.inv_trunc);
      const float w1 = w[j] + 1.0f;
      ts[j] = (ts[j] * w[j] + tv) / w1;
      if (col) {
        const uint8_t* px8 = cimg + ((int64_t)v * a.W + u) * 3;
        c0[j] = (c0[j] * w[j] + (float)px8[0]) / w1;
        c1[j] = (c1[j] * w[j] + (float)px8[1]) / w1;
        c2[j] = (c2[j] * w[j] + (float)px8[2]) / w1;
      }
      w[j] = w1;
    }
  }
#pragma unroll
  for (int j = 0; j < kSlabs; ++j) {
    a.tsdf[at[j]] = ts[j];
    a.weight[at[j]] = w[j];
    if (col) {
      a.cpool[at[j]] = c0[j];
      a.cpool[a.cstride + at[j]] = c1[j];
      a.cpool[2 * a.cstride + at[j]] = c2[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// pass D: marching cubes over the pool
// ------------------------------------------------------------------------------------------------
struct McArgs {
  const float *tsdf, *weight, *cpool;
  int64_t cstride, n_pool;
  const int32_t *pool_key, *table;
  Box box;
  double L;
  uint8_t *flags, *ntri;  // [n_pool * 4096][3], [n_pool * 4096]
  const int32_t *vert_off, *face_off;
  int64_t n_verts, n_faces;
  double* verts;
  uint8_t* colors;
  int32_t* faces;
};

struct Vox {
  int32_t id, ix, iy, iz;  // pool id, the block's table coordinates
  int32_t x, y, z;         // voxel in the block
};

// pool voxel p -> its block and local coordinates; false when the block's key is not a table cell
__device__ __forceinline__ bool vox_of(const McArgs& a, int64_t p, Vox& v) {
  v.id = (int32_t)(p >> 12);
  const int32_t l = (int32_t)(p & (kVox - 1));
  v.x = l >> 8;
  v.y = (l >> 4) & 15;
  v.z = l & 15;
  const int32_t key = a.pool_key[v.id];
  if (key < 0 || key >= a.box.cells()) return false;
  v.iz = key % a.box.n[2];
  v.iy = (key / a.box.n[2]) % a.box.n[1];
  v.ix = key / (a.box.n[2] * a.box.n[1]);
  return true;
}

// pool index of the voxel at local (x, y, z) of block v, each coordinate in 0..16: 16 is the first voxel of the
// neighbouring block, found through the table; -1 when that block lies outside the table or is not allocated
__device__ __forceinline__ int64_t voxel_at(const McArgs& a, const Vox& v, int32_t x, int32_t y, int32_t z) {
  if (((x | y | z) & kEdge) == 0) return (int64_t)v.id * kVox + ((x * kEdge + y) * kEdge + z);
  const int32_t ix = v.ix + (x >> 4), iy = v.iy + (y >> 4), iz = v.iz + (z >> 4);
  if (ix >= a.box.n[0] || iy >= a.box.n[1] || iz >= a.box.n[2]) return -1;
  const int32_t nid = a.table[((int64_t)ix * a.box.n[1] + iy) * a.box.n[2] + iz];
  if (nid < 0 || nid >= a.n_pool) return -1;
  return (int64_t)nid * kVox + (((x & 15) * kEdge + (y & 15)) * kEdge + (z & 15));
}

// the cell whose low corner is voxel v: its 8 corner voxels and its case; false when a corner is missing or
// has no weight
__device__ __forceinline__ bool cell_of(const McArgs& a, const Vox& v, int64_t q[8], int& cs) {
  cs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    q[k] = voxel_at(a, v, v.x + (k & 1), v.y + ((k >> 1) & 1), v.z + ((k >> 2) & 1));
    if (q[k] < 0 || !(a.weight[q[k]] > 0.f)) return false;
    cs |= (a.tsdf[q[k]] < 0.f) ? (1 << k) : 0;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void k_tsdf_mc_count(McArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.n_pool * kVox) return;
  Vox v;
  int64_t q[8];
  int cs;
  if (!vox_of(a, p, v) || !cell_of(a, v, q, cs)) {
    a.ntri[p] = 0;
    return;
  }
  a.ntri[p] = kMcNumTri[cs];
  if (cs == 0 || cs == 255) return;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int k0 = edge_owner(e), k1 = k0 | (1 << (e >> 2));
    // every valid cell around a crossing edge stores the same byte
    if (((cs >> k0) ^ (cs >> k1)) & 1) a.flags[3 * q[k0] + (e >> 2)] = 1;
  }
}

__global__ __launch_bounds__(kThreads) void k_tsdf_mc_emit(McArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.n_pool * kVox) return;
  Vox v;
  if (!vox_of(a, p, v)) return;
  const int32_t g[3] = {(v.ix + a.box.lo[0]) * kEdge + v.x, (v.iy + a.box.lo[1]) * kEdge + v.y,
                        (v.iz + a.box.lo[2]) * kEdge + v.z};
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    if (!a.flags[3 * p + ax]) continue;
    const int64_t q = voxel_at(a, v, v.x + (ax == 0), v.y + (ax == 1), v.z + (ax == 2));
    const int64_t vo = a.vert_off[3 * p + ax];
    if (q < 0 || vo < 0 || vo >= a.n_verts) continue;
    const float f0 = a.tsdf[p], f1 = a.tsdf[q];
    const float t = f0 / (f0 - f1);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      a.verts[3 * vo + c] = (((double)g[c] + 0.5) + (c == ax ? (double)t : 0.0)) * a.L;
    if (a.cpool && a.colors) {
      const float a0 = fabsf(f0), a1 = fabsf(f1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float cv = (a1 * a.cpool[c * a.cstride + p] + a0 * a.cpool[c * a.cstride + q]) / (a0 + a1);
        a.colors[3 * vo + c] = (uint8_t)fminf(255.f, fmaxf(0.f, floorf(cv + 0.5f)));
      }
    }
  }
  const int nt = a.ntri[p];
  if (nt == 0) return;
  int64_t q[8];
  int cs;
  if (!cell_of(a, v, q, cs)) return;
  const int64_t fo = a.face_off[p];
  const int rows = min(nt, (int)kMcNumTri[cs]);
  const McRow row = row_pack(cs);
  int tr = 0;
  while (tr < rows) {
    uint32_t loop;
    int n;
    const int next = row_loop(row, rows, tr, loop, n);
    const int apex = loop_apex(loop, n);
    for (int i = 1; i < n - 1; ++i) {
      const int64_t at = fo + tr + i - 1;
      if (fo < 0 || at >= a.n_faces) return;
      int32_t id[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int e = fan_edge(loop, n, apex, i, k);
        id[k] = a.vert_off[3 * q[edge_owner(e)] + (e >> 2)];
      }
      // the table winds toward the corners below the level; a TSDF's outside (free space) is above it
      int32_t* f = a.faces + 3 * at;
      f[0] = id[0];
      f[1] = id[2];
      f[2] = id[1];
    }
    tr = next;
  }
}

int mc_args(McArgs& a, const float* tsdf, const float* weight, const int32_t* pool_key, int64_t n_pool,
            const int32_t* table, const int32_t* lo, const int32_t* hi) {
  if (n_pool < 0) return NSLAM_EINVAL;
  const int rc = make_box(a.box, lo, hi);
  if (rc != NSLAM_OK) return rc;
  if (n_pool > 0 && (!tsdf || !weight || !pool_key || !table)) return NSLAM_EINVAL;
  if (3 * (int64_t)kVox * n_pool >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;  // int32 vertex ids
  a.tsdf = tsdf;
  a.weight = weight;
  a.pool_key = pool_key;
  a.table = table;
  a.n_pool = n_pool;
  return NSLAM_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C entry points (include/nslam.h)
// ------------------------------------------------------------------------------------------------
extern "C" int nslam_tsdf_block_range(const float* depth, const double* c2w, int32_t n_frames, int32_t H, int32_t W,
                                      double fx, double fy, double cx, double cy, int32_t stride, float depth_trunc,
                                      double voxel, double trunc, int32_t* bounds, int64_t* n_valid, void* stream) {
  SampleArgs a{};
  const int rc = sample_args(a, depth, c2w, n_frames, H, W, fx, fy, cx, cy, stride, depth_trunc, voxel, trunc);
  if (rc != NSLAM_OK) return rc;
  if (!bounds || !n_valid) return NSLAM_EINVAL;
  a.bounds = bounds;
  a.counter = reinterpret_cast<unsigned long long*>(n_valid);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_tsdf_range_init, dim3(1), dim3(64), 0, s, a.bounds, a.counter);
  hipLaunchKernelGGL(k_tsdf_range, dim3((unsigned)blocks_for(a.n)), dim3(kThreads), 0, s, a);
  return hip_status();
}

extern "C" int nslam_tsdf_touch(const float* depth, const double* c2w, int32_t n_frames, int32_t H, int32_t W,
                                double fx, double fy, double cx, double cy, int32_t stride, float depth_trunc,
                                double voxel, double trunc, const int32_t* block_lo, const int32_t* block_hi,
                                uint32_t* mask, int64_t* n_outside, void* stream) {
  SampleArgs a{};
  int rc = sample_args(a, depth, c2w, n_frames, H, W, fx, fy, cx, cy, stride, depth_trunc, voxel, trunc);
  if (rc != NSLAM_OK) return rc;
  if (n_frames > NSLAM_MAX_FRAMES || !mask || !n_outside) return NSLAM_EINVAL;
  rc = make_box(a.box, block_lo, block_hi);
  if (rc != NSLAM_OK) return rc;
  a.mask = mask;
  a.counter = reinterpret_cast<unsigned long long*>(n_outside);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(mask, 0, (size_t)a.box.cells() * 4, s) != hipSuccess ||
      hipMemsetAsync(n_outside, 0, 8, s) != hipSuccess)
    return NSLAM_EHIP - (int)hipGetLastError();
  hipLaunchKernelGGL(k_tsdf_touch, dim3((unsigned)blocks_for(a.n)), dim3(kThreads), 0, s, a);
  return hip_status();
}

extern "C" int nslam_tsdf_integrate(const float* depth, const uint8_t* color, const float* w2c, int32_t n_frames,
                                    int32_t H, int32_t W, float fx, float fy, float cx, float cy, float depth_trunc,
                                    double voxel, float trunc, const int32_t* block_lo, const int32_t* block_hi,
                                    const int32_t* list_key, const int32_t* list_id, const uint32_t* list_mask,
                                    int64_t n_list, int64_t n_pool, float* tsdf, float* weight, float* color_pool,
                                    int64_t color_stride, void* stream) {
  if (!depth || !w2c || n_frames <= 0 || n_frames > NSLAM_MAX_FRAMES || H <= 0 || W <= 0) return NSLAM_EINVAL;
  if (!(voxel > 0.0) || !(voxel <= 1.0e30) || !(trunc > 0.f) || !(depth_trunc > 0.f)) return NSLAM_EINVAL;
  if (!(fx != 0.f) || !(fy != 0.f) || n_list < 0 || n_pool < 0 || n_list > n_pool) return NSLAM_EINVAL;
  if (color_pool && (!color || color_stride < n_pool * kVox)) return NSLAM_EINVAL;
  FuseArgs a{};
  const int rc = make_box(a.box, block_lo, block_hi);
  if (rc != NSLAM_OK) return rc;
  if ((int64_t)H * W >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  if (3 * (int64_t)kVox * n_pool >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  if (n_list == 0) return NSLAM_OK;
  if (!list_key || !list_id || !list_mask || !tsdf || !weight) return NSLAM_EINVAL;
  a.depth = depth;
  a.color = color;
  a.w2c = w2c;
  a.K = n_frames;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.depth_trunc = depth_trunc;
  a.trunc = trunc;
  a.inv_trunc = 1.0f / trunc;
  a.L = voxel;
  a.key = list_key;
  a.id = list_id;
  a.mask = list_mask;
  a.n_list = n_list;
  a.n_pool = n_pool;
  a.tsdf = tsdf;
  a.weight = weight;
  a.cpool = color_pool;
  a.cstride = color_stride;
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)(n_list * (kEdge / kSlabs))), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_tsdf_mc_count(const float* tsdf, const float* weight, const int32_t* pool_key, int64_t n_pool,
                                   const int32_t* table, const int32_t* block_lo, const int32_t* block_hi,
                                   uint8_t* flags, uint8_t* ntri, void* stream) {
  McArgs a{};
  const int rc = mc_args(a, tsdf, weight, pool_key, n_pool, table, block_lo, block_hi);
  if (rc != NSLAM_OK) return rc;
  if (n_pool == 0) return NSLAM_OK;
  if (!flags || !ntri) return NSLAM_EINVAL;
  a.flags = flags;
  a.ntri = ntri;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(flags, 0, (size_t)n_pool * kVox * 3, s) != hipSuccess) return NSLAM_EHIP - (int)hipGetLastError();
  hipLaunchKernelGGL(k_tsdf_mc_count, dim3((unsigned)blocks_for(n_pool * kVox)), dim3(kThreads), 0, s, a);
  return hip_status();
}

extern "C" int nslam_tsdf_mc_emit(const float* tsdf, const float* weight, const float* color_pool, int64_t color_stride,
                                  const int32_t* pool_key, int64_t n_pool, const int32_t* table,
                                  const int32_t* block_lo, const int32_t* block_hi, double voxel, const uint8_t* flags,
                                  const uint8_t* ntri, const int32_t* vert_off, const int32_t* face_off,
                                  int64_t n_verts, int64_t n_faces, double* verts, uint8_t* colors, int32_t* faces,
                                  void* stream) {
  McArgs a{};
  const int rc = mc_args(a, tsdf, weight, pool_key, n_pool, table, block_lo, block_hi);
  if (rc != NSLAM_OK) return rc;
  if (!(voxel > 0.0) || n_verts < 0 || n_faces < 0) return NSLAM_EINVAL;
  if (color_pool && color_stride < n_pool * kVox) return NSLAM_EINVAL;
  if (n_pool == 0 || (n_verts == 0 && n_faces == 0)) return NSLAM_OK;
  if (!flags || !ntri || !vert_off || !face_off || !verts || !faces) return NSLAM_EINVAL;
  a.cpool = color_pool;
  a.cstride = color_stride;
  a.L = voxel;
  a.flags = const_cast<uint8_t*>(flags);
  a.ntri = const_cast<uint8_t*>(ntri);
  a.vert_off = vert_off;
  a.face_off = face_off;
  a.n_verts = n_verts;
  a.n_faces = n_faces;
  a.verts = verts;
  a.colors = colors;
  a.faces = faces;
  hipLaunchKernelGGL(k_tsdf_mc_emit, dim3((unsigned)blocks_for(n_pool * kVox)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}
