// nslam_eval.hip — the per-vertex, per-face and per-point work of the evaluation tools (src/tools/cull_mesh.py,
// src/tools/eval_recon.py):
//   nslam_frustum_seen        vertices inside any camera's viewing frustum (cull_mesh.py:47-71, check_proj)
//   nslam_views_see_any       the same test per view: does the view see any point of a cloud (eval_recon.py:176)
//   nslam_depth_l1            per-view mean |a - b| of two depth-image batches (eval_recon.py:206)
//   nslam_face_areas / nslam_sample_surface   area-weighted surface samples (replaces trimesh.sample.sample_surface)
//   nslam_nn_build / nslam_nn_query           exact float64 nearest neighbours on a uniform cell grid (replaces
//                                             scipy's cKDTree and open3d's correspondence search)
//   nslam_transform_points / nslam_kabsch_sums / nslam_kabsch_partials   the per-point half of point-to-point ICP
// Latency-bound elementwise work: one thread per vertex, sample or query, wave-uniform matrices and grid
// parameters, global_* loads (as_global), no atomics (the one exception in the evaluation module is the depth
// rasteriser's integer atomicMin, nslam_raster.hip: order-independent, so still the same from run to run).  The build has -ffp-contract=off: the float32 projection
// rounds where the reference's torch ops round and the float64 sampler where its numpy restatement rounds.
#include <math.h>

#include "nslam_dev.h"
#include "nslam_reduce.h"

namespace {

constexpr int kEvalThreads = 256;
constexpr int kKabschItems = 4;   // points per thread of k_kabsch_sums
constexpr int kKabschVals = 17;   // count, Σa, Σb, Σabᵀ, Σ|a-b|²
// relative slack on (r h)² in the ring stop rule: the cell index floor((p - lo) / h) is rounded, so a target in
// a cell r + 1 away differs by more than r h (1 - a few 2^-52 · cells per axis) along that axis, not quite r h
constexpr double kRingSlack = 1.0 - 0x1p-36;

inline int64_t blocks_for(int64_t n) { return (n + kEvalThreads - 1) / kEvalThreads; }

// ------------------------------------------------------------------------------------------------
// frustum
// ------------------------------------------------------------------------------------------------
struct SeenArgs {
  const double* verts;  // [n][3]
  const float* w2c;     // [K][16] row-major
  int64_t n;
  int32_t K, H, W;
  float fx, fy, cx, cy;
  uint8_t* seen;
};

// the sibling of nslam_mesh.hip's project() with cull_mesh.py's epsilon: cam = w2c . [p, 1] (four float32
// products summed left to right), x flipped, uv = K . cam, z = uv_z + 1e-5, uv /= z; seen: 0 <= -z, 0 < u < W,
// 0 < v < H
__device__ __forceinline__ bool frustum_test(const SeenArgs& a, gptr_t<float> m, float x, float y, float z) {
  const float cx_ = -(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
  const float cy_ = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  const float cz_ = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
  const float ux = a.fx * cx_ + a.cx * cz_;
  const float uy = a.fy * cy_ + a.cy * cz_;
  const float zz = cz_ + 1e-5f;
  const float u = ux / zz, v = uy / zz;
  return (0.f <= -zz) & (u < (float)a.W) & (u > 0.f) & (v < (float)a.H) & (v > 0.f);
}

__global__ __launch_bounds__(kEvalThreads) void k_frustum_seen(SeenArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  const bool live = i < a.n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const gptr_t<double> p = as_global(a.verts) + 3 * i;
    x = (float)p[0];
    y = (float)p[1];
    z = (float)p[2];
  }
  bool seen = false;
  for (int32_t k = 0; k < a.K; ++k) {
    if (__ballot(live && !seen) == 0) break;  // the whole wave is seen: nothing left to learn
    if (!live || seen) continue;
    seen = frustum_test(a, as_global(a.w2c) + 16 * k, x, y, z);  // k is wave-uniform: scalar loads
  }
  if (live) a.seen[i] = seen ? 1 : 0;
}

// check_proj with the roles swapped (eval_recon.py:62-88: many views, one cloud): any[view] = 1 when some point
// passes the view's frustum_test.  Grid (chunk of points, view); a wave with a hit stores one byte of 1 — every
// writer stores the same value, so the plain stores race benignly.  a.seen is [K] here and zeroed by the caller.
__global__ __launch_bounds__(kEvalThreads) void k_views_see_any(SeenArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  const int32_t view = blockIdx.y;  // wave-uniform: scalar loads of the matrix
  bool hit = false;
  if (i < a.n) {
    const gptr_t<double> p = as_global(a.verts) + 3 * i;
    hit = frustum_test(a, as_global(a.w2c) + 16 * (int64_t)view, (float)p[0], (float)p[1], (float)p[2]);
  }
  if (__ballot(hit) != 0 && (threadIdx.x & 63) == 0) a.seen[view] = 1;
}

// out[view] = mean |a - b| over the view's n_pix pixels in float64: every thread adds its pixels in order, the
// workgroup's sum is nslam_reduce.h's — the same sum every run
__global__ __launch_bounds__(kEvalThreads) void k_depth_l1(const float* a, const float* b, int64_t n_pix, double* out) {
  __shared__ double part[kEvalThreads / 64][1];
  const gptr_t<float> ga = as_global(a) + (int64_t)blockIdx.x * n_pix, gb = as_global(b) + (int64_t)blockIdx.x * n_pix;
  double s[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n_pix; i += kEvalThreads) s[0] += fabs((double)ga[i] - (double)gb[i]);
  const double t = group_sum<kEvalThreads>(s, part);
  if (threadIdx.x == 0) out[blockIdx.x] = t / (double)n_pix;
}

// ------------------------------------------------------------------------------------------------
// surface sampling
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser (as nslam_mapping.hip's draws)
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// uniform k of sample i in [0, 1): the top 53 bits of the counter-based stream (seed, sample, k)
__device__ __forceinline__ double uniform53(uint64_t seed, int64_t i, int k) {
  const uint64_t bits = mix64(seed ^ mix64((uint64_t)i * 0x9e3779b97f4a7c15ull + (uint64_t)k));
  return (double)(bits >> 11) * 0x1p-53;
}

__global__ __launch_bounds__(kEvalThreads) void k_face_areas(const double* verts, const int32_t* faces, int64_t nf,
                                                             double* area) {
  const int64_t f = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (f >= nf) return;
  const gptr_t<int32_t> t = as_global(faces) + 3 * f;
  const gptr_t<double> p = as_global(verts) + 3 * (int64_t)t[0], q = as_global(verts) + 3 * (int64_t)t[1],
                       r = as_global(verts) + 3 * (int64_t)t[2];
  const double ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
  const double vx = r[0] - p[0], vy = r[1] - p[1], vz = r[2] - p[2];
  const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
  area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

__global__ __launch_bounds__(kEvalThreads) void k_sample_surface(const double* verts, const int32_t* faces,
                                                                 const double* cdf, int64_t nf, int64_t count,
                                                                 uint64_t seed, double* points, int32_t* face_id) {
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (i >= count) return;
  const gptr_t<double> c = as_global(cdf);
  const double total = c[nf - 1];
  double* o = points + 3 * i;
  if (!(total > 0.0) || !(total < INFINITY)) {  // no area to draw from
    face_id[i] = -1;
    o[0] = o[1] = o[2] = NAN;
    return;
  }
  const double u0 = uniform53(seed, i, 0);
  double u1 = uniform53(seed, i, 1), u2 = uniform53(seed, i, 2);
  // the first f with cdf[f] > t (t < total, so there is one; a zero-area face repeats its predecessor's cdf
  // and is never the first)
  const double t = u0 * total;
  int64_t lo = 0, hi = nf - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (u1 + u2 > 1.0) {  // trimesh's reflection into the triangle
    u1 = 1.0 - u1;
    u2 = 1.0 - u2;
  }
  const gptr_t<int32_t> tr = as_global(faces) + 3 * lo;
  const gptr_t<double> p = as_global(verts) + 3 * (int64_t)tr[0], q = as_global(verts) + 3 * (int64_t)tr[1],
                       r = as_global(verts) + 3 * (int64_t)tr[2];
#pragma unroll
  for (int d = 0; d < 3; ++d) o[d] = (p[d] + u1 * (q[d] - p[d])) + u2 * (r[d] - p[d]);
  face_id[i] = (int32_t)lo;
}

// ------------------------------------------------------------------------------------------------
// nearest neighbours on a uniform cell grid
// ------------------------------------------------------------------------------------------------
struct NnGrid {
  double lo[3];
  double h;
  int32_t dims[3];
};

__device__ __forceinline__ int32_t cell_of(const NnGrid& g, double p, int ax) {
  const double c = floor((p - g.lo[ax]) / g.h);
  // clamped in double: a query far outside the box does not fit an int
  return !(c > 0.0) ? 0 : (c >=(double)(g.dims[ax] - 1) ? g.dims[ax] - 1 : (int32_t)c);
}

__global__ __launch_bounds__(kEvalThreads) void k_nn_keys(const double* targets, int64_t m, NnGrid g,
                                                          int32_t* keys) {
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (i >= m) return;
  const gptr_t<double> p = as_global(targets) + 3 * i;
  const int32_t cx = cell_of(g, p[0], 0), cy = cell_of(g, p[1], 1), cz = cell_of(g, p[2], 2);
  keys[i] = (cx * g.dims[1] + cy) * g.dims[2] + cz;
}

struct NnArgs {
  const double* queries;    // [n][3]
  const double* targets;    // [m][3] sorted by cell key (stable: ascending original index inside a cell)
  const int32_t* orig;      // [m] original index of each sorted target
  const int32_t* start;     // [cells + 1] first sorted target of each cell
  int64_t n;
  NnGrid g;
  double max_dist;          // < 0: none
  double* dist;
  int32_t* idx;
};

__global__ __launch_bounds__(kEvalThreads) void k_nn_query(NnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (i >= a.n) return;
  const gptr_t<double> q = as_global(a.queries) + 3 * i;
  const gptr_t<double> tg = as_global(a.targets);
  const gptr_t<int32_t> og = as_global(a.orig), st = as_global(a.start);
  const double qx = q[0], qy = q[1], qz = q[2];
  const int32_t dx = a.g.dims[0], dy = a.g.dims[1], dz = a.g.dims[2];
  const int32_t cx = cell_of(a.g, qx, 0), cy = cell_of(a.g, qy, 1), cz = cell_of(a.g, qz, 2);
  double best = INFINITY;  // squared
  int32_t best_i = -1;
  // one run of sorted targets (the cells (x, y, z0..z1) are consecutive keys, hence consecutive targets)
  auto scan = [&](int32_t x, int32_t y, int32_t z0, int32_t z1) {
    const int32_t row = (x * dy + y) * dz;
    const int32_t b = st[row + z0], e = st[row + z1 + 1];
    for (int32_t j = b; j < e; ++j) {
      const double ex = tg[3 * (int64_t)j] - qx, ey = tg[3 * (int64_t)j + 1] - qy, ez = tg[3 * (int64_t)j + 2] - qz;
      const double d2 = (ex * ex + ey * ey) + ez * ez;
      if (d2 <= best) {  // ties go to the lowest original index
        const int32_t o = og[j];
        if (d2 < best || o < best_i) {
          best = d2;
          best_i = o;
        }
      }
    }
  };
  for (int32_t r = 0;; ++r) {
    const int32_t x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1);
    const int32_t y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
    const int32_t z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1);
    for (int32_t x = x0; x <= x1; ++x) {
      const bool xs = (x == cx - r) | (x == cx + r);
      for (int32_t y = y0; y <= y1; ++y) {
        if (xs || y == cy - r || y == cy + r) {
          scan(x, y, z0, z1);  // on the shell in x or y: the whole z run
        } else {               // inside in x and y: the two z caps (r > 0 here)
          if (cz - r >= 0) scan(x, y, cz - r, cz - r);
          if (cz + r < dz) scan(x, y, cz + r, cz + r);
        }
      }
    }
    // every target in a cell beyond ring r differs from the query by more than r h along some axis
    const double rh = (double)r * a.g.h;
    if (best <= rh * rh * kRingSlack) break;
    if (a.max_dist >= 0.0 && rh * kRingSlack >= a.max_dist) break;
    if (cx - r <= 0 && cx + r >= dx - 1 && cy - r <= 0 && cy + r >= dy - 1 && cz - r <= 0 && cz + r >= dz - 1) break;
  }
  double d = sqrt(best);
  if (a.max_dist >= 0.0 && !(d <= a.max_dist)) {
    d = INFINITY;
    best_i = -1;
  }
  a.dist[i] = d;
  a.idx[i] = best_i;
}

// ------------------------------------------------------------------------------------------------
// ICP: rigid transform and the Kabsch sums
// ------------------------------------------------------------------------------------------------
struct Rigid {
  double m[12];  // [3][4] row-major
};

__global__ __launch_bounds__(kEvalThreads) void k_transform(const double* pts, int64_t n, Rigid t, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (i >= n) return;
  const gptr_t<double> p = as_global(pts) + 3 * i;
  const double x = p[0], y = p[1], z = p[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) out[3 * i + r] = ((t.m[4 * r] * x + t.m[4 * r + 1] * y) + t.m[4 * r + 2] * z) + t.m[4 * r + 3];
}

// partials[wg][17] over the workgroup's kKabschItems * 256 points with idx >= 0: every thread adds its points
// in order, the workgroup's sums are nslam_reduce.h's — the same sums every run
__global__ __launch_bounds__(kEvalThreads) void k_kabsch_sums(const double* src, const int32_t* idx, int64_t n,
                                                              const double* targets, int64_t m,
                                                              double* partials) {
  __shared__ double part[kEvalThreads / 64][kKabschVals];
  double s[kKabschVals];
#pragma unroll
  for (int v = 0; v < kKabschVals; ++v) s[v] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * (kEvalThreads * kKabschItems);
#pragma unroll
  for (int k = 0; k < kKabschItems; ++k) {
    const int64_t i = base + (int64_t)k * kEvalThreads + threadIdx.x;
    if (i >= n) continue;
    const int32_t j = as_global(idx)[i];
    if (j < 0 || j >= m) continue;
    const gptr_t<double> pa = as_global(src) + 3 * i, pb = as_global(targets) + 3 * (int64_t)j;
    const double a[3] = {pa[0], pa[1], pa[2]}, b[3] = {pb[0], pb[1], pb[2]};
    s[0] += 1.0;
    double e2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      s[1 + r] += a[r];
      s[4 + r] += b[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) s[7 + 3 * r + c] += a[r] * b[c];
      const double d = a[r] - b[r];
      e2 += d * d;
    }
    s[16] += e2;
  }
  const double t = group_sum<kEvalThreads>(s, part);
  if (threadIdx.x < kKabschVals) partials[(int64_t)blockIdx.x * kKabschVals + threadIdx.x] = t;
}

inline bool finite_d(double v) { return v == v && v - v == 0.0; }

// the grid description every nn entry point takes (host pointers); cells = its cell count
int nn_grid(NnGrid& g, int64_t& cells, const double* lo, double cell, const int32_t* dims) {
  if (!lo || !dims || !finite_d(cell) || !(cell > 0.0)) return NSLAM_EINVAL;
  cells = 1;
  for (int c = 0; c < 3; ++c) {
    if (!finite_d(lo[c]) || dims[c] < 1) return NSLAM_EINVAL;
    g.lo[c] = lo[c];
    g.dims[c] = dims[c];
    cells *= dims[c];
    if (cells > (int64_t(1) << 24)) return NSLAM_EINVAL;
  }
  g.h = cell;
  return NSLAM_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C entry points (include/nslam.h)
// ------------------------------------------------------------------------------------------------
extern "C" int nslam_frustum_seen(const double* verts, int64_t n, const float* w2c, int32_t n_frames, int32_t H,
                                  int32_t W, float fx, float fy, float cx, float cy, uint8_t* seen, void* stream) {
  if (n < 0 || n_frames < 0 || H <= 0 || W <= 0) return NSLAM_EINVAL;
  if (n == 0) return NSLAM_OK;
  if (!verts || !seen || (n_frames > 0 && !w2c)) return NSLAM_EINVAL;
  if (blocks_for(n) >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  SeenArgs a{};
  a.verts = verts;
  a.w2c = w2c;
  a.n = n;
  a.K = n_frames;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.seen = seen;
  hipLaunchKernelGGL(k_frustum_seen, dim3((unsigned)blocks_for(n)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_views_see_any(const double* pts, int64_t n, const float* w2c, int32_t n_views, int32_t H,
                                   int32_t W, float fx, float fy, float cx, float cy, uint8_t* any, void* stream) {
  if (n < 0 || n_views < 0 || H <= 0 || W <= 0) return NSLAM_EINVAL;
  if (n == 0 || n_views == 0) return NSLAM_OK;  // nothing can be seen: `any` stays as the caller zeroed it
  if (!pts || !w2c || !any) return NSLAM_EINVAL;
  if (blocks_for(n) >= (int64_t(1) << 31) || n_views > 65535) return NSLAM_EUNSUPPORTED;
  SeenArgs a{};
  a.verts = pts;
  a.w2c = w2c;
  a.n = n;
  a.K = n_views;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.seen = any;
  hipLaunchKernelGGL(k_views_see_any, dim3((unsigned)blocks_for(n), (unsigned)n_views), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_depth_l1(const float* a, const float* b, int64_t n_views, int64_t n_pix, double* out,
                              void* stream) {
  if (n_views < 0 || n_pix < 0) return NSLAM_EINVAL;
  if (n_views == 0) return NSLAM_OK;
  if (n_pix == 0 || !a || !b || !out) return NSLAM_EINVAL;  // the mean of no pixels
  if (n_views >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_depth_l1, dim3((unsigned)n_views), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a, b, n_pix, out);
  return hip_status();
}

extern "C" int nslam_face_areas(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                double* area, void* stream) {
  if (n_faces < 0 || n_verts < 0 || n_verts >= (int64_t(1) << 31) || n_faces >= (int64_t(1) << 31))
    return NSLAM_EINVAL;
  if (n_faces == 0) return NSLAM_OK;
  if (!verts || !faces || !area || n_verts == 0) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_face_areas, dim3((unsigned)blocks_for(n_faces)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), verts, faces, n_faces, area);
  return hip_status();
}

extern "C" int nslam_sample_surface(const double* verts, int64_t n_verts, const int32_t* faces, const double* cdf,
                                    int64_t n_faces, int64_t count, uint64_t seed, double* points, int32_t* face_id,
                                    void* stream) {
  if (count < 0 || n_faces < 0 || n_verts < 0 || n_faces >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  if (count == 0) return NSLAM_OK;
  if (n_faces == 0 || n_verts == 0 || !verts || !faces || !cdf || !points || !face_id) return NSLAM_EINVAL;
  if (blocks_for(count) >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_sample_surface, dim3((unsigned)blocks_for(count)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), verts, faces, cdf, n_faces, count, seed, points, face_id);
  return hip_status();
}

extern "C" int nslam_nn_build(const double* targets, int64_t m, const double* lo, double cell, const int32_t* dims,
                              int32_t* keys, void* stream) {
  NnGrid g{};
  int64_t cells = 0;
  if (m <= 0 || m >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  const int rc = nn_grid(g, cells, lo, cell, dims);
  if (rc != NSLAM_OK) return rc;
  if (!targets || !keys) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_nn_keys, dim3((unsigned)blocks_for(m)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), targets, m, g, keys);
  return hip_status();
}

extern "C" int nslam_nn_query(const double* queries, int64_t n, const double* sorted_targets,
                              const int32_t* orig_idx, int64_t m, const int32_t* cell_start, int64_t n_cell_start,
                              const double* lo, double cell, const int32_t* dims, double max_dist, double* dist,
                              int32_t* idx, void* stream) {
  NnGrid g{};
  int64_t cells = 0;
  if (n < 0 || m <= 0 || m >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  const int rc = nn_grid(g, cells, lo, cell, dims);
  if (rc != NSLAM_OK) return rc;
  if (n_cell_start != cells + 1) return NSLAM_EINVAL;  // the offsets belong to another grid
  if (max_dist != max_dist) return NSLAM_EINVAL;
  if (n == 0) return NSLAM_OK;
  if (!queries || !sorted_targets || !orig_idx || !cell_start || !dist || !idx) return NSLAM_EINVAL;
  if (blocks_for(n) >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  NnArgs a{};
  a.queries = queries;
  a.targets = sorted_targets;
  a.orig = orig_idx;
  a.start = cell_start;
  a.n = n;
  a.g = g;
  a.max_dist = (max_dist < 0.0 || max_dist == INFINITY) ? -1.0 : max_dist;
  a.dist = dist;
  a.idx = idx;
  hipLaunchKernelGGL(k_nn_query, dim3((unsigned)blocks_for(n)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_transform_points(const double* pts, int64_t n, const double* rigid, double* out, void* stream) {
  if (n < 0 || !rigid) return NSLAM_EINVAL;
  Rigid t;
  for (int k = 0; k < 12; ++k) {
    if (!finite_d(rigid[k])) return NSLAM_EINVAL;
    t.m[k] = rigid[k];
  }
  if (n == 0) return NSLAM_OK;
  if (!pts || !out) return NSLAM_EINVAL;
  if (blocks_for(n) >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_transform, dim3((unsigned)blocks_for(n)), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), pts, n, t, out);
  return hip_status();
}

extern "C" int64_t nslam_kabsch_partials(int64_t n) {
  if (n <= 0) return 0;
  const int64_t per = (int64_t)kEvalThreads * kKabschItems;
  return (n + per - 1) / per;
}

extern "C" int nslam_kabsch_sums(const double* src, const int32_t* idx, int64_t n, const double* targets, int64_t m,
                                 double* partials, int64_t n_partials, void* stream) {
  if (n < 0 || m <= 0 || m >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  if (n_partials != nslam_kabsch_partials(n)) return NSLAM_EINVAL;
  if (n == 0) return NSLAM_OK;
  if (!src || !idx || !targets || !partials) return NSLAM_EINVAL;
  if (n_partials >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_kabsch_sums, dim3((unsigned)n_partials), dim3(kEvalThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), src, idx, n, targets, m, partials);
  return hip_status();
}
