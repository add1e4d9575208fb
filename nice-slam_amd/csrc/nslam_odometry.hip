// nslam_odometry.hip — depth odometry against the TSDF volume of nslam_tsdf.hip (KinectFusion's two steps;
// contract in include/nslam.h):
//   nslam_depth_maps     depth image -> camera-frame vertex and normal maps
//   nslam_tsdf_raycast   the volume seen from a pose -> world-space vertex and normal maps
//   nslam_icp_sums       projective point-to-plane association and the 29 sums of the normal equations
//   nslam_gray_pyramid   colour image -> grey levels, each the 3 x 3 binomial of the one below at every second pixel
//   nslam_photo_sums     the 29 sums of the photometric residual against a reference frame's grey level
// One stream, no graph capture, no float atomics: every output is the same from run to run (the 29 sums are
// added in nslam_reduce.h's order).  Every table, pool and image index is checked before use and every loop has
// a fixed trip-count cap; a pose or a value that is not finite ends as an invalid pixel.  The build has
// -ffp-contract=off: the arithmetic below rounds where include/nslam.h says it does.
#include <math.h>

#include "nslam_dev.h"
#include "nslam_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVox = 4096;
constexpr int kMaxSteps = 4096;       // lattice samples of a ray: the march's trip-count cap
constexpr int kMaxGroups = 1024;      // workgroups (rows of partials) of an icp_sums call
constexpr int kSums = 29;
constexpr int64_t kMaxCells = int64_t(1) << 27;
constexpr int32_t kMaxBlock = 1 << 26;

inline int64_t blocks_for(int64_t n) { return (n + kThreads - 1) / kThreads; }

__device__ __forceinline__ float qnan() { return __uint_as_float(0x7fc00000u); }

// ------------------------------------------------------------------------------------------------
// depth maps
// ------------------------------------------------------------------------------------------------
struct MapArgs {
  const float* depth;
  int32_t H, W;
  float fx, fy, cx, cy, depth_trunc, max_jump;
  float *vertex, *normal;
};

__device__ __forceinline__ bool depth_ok(float d, float trunc) { return d > 0.f && d <= trunc; }

__global__ __launch_bounds__(kThreads) void k_depth_maps(MapArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)a.H * a.W) return;
  const int32_t u = (int32_t)(i % a.W), v = (int32_t)(i / a.W);
  const float nan = qnan();
  const float d = a.depth[i];
  const bool ok = depth_ok(d, a.depth_trunc);
  const float xn = ((float)u - a.cx) / a.fx, yn = ((float)v - a.cy) / a.fy;
  const float px = xn * d, py = yn * d;
  a.vertex[3 * i + 0] = ok ? px : nan;
  a.vertex[3 * i + 1] = ok ? py : nan;
  a.vertex[3 * i + 2] = ok ? d : nan;
  float nx = nan, ny = nan, nz = nan;
  if (ok && u + 1 < a.W && v + 1 < a.H) {
    const float dr = a.depth[i + 1], dd = a.depth[i + a.W];
    if (depth_ok(dr, a.depth_trunc) && depth_ok(dd, a.depth_trunc) && !(fabsf(dr - d) > a.max_jump) &&
        !(fabsf(dd - d) > a.max_jump)) {
      const float xr = ((float)(u + 1) - a.cx) / a.fx, yd = ((float)(v + 1) - a.cy) / a.fy;
      const float ax = xr * dr - px, ay = yn * dr - py, az = dr - d;   // to pixel (u + 1, v)
      const float bx = xn * dd - px, by = yd * dd - py, bz = dd - d;   // to pixel (u, v + 1)
      const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
      if (len > 0.f && len <= 3.0e38f) {
        nx = cx / len, ny = cy / len, nz = cz / len;
        if ((nx * px + ny * py) + nz * d > 0.f) nx = -nx, ny = -ny, nz = -nz;
      }
    }
  }
  a.normal[3 * i + 0] = nx;
  a.normal[3 * i + 1] = ny;
  a.normal[3 * i + 2] = nz;
}

// ------------------------------------------------------------------------------------------------
// ray cast
// ------------------------------------------------------------------------------------------------
struct CastArgs {
  const int32_t *table, *pool_key;
  const float *tsdf, *weight;
  int64_t n_pool;
  int32_t lo[3], n[3];
  int32_t H, W;
  float m[12];  // c2w rows 0..2, rounded to float32
  float fx, fy, cx, cy, near, far, L, B, step;
  float *vertex, *normal;
};

// pool index of global voxel (x, y, z); -1 outside the table, in an unallocated block or a block whose pool id
// or key is out of range
__device__ __forceinline__ int64_t voxel_index(const CastArgs& a, int32_t x, int32_t y, int32_t z) {
  const int32_t ix = (x >> 4) - a.lo[0], iy = (y >> 4) - a.lo[1], iz = (z >> 4) - a.lo[2];
  if (ix < 0 || ix >= a.n[0] || iy < 0 || iy >= a.n[1] || iz < 0 || iz >= a.n[2]) return -1;
  const int32_t id = a.table[((int64_t)ix * a.n[1] + iy) * a.n[2] + iz];
  if (id < 0 || id >= a.n_pool) return -1;
  return (int64_t)id * kVox + (((x & 15) * 16 + (y & 15)) * 16 + (z & 15));
}

// the trilinear field at p: false unless all 8 voxel centres around p are allocated and weighted
__device__ __forceinline__ bool field(const CastArgs& a, float px, float py, float pz, float& f) {
  const float gx = px / a.L - 0.5f, gy = py / a.L - 0.5f, gz = pz / a.L - 0.5f;
  if (!(fabsf(gx) < 1.0e9f && fabsf(gy) < 1.0e9f && fabsf(gz) < 1.0e9f)) return false;
  const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
  const float tx = gx - x0, ty = gy - y0, tz = gz - z0;
  const int32_t ix = (int32_t)x0, iy = (int32_t)y0, iz = (int32_t)z0;
  float c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t q = voxel_index(a, ix + (k >> 2), iy + ((k >> 1) & 1), iz + (k & 1));
    if (q < 0 || !(a.weight[q] > 0.f)) return false;
    c[k] = a.tsdf[q];
  }
  // along x, then y, then z; corner k = dx * 4 + dy * 2 + dz
  const float c00 = c[0] + tx * (c[4] - c[0]), c01 = c[1] + tx * (c[5] - c[1]);
  const float c10 = c[2] + tx * (c[6] - c[2]), c11 = c[3] + tx * (c[7] - c[3]);
  const float c0 = c00 + ty * (c10 - c00), c1 = c01 + ty * (c11 - c01);
  f = c0 + tz * (c1 - c0);
  return true;
}

__device__ __forceinline__ int32_t block_of_f(float q) {
  q = floorf(q);
  q = q < -1073741824.f ? -1073741824.f : (q > 1073741824.f ? 1073741824.f : q);
  return (int32_t)q;
}

__global__ __launch_bounds__(kThreads) void k_tsdf_raycast(CastArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)a.H * a.W) return;
  const int32_t u = (int32_t)(i % a.W), v = (int32_t)(i / a.W);
  const float nan = qnan();
  float out[6] = {nan, nan, nan, nan, nan, nan};
  const float xn = ((float)u - a.cx) / a.fx, yn = ((float)v - a.cy) / a.fy;
  float d[3], o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[c] = (a.m[4 * c] * xn + a.m[4 * c + 1] * yn) + a.m[4 * c + 2];
    o[c] = a.m[4 * c + 3];
  }
  const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = d[c] / len;

  // samples lie on the lattice t_k = near + k * step; last: sign of the last valid non-zero sample
  int k = 0, last = 0;
  bool adj = false, hit = false;
  float tp = 0.f, fp = 0.f, tc = 0.f, fc = 0.f;
  for (int it = 0; it < kMaxSteps && k < kMaxSteps; ++it) {
    const float t = a.near + (float)k * a.step;
    if (!(t <= a.far)) break;
    const float p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    if (!(fabsf(p[0]) <= 1.0e30f && fabsf(p[1]) <= 1.0e30f && fabsf(p[2]) <= 1.0e30f)) break;
    const int32_t b[3] = {block_of_f(p[0] / a.B), block_of_f(p[1] / a.B), block_of_f(p[2] / a.B)};
    const int32_t ix = b[0] - a.lo[0], iy = b[1] - a.lo[1], iz = b[2] - a.lo[2];
    int32_t id = -1;
    if (ix >= 0 && ix < a.n[0] && iy >= 0 && iy < a.n[1] && iz >= 0 && iz < a.n[2])
      id = a.table[((int64_t)ix * a.n[1] + iy) * a.n[2] + iz];
    const bool empty = id < 0 || id >= a.n_pool;
    float f = 0.f;
    if (empty || !field(a, p[0], p[1], p[2], f)) {
      // right after a valid positive sample the step may have crossed the whole band behind a surface: one
      // sample midway
      if (adj && fp > 0.f) {
        const float tm = a.near + ((float)k - 0.5f) * a.step;
        float fm;
        if (field(a, o[0] + tm * d[0], o[1] + tm * d[1], o[2] + tm * d[2], fm) && fm < 0.f) {
          hit = true;
          tc = tm, fc = fm;
          break;
        }
      }
      adj = false;
      int kn = k + 1;
      if (empty) {
        // an empty block: on to the first lattice sample at or past its exit face
        float te = 3.0e38f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (d[c] > 0.f) te = fminf(te, ((float)(b[c] + 1) * a.B - o[c]) / d[c]);
          else if (d[c] < 0.f) te = fminf(te, ((float)b[c] * a.B - o[c]) / d[c]);
        }
        const float kf = ceilf((te - a.near) / a.step);
        if (kf > (float)kn) kn = kf < (float)kMaxSteps ? (int)kf : kMaxSteps;
      }
      k = kn;
      continue;
    }
    if (f < 0.f && last > 0) {
      hit = adj;  // a valid positive sample right before: a front face; a gap in between: no hit
      tc = t, fc = f;
      break;
    }
    if (f > 0.f && last < 0) break;  // a back face
    if (f > 0.f) last = 1;
    if (f < 0.f) last = -1;
    adj = true;
    tp = t, fp = f;
    ++k;
  }
  if (hit) {
    float ts = tp + (tc - tp) * (fp / (fp - fc));
    float fs;
    if (field(a, o[0] + ts * d[0], o[1] + ts * d[1], o[2] + ts * d[2], fs)) {
      if (fs > 0.f) ts = ts + (tc - ts) * (fs / (fs - fc));
      else if (fs < 0.f) ts = tp + (ts - tp) * (fp / (fp - fs));
    }
    const float p[3] = {o[0] + ts * d[0], o[1] + ts * d[1], o[2] + ts * d[2]};
    float g[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float fa, fb;
      ok = ok && field(a, p[0] + (c == 0 ? a.L : 0.f), p[1] + (c == 1 ? a.L : 0.f), p[2] + (c == 2 ? a.L : 0.f), fa);
      ok = ok && field(a, p[0] - (c == 0 ? a.L : 0.f), p[1] - (c == 1 ? a.L : 0.f), p[2] - (c == 2 ? a.L : 0.f), fb);
      g[c] = ok ? fa - fb : 0.f;
    }
    const float gl = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (ok && gl > 0.f) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = p[c], out[3 + c] = g[c] / gl;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.vertex[3 * i + c] = out[c];
    a.normal[3 * i + c] = out[3 + c];
  }
}

// ------------------------------------------------------------------------------------------------
// ICP sums
// ------------------------------------------------------------------------------------------------
struct IcpArgs {
  const float *sv, *sn, *mv, *mn;  // source maps [Hs][Ws][3] (camera frame), model maps [Hm][Wm][3] (world)
  int32_t Hs, Ws, Hm, Wm, stride, sh, sw;
  int64_t n;      // sh * sw strided source pixels
  double T[12];   // the estimate, rows 0..2
  double M[12];   // the model camera's world-to-camera, rows 0..2
  double fx, fy, cx, cy, dist_th, cos_th;
  int32_t groups;
  double *partial, *out;  // [groups][29], [29]
  uint8_t* mask;          // [Hs][Ws] accepted pixels, or NULL
};

__device__ __forceinline__ void rigid(const double* m, const double x, const double y, const double z, double p[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) p[c] = ((m[4 * c] * x + m[4 * c + 1] * y) + m[4 * c + 2] * z) + m[4 * c + 3];
}

// the terms of strided pixel i: false when it has no accepted association
__device__ __forceinline__ bool icp_term(const IcpArgs& a, int64_t i, double J[6], double& r, int64_t& at) {
  const int32_t u = (int32_t)(i % a.sw) * a.stride, v = (int32_t)(i / a.sw) * a.stride;
  at = (int64_t)v * a.Ws + u;
  const float* s = a.sv + 3 * at;
  const float* sn = a.sn + 3 * at;
  const float sx = s[0], sy = s[1], sz = s[2], nx = sn[0], ny = sn[1], nz = sn[2];
  if (!(sx == sx && sy == sy && sz == sz && nx == nx && ny == ny && nz == nz)) return false;
  double p[3], pc[3];
  rigid(a.T, (double)sx, (double)sy, (double)sz, p);
  rigid(a.M, p[0], p[1], p[2], pc);
  if (!(pc[2] > 0.0)) return false;
  const double uf = ((pc[0] * a.fx) / pc[2] + a.cx) + 0.5, vf = ((pc[1] * a.fy) / pc[2] + a.cy) + 0.5;
  if (!(uf >= 0.0 && uf < (double)a.Wm && vf >= 0.0 && vf < (double)a.Hm)) return false;
  const int32_t um = (int32_t)uf, vm = (int32_t)vf;  // 0 <= um < Wm, 0 <= vm < Hm by the test above
  const float* mq = a.mv + 3 * ((int64_t)vm * a.Wm + um);
  const float* mn = a.mn + 3 * ((int64_t)vm * a.Wm + um);
  const float qx = mq[0], qy = mq[1], qz = mq[2], mx = mn[0], my = mn[1], mz = mn[2];
  if (!(qx == qx && qy == qy && qz == qz && mx == mx && my == my && mz == mz)) return false;
  const double dx = p[0] - (double)qx, dy = p[1] - (double)qy, dz = p[2] - (double)qz;
  if (!(sqrt((dx * dx + dy * dy) + dz * dz) <= a.dist_th)) return false;
  const double n[3] = {(double)mx, (double)my, (double)mz};
  double rn[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rn[c] = (a.T[4 * c] * (double)nx + a.T[4 * c + 1] * (double)ny) + a.T[4 * c + 2] * (double)nz;
  if (!((rn[0] * n[0] + rn[1] * n[1]) + rn[2] * n[2] >= a.cos_th)) return false;
  r = (n[0] * dx + n[1] * dy) + n[2] * dz;
  J[0] = p[1] * n[2] - p[2] * n[1];
  J[1] = p[2] * n[0] - p[0] * n[2];
  J[2] = p[0] * n[1] - p[1] * n[0];
  J[3] = n[0], J[4] = n[1], J[5] = n[2];
  return true;
}

// The reduction both sums kernels share.  Each thread adds its pixels i = tid, tid + threads, ... in ascending
// order (add_term); the workgroup's 29 partials are nslam_reduce.h's group_sum (store_group_sums), and k_icp_final
// adds the workgroups' partials with its wave_ordered_sum.
__device__ __forceinline__ void add_term(double acc[kSums], const double J[6], const double r) {
  int j = 0;
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int y = x; y < 6; ++y) acc[j++] += J[x] * J[y];
#pragma unroll
  for (int x = 0; x < 6; ++x) acc[21 + x] += J[x] * r;
  acc[27] += r * r;
  acc[28] += 1.0;
}

__device__ __forceinline__ void store_group_sums(const double (&acc)[kSums], double (*lds)[kSums], double* partial) {
  const double s = group_sum<kThreads>(acc, lds);
  if (threadIdx.x < kSums) partial[(int64_t)blockIdx.x * kSums + threadIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void k_icp_partials(IcpArgs a) {
  __shared__ double lds[kThreads / 64][kSums];
  double acc[kSums];
#pragma unroll
  for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
  const int64_t total = (int64_t)a.groups * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += total) {
    double J[6], r;
    int64_t at;
    const bool ok = icp_term(a, i, J, r, at);
    if (a.mask) a.mask[at] = ok ? 1 : 0;
    if (!ok) continue;
    add_term(acc, J, r);
  }
  store_group_sums(acc, lds, a.partial);
}

// out[j] = the partials of workgroups 0, 1, ... added in that order: one wave per sum j
__global__ __launch_bounds__(64) void k_icp_final(const double* partial, int32_t groups, double* out) {
  const int j = blockIdx.x;
  if (j >= kSums) return;
  groups = groups < kMaxGroups ? groups : kMaxGroups;
  const double s = wave_ordered_sum(as_global(partial) + j, groups, kSums);
  if (threadIdx.x == 0) out[j] = s;
}

// ------------------------------------------------------------------------------------------------
// grey pyramid
// ------------------------------------------------------------------------------------------------
constexpr int kMaxLevels = 8;

inline int32_t half_up(int32_t n) { return (n + 1) / 2; }

__global__ __launch_bounds__(kThreads) void k_gray(const uint8_t* rgb, int64_t n, float* out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float r = (float)rgb[3 * i], g = (float)rgb[3 * i + 1], b = (float)rgb[3 * i + 2];
  out[i] = ((0.299f * r + 0.587f * g) + 0.114f * b) / 255.0f;
}

// out (oh x ow) from in (h x w): pixel (i, j) is the (1/4, 1/2, 1/4) binomial around in(2 i, 2 j), rows first,
// indices clamped to the image (2 i <= w - 1 and 2 j <= h - 1 since ow = ceil(w / 2), oh = ceil(h / 2))
__global__ __launch_bounds__(kThreads) void k_gray_down(const float* in, int32_t h, int32_t w, float* out,
                                                        int32_t oh, int32_t ow) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= (int64_t)oh * ow) return;
  const int32_t i = (int32_t)(q % ow), j = (int32_t)(q / ow);
  const int32_t x1 = 2 * i, x0 = x1 > 0 ? x1 - 1 : 0, x2 = x1 + 1 < w ? x1 + 1 : w - 1;
  const int32_t y1 = 2 * j, y0 = y1 > 0 ? y1 - 1 : 0, y2 = y1 + 1 < h ? y1 + 1 : h - 1;
  const float* r0 = in + (int64_t)y0 * w;
  const float* r1 = in + (int64_t)y1 * w;
  const float* r2 = in + (int64_t)y2 * w;
  const float h0 = (0.25f * r0[x0] + 0.5f * r0[x1]) + 0.25f * r0[x2];
  const float h1 = (0.25f * r1[x0] + 0.5f * r1[x1]) + 0.25f * r1[x2];
  const float h2 = (0.25f * r2[x0] + 0.5f * r2[x1]) + 0.25f * r2[x2];
  out[q] = (0.25f * h0 + 0.5f * h1) + 0.25f * h2;
}

// ------------------------------------------------------------------------------------------------
// photometric sums
// ------------------------------------------------------------------------------------------------
struct PhotoArgs {
  const float *sv, *sg, *rg, *rv;  // source vertices [Hs][Ws][3], source / reference grey level, reference
                                   // vertices [Hr][Wr][3] (each in its own camera frame)
  int32_t Hs, Ws, Hr, Wr, stride, sh, sw, rh, rw;
  int64_t n;      // sh * sw strided source pixels = the pixels of the source level
  double T[12];   // the estimate, rows 0..2
  double M[12];   // the reference camera's world-to-camera, rows 0..2
  double fx, fy, cx, cy, depth_th, photo_th, scale;  // scale = 2^level = stride
  int32_t groups;
  double* partial;  // [groups][29]
  uint8_t* mask;    // [Hs][Ws] accepted pixels, or NULL
};

// the terms of strided pixel i: false when a gate rejects it
__device__ __forceinline__ bool photo_term(const PhotoArgs& a, int64_t i, double J[6], double& r, int64_t& at) {
  const int32_t u = (int32_t)(i % a.sw) * a.stride, v = (int32_t)(i / a.sw) * a.stride;
  at = (int64_t)v * a.Ws + u;
  const float* s = a.sv + 3 * at;
  const float sx = s[0], sy = s[1], sz = s[2];
  if (!(sx == sx && sy == sy && sz == sz)) return false;
  double p[3], pc[3];
  rigid(a.T, (double)sx, (double)sy, (double)sz, p);
  rigid(a.M, p[0], p[1], p[2], pc);
  const double z = pc[2];
  if (!(z > 0.0)) return false;
  const double x0 = (pc[0] * a.fx) / z + a.cx, y0 = (pc[1] * a.fy) / z + a.cy;
  // occlusion: the reference frame's own depth at the nearest pixel
  const double xn = x0 + 0.5, yn = y0 + 0.5;
  if (!(xn >= 0.0 && xn < (double)a.Wr && yn >= 0.0 && yn < (double)a.Hr)) return false;
  const int32_t un = (int32_t)xn, vn = (int32_t)yn;  // 0 <= un < Wr, 0 <= vn < Hr by the test above
  const float* q = a.rv + 3 * ((int64_t)vn * a.Wr + un);
  const float qx = q[0], qy = q[1], qz = q[2];
  if (!(qx == qx && qy == qy && qz == qz)) return false;
  if (!(fabs(z - (double)qz) <= a.depth_th)) return false;
  // the bilinear cell of the reference level
  const double xl = x0 / a.scale, yl = y0 / a.scale;
  const double fi = floor(xl), fj = floor(yl);
  if (!(fi >= 0.0 && fi + 1.0 <= (double)(a.rw - 1) && fj >= 0.0 && fj + 1.0 <= (double)(a.rh - 1))) return false;
  const int32_t i0 = (int32_t)fi, j0 = (int32_t)fj;  // 0 <= i0 <= rw - 2, 0 <= j0 <= rh - 2 by the test above
  const double ca = xl - fi, cb = yl - fj;
  const float* t0 = a.rg + (int64_t)j0 * a.rw + i0;
  const float* t1 = t0 + a.rw;
  const double I00 = (double)t0[0], I10 = (double)t0[1], I01 = (double)t1[0], I11 = (double)t1[1];
  const double Iref = (1.0 - cb) * ((1.0 - ca) * I00 + ca * I10) + cb * ((1.0 - ca) * I01 + ca * I11);
  const double gx = ((1.0 - cb) * (I10 - I00) + cb * (I11 - I01)) / a.scale;
  const double gy = ((1.0 - ca) * (I01 - I00) + ca * (I11 - I10)) / a.scale;
  r = Iref - (double)a.sg[i];
  if (!(fabs(r) <= a.photo_th)) return false;
  const double zz = z * z;
  const double gc[3] = {gx * (a.fx / z), gy * (a.fy / z),
                        gx * (-((a.fx * pc[0]) / zz)) + gy * (-((a.fy * pc[1]) / zz))};
  double gw[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) gw[c] = (a.M[c] * gc[0] + a.M[4 + c] * gc[1]) + a.M[8 + c] * gc[2];
  J[0] = p[1] * gw[2] - p[2] * gw[1];
  J[1] = p[2] * gw[0] - p[0] * gw[2];
  J[2] = p[0] * gw[1] - p[1] * gw[0];
  J[3] = gw[0], J[4] = gw[1], J[5] = gw[2];
  return true;
}

__global__ __launch_bounds__(kThreads) void k_photo_partials(PhotoArgs a) {
  __shared__ double lds[kThreads / 64][kSums];
  double acc[kSums];
#pragma unroll
  for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
  const int64_t total = (int64_t)a.groups * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += total) {
    double J[6], r;
    int64_t at;
    const bool ok = photo_term(a, i, J, r, at);
    if (a.mask) a.mask[at] = ok ? 1 : 0;
    if (!ok) continue;
    add_term(acc, J, r);
  }
  store_group_sums(acc, lds, a.partial);
}

bool finite12(const double* m) {
  for (int k = 0; k < 12; ++k)
    if (!(fabs(m[k]) <= 1.0e300)) return false;
  return true;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C entry points (include/nslam.h)
// ------------------------------------------------------------------------------------------------
extern "C" int nslam_depth_maps(const float* depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                float depth_trunc, float max_jump, float* vertex, float* normal, void* stream) {
  if (!depth || !vertex || !normal || H <= 0 || W <= 0) return NSLAM_EINVAL;
  if (!(fx != 0.f) || !(fy != 0.f) || !(depth_trunc > 0.f) || !(max_jump >= 0.f)) return NSLAM_EINVAL;
  if ((int64_t)H * W >= (int64_t(1) << 31) / 3) return NSLAM_EUNSUPPORTED;
  MapArgs a{depth, H, W, fx, fy, cx, cy, depth_trunc, max_jump, vertex, normal};
  hipLaunchKernelGGL(k_depth_maps, dim3((unsigned)blocks_for((int64_t)H * W)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_tsdf_raycast(const int32_t* table, const int32_t* pool_key, const float* tsdf,
                                  const float* weight, int64_t n_pool, const int32_t* block_lo,
                                  const int32_t* block_hi, double voxel, double trunc, const double* c2w, int32_t H,
                                  int32_t W, double fx, double fy, double cx, double cy, double near, double far,
                                  float* vertex, float* normal, void* stream) {
  if (!table || !block_lo || !block_hi || !c2w || !vertex || !normal || H <= 0 || W <= 0 || n_pool < 0)
    return NSLAM_EINVAL;
  if (n_pool > 0 && (!pool_key || !tsdf || !weight)) return NSLAM_EINVAL;
  if (!(voxel > 0.0) || !(voxel <= 1.0e30) || !(trunc > 0.0) || !(2.0 * trunc <= 16.0 * voxel)) return NSLAM_EINVAL;
  if (!(fx != 0.0) || !(fy != 0.0) || !(near >= 0.0) || !(far > near) || !(far <= 1.0e30)) return NSLAM_EINVAL;
  CastArgs a{};
  int64_t cells = 1;
  for (int c = 0; c < 3; ++c) {
    if (block_hi[c] <= block_lo[c] || block_lo[c] < -kMaxBlock || block_hi[c] > kMaxBlock) return NSLAM_EINVAL;
    a.lo[c] = block_lo[c];
    a.n[c] = block_hi[c] - block_lo[c];
    cells *= a.n[c];
    if (cells > kMaxCells) return NSLAM_EINVAL;
  }
  if ((int64_t)H * W >= (int64_t(1) << 31) / 3) return NSLAM_EUNSUPPORTED;
  if (3 * (int64_t)kVox * n_pool >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  a.table = table;
  a.pool_key = pool_key;
  a.tsdf = tsdf;
  a.weight = weight;
  a.n_pool = n_pool;
  a.H = H;
  a.W = W;
  for (int k = 0; k < 12; ++k) a.m[k] = (float)c2w[k];  // a pose that is not finite: every pixel ends invalid
  a.fx = (float)fx;
  a.fy = (float)fy;
  a.cx = (float)cx;
  a.cy = (float)cy;
  a.near = (float)near;
  a.far = (float)far;
  a.L = (float)voxel;
  a.B = 16.0f * a.L;
  a.step = 0.75f * (float)trunc;
  if (!(a.step > 0.f) || !(a.L > 0.f)) return NSLAM_EINVAL;
  a.vertex = vertex;
  a.normal = normal;
  hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)blocks_for((int64_t)H * W)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int64_t nslam_icp_partials(int32_t H, int32_t W, int32_t stride) {
  if (H <= 0 || W <= 0 || stride < 1) return 0;
  const int64_t n = (int64_t)((H + stride - 1) / stride) * ((W + stride - 1) / stride);
  const int64_t g = blocks_for(n);
  return g < kMaxGroups ? g : kMaxGroups;
}

extern "C" int nslam_icp_sums(const float* src_vertex, const float* src_normal, int32_t Hs, int32_t Ws,
                              int32_t stride, const double* T, const float* model_vertex,
                              const float* model_normal, int32_t Hm, int32_t Wm, const double* w2c, double fx,
                              double fy, double cx, double cy, double dist_th, double cos_th, double* partial,
                              int64_t n_partial, double* out, uint8_t* mask, void* stream) {
  if (!src_vertex || !src_normal || !model_vertex || !model_normal || !T || !w2c || !out || !partial)
    return NSLAM_EINVAL;
  if (Hs <= 0 || Ws <= 0 || Hm <= 0 || Wm <= 0 || stride < 1) return NSLAM_EINVAL;
  if (!(fx != 0.0) || !(fy != 0.0) || !(dist_th >= 0.0) || !(cos_th >= -1.0 && cos_th <= 1.0)) return NSLAM_EINVAL;
  if (!finite12(T) || !finite12(w2c)) return NSLAM_EINVAL;
  if ((int64_t)Hs * Ws >= (int64_t(1) << 31) / 3 || (int64_t)Hm * Wm >= (int64_t(1) << 31) / 3)
    return NSLAM_EUNSUPPORTED;
  const int64_t groups = nslam_icp_partials(Hs, Ws, stride);
  if (n_partial < groups) return NSLAM_EWORKSPACE;
  IcpArgs a{};
  a.sv = src_vertex;
  a.sn = src_normal;
  a.mv = model_vertex;
  a.mn = model_normal;
  a.Hs = Hs;
  a.Ws = Ws;
  a.Hm = Hm;
  a.Wm = Wm;
  a.stride = stride;
  a.sh = (Hs + stride - 1) / stride;
  a.sw = (Ws + stride - 1) / stride;
  a.n = (int64_t)a.sh * a.sw;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k], a.M[k] = w2c[k];
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.dist_th = dist_th;
  a.cos_th = cos_th;
  a.groups = (int32_t)groups;
  a.partial = partial;
  a.out = out;
  a.mask = mask;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (mask && hipMemsetAsync(mask, 0, (size_t)Hs * Ws, s) != hipSuccess) return NSLAM_EHIP - (int)hipGetLastError();
  hipLaunchKernelGGL(k_icp_partials, dim3((unsigned)groups), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_icp_final, dim3(kSums), dim3(64), 0, s, (const double*)partial, (int32_t)groups, out);
  return hip_status();
}

extern "C" int64_t nslam_gray_pyramid_size(int32_t H, int32_t W, int32_t levels) {
  if (H <= 0 || W <= 0 || levels < 1 || levels > kMaxLevels) return 0;
  int64_t n = 0;
  for (int l = 0; l < levels; ++l, H = half_up(H), W = half_up(W)) n += (int64_t)H * W;
  return n;
}

extern "C" int nslam_gray_pyramid(const uint8_t* rgb, int32_t H, int32_t W, int32_t levels, float* out,
                                  void* stream) {
  if (!rgb || !out || H <= 0 || W <= 0 || levels < 1 || levels > kMaxLevels) return NSLAM_EINVAL;
  if ((int64_t)H * W >= (int64_t(1) << 31) / 3) return NSLAM_EUNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_gray, dim3((unsigned)blocks_for((int64_t)H * W)), dim3(kThreads), 0, s, rgb, (int64_t)H * W,
                     out);
  int32_t h = H, w = W;
  for (int l = 1; l < levels; ++l) {
    const int32_t oh = half_up(h), ow = half_up(w);
    float* next = out + (int64_t)h * w;
    hipLaunchKernelGGL(k_gray_down, dim3((unsigned)blocks_for((int64_t)oh * ow)), dim3(kThreads), 0, s,
                       (const float*)out, h, w, next, oh, ow);
    out = next, h = oh, w = ow;
  }
  return hip_status();
}

extern "C" int nslam_photo_sums(const float* src_vertex, int32_t Hs, int32_t Ws, const float* src_gray,
                                int32_t src_h, int32_t src_w, const float* ref_gray, int32_t ref_h, int32_t ref_w,
                                int32_t level, const float* ref_vertex, int32_t Hr, int32_t Wr, const double* T,
                                const double* w2c, double fx, double fy, double cx, double cy, double depth_th,
                                double photo_th, double* partial, int64_t n_partial, double* out, uint8_t* mask,
                                void* stream) {
  if (!src_vertex || !src_gray || !ref_gray || !ref_vertex || !T || !w2c || !out || !partial) return NSLAM_EINVAL;
  if (Hs <= 0 || Ws <= 0 || Hr <= 0 || Wr <= 0 || level < 0 || level >= kMaxLevels) return NSLAM_EINVAL;
  if (!(fx != 0.0) || !(fy != 0.0) || !(depth_th >= 0.0) || !(photo_th >= 0.0)) return NSLAM_EINVAL;
  if (!(fabs(fx) <= 1.0e300 && fabs(fy) <= 1.0e300 && fabs(cx) <= 1.0e300 && fabs(cy) <= 1.0e300)) return NSLAM_EINVAL;
  if (!finite12(T) || !finite12(w2c)) return NSLAM_EINVAL;
  if ((int64_t)Hs * Ws >= (int64_t(1) << 31) / 3 || (int64_t)Hr * Wr >= (int64_t(1) << 31) / 3)
    return NSLAM_EUNSUPPORTED;
  const int32_t stride = 1 << level;
  PhotoArgs a{};
  a.sh = (Hs + stride - 1) / stride;
  a.sw = (Ws + stride - 1) / stride;
  a.rh = (Hr + stride - 1) / stride;
  a.rw = (Wr + stride - 1) / stride;
  if (src_h != a.sh || src_w != a.sw || ref_h != a.rh || ref_w != a.rw) return NSLAM_EINVAL;
  const int64_t groups = nslam_icp_partials(Hs, Ws, stride);
  if (n_partial < groups) return NSLAM_EWORKSPACE;
  a.sv = src_vertex;
  a.sg = src_gray;
  a.rg = ref_gray;
  a.rv = ref_vertex;
  a.Hs = Hs;
  a.Ws = Ws;
  a.Hr = Hr;
  a.Wr = Wr;
  a.stride = stride;
  a.n = (int64_t)a.sh * a.sw;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k], a.M[k] = w2c[k];
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.depth_th = depth_th;
  a.photo_th = photo_th;
  a.scale = (double)stride;
  a.groups = (int32_t)groups;
  a.partial = partial;
  a.mask = mask;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (mask && hipMemsetAsync(mask, 0, (size_t)Hs * Ws, s) != hipSuccess) return NSLAM_EHIP - (int)hipGetLastError();
  hipLaunchKernelGGL(k_photo_partials, dim3((unsigned)groups), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_icp_final, dim3(kSums), dim3(64), 0, s, (const double*)partial, (int32_t)groups, out);
  return hip_status();
}
