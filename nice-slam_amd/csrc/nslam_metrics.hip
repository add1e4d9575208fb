// nslam_metrics.hip — rendering-quality metrics of a finished run (evaluation.render_metrics / eval_rendering):
//   nslam_image_errors   per image Σ(color - gt_color)², its count, Σ|depth - gt_depth| over gt_depth > 0, its count
//   nslam_ssim           per image, level and channel the spatial means of the SSIM and CS maps (Wang et al. 2004;
//                        Wang, Simoncelli, Bovik 2003 for the five-level form): 11-tap Gaussian window, "valid"
//                        correlation, 2x2 mean pooling between levels
// Sums: every workgroup writes ONE float64 partial per quantity to the workspace and a second launch adds the
// partials in index order, so two calls give the same bits (nslam_reduce.h has the order and the two sums).
// Float32 order of the SSIM maps (the build has -ffp-contract=off; tests/metrics_cases.py restates it): products
// x², y², xy first, then per moment the horizontal pass Σ_i g[i]·v[c+i] with i ascending from a zero sum, then the
// vertical pass over the horizontal results in the same way, then the formulas of ssim_point() as written.
#include <math.h>

#include "nslam_dev.h"
#include "nslam_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ------------------------------------------------------------------------------------------------
// image errors
// ------------------------------------------------------------------------------------------------
constexpr int kErrPixels = 4;                        // pixels per thread and pass
constexpr int kErrShare = kThreads * kErrPixels;     // a workgroup's pixels per pass
constexpr int kErrMaxBlocks = 1024;                  // workgroups per image; past share x grid they stride

struct ErrArgs {
  const float *color, *gt_color, *depth, *gt_depth;
  int64_t n_pix;
  int32_t C, mask_mode, clamp, blocks;
  double* partials;  // [B][blocks][4]
};

inline int32_t err_blocks(int64_t n_pix) {
  const int64_t b = (n_pix + kErrShare - 1) / kErrShare;
  return (int32_t)(b < 1 ? 1 : (b > kErrMaxBlocks ? kErrMaxBlocks : b));
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// grid (blocks, B): a thread walks pixels tid + kThreads·(j + kErrPixels·(block + blocks·pass)) in order
__global__ __launch_bounds__(kThreads) void k_image_errors(ErrArgs a) {
  __shared__ double part[kWaves][4];
  const int64_t img = blockIdx.y;
  const gptr_t<float> col = a.color ? as_global(a.color) + img * a.n_pix * a.C : nullptr;
  const gptr_t<float> gcol = a.color ? as_global(a.gt_color) + img * a.n_pix * a.C : nullptr;
  const gptr_t<float> dep = a.depth ? as_global(a.depth) + img * a.n_pix : nullptr;
  const gptr_t<float> gdep = a.gt_depth ? as_global(a.gt_depth) + img * a.n_pix : nullptr;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t base = (int64_t)blockIdx.x * kErrShare; base < a.n_pix; base += (int64_t)a.blocks * kErrShare) {
#pragma unroll
    for (int j = 0; j < kErrPixels; ++j) {
      const int64_t p = base + j * kThreads + threadIdx.x;
      if (p >= a.n_pix) continue;
      const bool valid = gdep ? gdep[p] > 0.f : false;
      if (dep && valid) {
        s[2] += fabs((double)dep[p] - (double)gdep[p]);
        s[3] += 1.0;
      }
      if (col && (a.mask_mode == 0 || valid)) {
        for (int c = 0; c < a.C; ++c) {
          float v = col[p * a.C + c];
          if (a.clamp) v = clamp01(v);
          const double d = (double)v - (double)gcol[p * a.C + c];
          s[0] += d * d;
        }
        s[1] += (double)a.C;
      }
    }
  }
  const double t = group_sum<kThreads>(s, part);
  if (threadIdx.x < 4) a.partials[(img * a.blocks + blockIdx.x) * 4 + threadIdx.x] = t;
}

// out[i][k] = Σ_j partials[i][j][k], j ascending: one wave per output value, grid n_out · K
__global__ __launch_bounds__(64) void k_sum_partials(const double* partials, int32_t n_part, int32_t K, double* out) {
  const int64_t t = blockIdx.x;
  const int64_t i = t / K;
  const int k = (int)(t % K);
  const double s = wave_ordered_sum(as_global(partials) + i * n_part * K + k, n_part, K);
  if (threadIdx.x == 0) out[t] = s;
}

// ------------------------------------------------------------------------------------------------
// SSIM
// ------------------------------------------------------------------------------------------------
constexpr int kWin = 11;
constexpr int kHalo = kWin - 1;
constexpr int kTile = 32;                 // outputs per tile side (profiles/metrics_resources.txt: why 32)
constexpr int kIn = kTile + kHalo;        // 42: the tile with its halo
constexpr int kRows = kTile / (kThreads / kTile);  // 4 output rows per thread of the vertical pass
constexpr int kMaxLevels = 5;

struct Window {
  float g[kWin];
};

struct SsimArgs {
  const float *x, *y;   // level 0: [B][h][w][C] interleaved (C = channels); pooled levels: planar [B·C][h][w]
  int32_t h, w, C;      // C = 1 for a planar level
  int32_t tiles_x, tiles_y;
  float C1, C2;
  Window win;
  double* partials;     // [B·C][tiles_y][tiles_x][2]
};

__device__ __forceinline__ void ssim_point(float mx, float my, float exx, float eyy, float exy, float C1, float C2,
                                           float& ssim, float& cs) {
  const float mxx = mx * mx, myy = my * my, mxy = mx * my;
  const float sx = exx - mxx, sy = eyy - myy, sxy = exy - mxy;
  cs = (2.f * sxy + C2) / ((sx + sy) + C2);
  ssim = ((2.f * mxy + C1) / ((mxx + myy) + C1)) * cs;
}

// grid (tiles_x, tiles_y, images·channels), 256 threads: the tile and its halo of x and y into LDS, the
// horizontal pass into five moment planes in LDS, the vertical pass into registers (4 rows per thread, one column),
// ssim and cs per output, their float64 sums over the workgroup → one partial pair
__global__ __launch_bounds__(kThreads) void k_ssim_level(SsimArgs a) {
  __shared__ float in_x[kIn][kIn], in_y[kIn][kIn];
  __shared__ float hp[5][kIn][kTile];
  __shared__ double part[kWaves][2];
  const int tid = threadIdx.x;
  const int plane = blockIdx.z;
  const int img = plane / a.C, ch = plane % a.C;   // planar levels: C = 1, img = plane
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const gptr_t<float> gx = as_global(a.x) + (int64_t)img * a.h * a.w * a.C + ch;
  const gptr_t<float> gy = as_global(a.y) + (int64_t)img * a.h * a.w * a.C + ch;
  for (int e = tid; e < kIn * kIn; e += kThreads) {
    const int r = e / kIn, c = e % kIn;
    const int yy = y0 + r, xx = x0 + c;
    float vx = 0.f, vy = 0.f;
    if (yy < a.h && xx < a.w) {
      const int64_t o = ((int64_t)yy * a.w + xx) * a.C;
      vx = gx[o];
      vy = gy[o];
    }
    in_x[r][c] = vx;
    in_y[r][c] = vy;
  }
  __syncthreads();
  for (int e = tid; e < kIn * kTile; e += kThreads) {
    const int r = e / kTile, c = e % kTile;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int i = 0; i < kWin; ++i) {
      const float vx = in_x[r][c + i], vy = in_y[r][c + i], g = a.win.g[i];
      s0 += g * vx;
      s1 += g * vy;
      s2 += g * (vx * vx);
      s3 += g * (vy * vy);
      s4 += g * (vx * vy);
    }
    hp[0][r][c] = s0;
    hp[1][r][c] = s1;
    hp[2][r][c] = s2;
    hp[3][r][c] = s3;
    hp[4][r][c] = s4;
  }
  __syncthreads();
  const int tx = tid % kTile, tr = (tid / kTile) * kRows;
  float acc[kRows][5];
#pragma unroll
  for (int o = 0; o < kRows; ++o)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[o][k] = 0.f;
#pragma unroll
  for (int j = 0; j < kRows + kHalo; ++j) {
    float v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = hp[k][tr + j][tx];
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
      const int i = j - o;  // the tap of output row o that meets input row j: ascending in j
      if (i >= 0 && i < kWin) {
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[o][k] += a.win.g[i] * v[k];
      }
    }
  }
  double s[2] = {0.0, 0.0};
  const int out_h = a.h - kHalo, out_w = a.w - kHalo;
#pragma unroll
  for (int o = 0; o < kRows; ++o) {
    if (y0 + tr + o < out_h && x0 + tx < out_w) {
      float ssim, cs;
      ssim_point(acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4], a.C1, a.C2, ssim, cs);
      s[0] += (double)ssim;
      s[1] += (double)cs;
    }
  }
  const double t = group_sum<kThreads>(s, part);
  if (tid < 2) a.partials[(((int64_t)plane * a.tiles_y + blockIdx.y) * a.tiles_x + blockIdx.x) * 2 + tid] = t;
}

struct PoolArgs {
  const float *x, *y;  // [B][h][w][C] (C channels interleaved) or planar with C = 1
  float *ox, *oy;      // planar [B·C][h2][w2]
  int32_t h, w, C, h2, w2, pad_y, pad_x;
  int64_t n;           // B·C·h2·w2
};

// 2x2 mean with stride 2; an odd side is padded with one zero row / column on each side first (the divisor
// stays 4): ((v00 + v01) + v10) + v11, then · 0.25
__global__ __launch_bounds__(kThreads) void k_pool2(PoolArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= a.n) return;
  const int ox = (int)(t % a.w2);
  const int oy = (int)((t / a.w2) % a.h2);
  const int64_t plane = t / ((int64_t)a.w2 * a.h2);
  const int64_t img = plane / a.C;
  const int ch = (int)(plane % a.C);
  const gptr_t<float> gx = as_global(a.x) + img * a.h * a.w * a.C + ch;
  const gptr_t<float> gy = as_global(a.y) + img * a.h * a.w * a.C + ch;
  float vx[4], vy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = 2 * oy - a.pad_y + (k >> 1), xx = 2 * ox - a.pad_x + (k & 1);
    vx[k] = vy[k] = 0.f;
    if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
      const int64_t o = ((int64_t)yy * a.w + xx) * a.C;
      vx[k] = gx[o];
      vy[k] = gy[o];
    }
  }
  as_global_w(a.ox)[t] = (((vx[0] + vx[1]) + vx[2]) + vx[3]) * 0.25f;
  as_global_w(a.oy)[t] = (((vy[0] + vy[1]) + vy[2]) + vy[3]) * 0.25f;
}

// out[b][l][c][k] = (Σ_t partials_l[b·C + c][t][k], t ascending) / outputs_l
struct SsimSumArgs {
  const double* partials[kMaxLevels];
  int32_t n_tiles[kMaxLevels];
  double n_out[kMaxLevels];
  int32_t levels, planes, C;  // planes = B·C
  double* out;              // [B][levels][C][2]
};

__global__ __launch_bounds__(64) void k_ssim_sum(SsimSumArgs a) {  // one wave per sum, grid planes · levels · 2
  const int t = blockIdx.x;
  const int k = t & 1, plane = (t >> 1) % a.planes, l = (t >> 1) / a.planes;
  const double* pl = a.partials[0];
  int32_t n = a.n_tiles[0];
  double n_out = a.n_out[0];
#pragma unroll
  for (int q = 1; q < kMaxLevels; ++q)
    if (l == q) {
      pl = a.partials[q];
      n = a.n_tiles[q];
      n_out = a.n_out[q];
    }
  const double s = wave_ordered_sum(as_global(pl) + (int64_t)plane * n * 2 + k, n, 2);
  const int img = plane / a.C, ch = plane % a.C;
  if (threadIdx.x == 0) a.out[(((int64_t)img * a.levels + l) * a.C + ch) * 2 + k] = s / n_out;
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int32_t pooled(int32_t s) { return (s + 1) / 2; }  // floor((s + 2 (s mod 2) - 2) / 2) + 1
inline int32_t tiles(int32_t s) { return (s - kHalo + kTile - 1) / kTile; }

inline bool ssim_shape_ok(int32_t B, int32_t H, int32_t W, int32_t C, int32_t levels) {
  if (B < 0 || (C != 1 && C != 3) || (levels != 1 && levels != kMaxLevels)) return false;
  const int32_t m = H < W ? H : W;
  if (levels == 1 ? m < kWin : m <= 160) return false;
  return (int64_t)B * C <= 65535 && tiles(H) <= 65535 && (int64_t)H * W < ((int64_t)1 << 31);
}

}  // namespace

extern "C" size_t nslam_image_errors_workspace_size(int32_t n_images, int64_t n_pix) {
  if (n_images <= 0 || n_pix <= 0) return 0;
  return (size_t)n_images * err_blocks(n_pix) * 4 * sizeof(double);
}

extern "C" int nslam_image_errors(const float* color, const float* gt_color, const float* depth,
                                  const float* gt_depth, int32_t n_images, int64_t n_pix, int32_t channels,
                                  int32_t mask_mode, int32_t clamp, double* out, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (n_images < 0 || n_images > 65535 || n_pix <= 0 || n_pix >= ((int64_t)1 << 40)) return NSLAM_EINVAL;
  if ((color == nullptr) != (gt_color == nullptr)) return NSLAM_EINVAL;
  if (color && channels != 1 && channels != 3) return NSLAM_EINVAL;
  if (depth && !gt_depth) return NSLAM_EINVAL;
  if (mask_mode != 0 && mask_mode != 1) return NSLAM_EINVAL;
  if (mask_mode == 1 && color && !gt_depth) return NSLAM_EINVAL;
  if (n_images == 0) return NSLAM_OK;
  if (!out) return NSLAM_EINVAL;
  if (!ws || ws_bytes < nslam_image_errors_workspace_size(n_images, n_pix)) return NSLAM_EWORKSPACE;
  ErrArgs a;
  a.color = color;
  a.gt_color = gt_color;
  a.depth = depth;
  a.gt_depth = gt_depth;
  a.n_pix = n_pix;
  a.C = color ? channels : 1;
  a.mask_mode = mask_mode;
  a.clamp = clamp ? 1 : 0;
  a.blocks = err_blocks(n_pix);
  a.partials = (double*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_image_errors, dim3((unsigned)a.blocks, (unsigned)n_images), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(k_sum_partials, dim3((unsigned)n_images * 4), dim3(64), 0, st, (const double*)a.partials,
                     a.blocks, 4, out);
  return hip_status();
}

extern "C" size_t nslam_ssim_workspace_size(int32_t n_images, int32_t H, int32_t W, int32_t channels,
                                            int32_t levels) {
  if (!ssim_shape_ok(n_images, H, W, channels, levels) || n_images == 0) return 0;
  const size_t planes = (size_t)n_images * channels;
  size_t bytes = 0;
  int32_t h = H, w = W;
  for (int l = 0; l < levels; ++l) {
    if (l > 0) {
      h = pooled(h);
      w = pooled(w);
      bytes += 2 * align256(planes * h * w * sizeof(float));  // the pooled x and y
    }
    bytes += align256(planes * tiles(h) * tiles(w) * 2 * sizeof(double));
  }
  return bytes;
}

extern "C" int nslam_ssim(const float* x, const float* y, int32_t n_images, int32_t H, int32_t W, int32_t channels,
                          double data_range, const float* window, int32_t levels, double* out, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!ssim_shape_ok(n_images, H, W, channels, levels)) return NSLAM_EINVAL;
  if (!window || !(data_range > 0.0)) return NSLAM_EINVAL;
  if (n_images == 0) return NSLAM_OK;
  if (!x || !y || !out) return NSLAM_EINVAL;
  if (!ws || ws_bytes < nslam_ssim_workspace_size(n_images, H, W, channels, levels)) return NSLAM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int32_t planes = n_images * channels;
  SsimArgs a;
  for (int i = 0; i < kWin; ++i) a.win.g[i] = window[i];
  a.C1 = (float)((0.01 * data_range) * (0.01 * data_range));
  a.C2 = (float)((0.03 * data_range) * (0.03 * data_range));
  SsimSumArgs sum;
  sum.levels = levels;
  sum.planes = planes;
  sum.C = channels;
  sum.out = out;
  for (int l = 0; l < kMaxLevels; ++l) {
    sum.partials[l] = nullptr;
    sum.n_tiles[l] = 0;
    sum.n_out[l] = 1.0;
  }
  char* p = (char*)ws;
  const float *cx = x, *cy = y;
  int32_t h = H, w = W, C = channels;
  for (int l = 0; l < levels; ++l) {
    if (l > 0) {
      PoolArgs q;
      q.x = cx;
      q.y = cy;
      q.h = h;
      q.w = w;
      q.C = C;
      q.pad_y = h & 1;
      q.pad_x = w & 1;
      q.h2 = pooled(h);
      q.w2 = pooled(w);
      q.n = (int64_t)planes * q.h2 * q.w2;
      const size_t plane_bytes = align256((size_t)q.n * sizeof(float));
      q.ox = (float*)p;
      q.oy = (float*)(p + plane_bytes);
      p += 2 * plane_bytes;
      hipLaunchKernelGGL(k_pool2, dim3((unsigned)((q.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
      cx = q.ox;
      cy = q.oy;
      h = q.h2;
      w = q.w2;
      C = 1;
    }
    a.x = cx;
    a.y = cy;
    a.h = h;
    a.w = w;
    a.C = C;
    a.tiles_x = tiles(w);
    a.tiles_y = tiles(h);
    a.partials = (double*)p;
    p += align256((size_t)planes * a.tiles_x * a.tiles_y * 2 * sizeof(double));
    sum.partials[l] = a.partials;
    sum.n_tiles[l] = a.tiles_x * a.tiles_y;
    sum.n_out[l] = (double)(h - kHalo) * (double)(w - kHalo);
    hipLaunchKernelGGL(k_ssim_level, dim3((unsigned)a.tiles_x, (unsigned)a.tiles_y, (unsigned)planes), dim3(kThreads),
                       0, st, a);
  }
  hipLaunchKernelGGL(k_ssim_sum, dim3((unsigned)(planes * levels * 2)), dim3(64), 0, st, sum);
  return hip_status();
}
