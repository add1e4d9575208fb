// nslam_imap.hip — the iMAP* decoder (configs/imap.yaml; decoder.py:91-203 with c_dim=0) on gfx950:
//   e = sin(p.float() @ B) [93];  h1 = relu(W0 e + b0);  h(i+1) = relu(Wi hi + bi), i = 1..3 [256];  raw = Wo h4 + bo
// forward, and a backward in three launches plus a reduction (nslam.h).
//
// Tiling.  A 512-thread workgroup (8 waves) owns a tile of 128 points.  The layer's input lives in LDS as a
// [feature][point] image X[256][128] (128 KiB of the CU's 160); wave w computes output features 32w..32w+31
// for all four 32-point sub-tiles as four v_mfma_f32_32x32x2_f32 accumulators, K running over the image's rows:
// the B operand of step s is X[2s + (lane>>5)][32 pt + (lane&31)] (one conflict-free ds_read_b32), the A
// operand is the wave's weight fragment, packed by nslam_imap_pack so that a lane's four steps are one
// 16-byte load shared by the four sub-tiles.  The accumulators stay in registers until a barrier after the K
// loop, so the image is updated in place.  A tile's weights (256 KiB per layer) are read once per workgroup
// and stay in L2.  The tape is the image itself, dumped per layer ([tile][layer][256][128]).
//
// The cotangent chain (k_imap_chain) is the same GEMM with the transposed fragments and the mask h > 0 read from
// the tape; it leaves every layer's masked cotangent G_l = da_l * mask_l as a tile image in the workspace.
// The weight gradients (k_imap_wgrad) are GEMMs over POINTS: both operands ([feature][point] images) are staged
// through LDS in 64-point chunks and read column-wise; a workgroup owns one layer and a slab of tiles, and
// writes one partial per slab, which k_imap_reduce sums in slab order into the caller's gradients.
#include <algorithm>
#include <cmath>

#include "nslam_dev.h"

namespace {

constexpr int kH = 256;    // hidden width
constexpr int kE = 93;     // embedding size
constexpr int kEP = 96;    // ... padded to the MFMA's K granularity (rows 93..95 are zero)
constexpr int kTP = 128;   // points per tile
constexpr int kThreads = 512;
constexpr int kImg = kH * kTP;          // floats of one tile image
constexpr int kGTile = 4 * kImg + kEP * kTP;  // chain output per tile: G_0..G_3 and de * cos
constexpr int kMaxSlabs = 64;

// packed fragments (floats): forward l0 (8 blocks, K 96), forward l1..3 (8 blocks, K 256), transposed l0
// (3 blocks, K 256), transposed l1..3
constexpr int kFsz = 8 * 32 * 256;
constexpr int kF0 = 0;
constexpr int kF1 = kF0 + 8 * 12 * 256;
constexpr int kT0 = kF1 + 3 * kFsz;
constexpr int kT1 = kT0 + 3 * 32 * 256;
constexpr int kPacked = kT1 + 3 * kFsz;

// per-slab partial of the weight-gradient launch (floats)
constexpr int kPW = 0;                  // 4 x [256][256] (layer 0 uses columns < 93)
constexpr int kPB = 4 * kH * kH;        // 4 x [256]
constexpr int kPWo = kPB + 4 * kH;      // [4][256]
constexpr int kPBo = kPWo + 4 * kH;     // [4] (16 reserved)
constexpr int kPFB = kPBo + 16;         // [3][93] (288 reserved)
constexpr int kPart = kPFB + 288;

constexpr int kCP = 64;                 // points per staged chunk of the weight-gradient GEMM
constexpr int kPitch = 66;              // LDS pitch of a staged [feature][64 points] image (column reads)

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_imap_pack(nslam_imap_params P, float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kPacked) return;
  const bool tr = idx >= kT0;
  int l, e, K8;
  if (!tr) {
    if (idx < kF1) {
      l = 0;
      e = idx;
      K8 = 12;
    } else {
      l = 1 + (idx - kF1) / kFsz;
      e = (idx - kF1) % kFsz;
      K8 = 32;
    }
  } else {
    K8 = 32;
    if (idx < kT1) {
      l = 0;
      e = idx - kT0;
    } else {
      l = 1 + (idx - kT1) / kFsz;
      e = (idx - kT1) % kFsz;
    }
  }
  const int j = e & 3, lane = (e >> 2) & 63, q = e >> 8;
  const int s4 = q % K8, ob = q / K8;
  const int row = 32 * ob + (lane & 31), col = 2 * (4 * s4 + j) + (lane >> 5);
  const int in = l == 0 ? kE : kH;  // W_l is [256][in]
  float v = 0.f;
  if (!tr) {
    if (row < kH && col < in) v = P.w[l][row * in + col];
  } else {
    if (col < kH && row < in) v = P.w[l][col * in + row];
  }
  out[idx] = v;
}

// ------------------------------------------------------------------------------------------------
struct IPt {
  float x[3];
  bool valid, inside;
};

// the fused query's point rule (nslam_query_core.h load_point): float64 point, strict inside test, p.float()
__device__ __forceinline__ IPt imap_point(const nslam_imap_query& q, int64_t idx, int64_t n) {
  IPt r;
  r.valid = idx < n;
  const int64_t i = r.valid ? idx : 0;  // tail lanes compute on a real point and write nothing
  double p[3];
  if (!q.pts) {
    const uint32_t ray = (uint32_t)i / (uint32_t)q.n_samples;
    const double z = q.z_vals[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = (double)q.rays_o[ray * 3 + k] + (double)q.rays_d[ray * 3 + k] * z;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = q.pts[i * 3 + k];
  }
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.x[k] = (float)p[k];
    in = in && (p[k] < q.bound_hi[k]) && (p[k] > q.bound_lo[k]);  // Renderer.py:43-46
  }
  r.inside = in;
  return r;
}

// (p.float() @ B)[k]
__device__ __forceinline__ float emb_arg(float x0, float x1, float x2, const float* __restrict__ B, int k) {
  return fmaf(x2, B[2 * kE + k], fmaf(x1, B[kE + k], x0 * B[k]));
}

// acc[pt] += Wfrag * X for the wave's 32 output rows and the tile's four 32-point sub-tiles; K = 8 K8
__device__ __forceinline__ void tile_gemm(f32x16 (&acc)[4], const float* __restrict__ frag, int K8,
                                          const float* X, int lane) {
  const gptr_t<f32x4> f = as_global(reinterpret_cast<const f32x4*>(frag)) + lane;
  const float* xb = X + (lane >> 5) * kTP + (lane & 31);
  for (int s4 = 0; s4 < K8; ++s4) {
    const f32x4 a = f[s4 * 64];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* xr = xb + (s4 * 4 + j) * 2 * kTP;
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[pt] = mfma32(a[j], xr[pt * 32], acc[pt]);
    }
  }
}

// the whole image (or its first `rows` rows) to / from global memory, 16 bytes per thread and step
__device__ __forceinline__ void image_store(float* __restrict__ dst, const float* X, int rows) {
  const f32x4* s = reinterpret_cast<const f32x4*>(X);
  f32x4* d = reinterpret_cast<f32x4*>(dst);
  for (int i = threadIdx.x; i < rows * kTP / 4; i += kThreads) d[i] = s[i];
}

struct FwdArgs {
  nslam_imap_params P;
  const float* packed;
  nslam_imap_query q;
  int64_t n;
  float* raw;
  float* tape;
};

__global__ __launch_bounds__(kThreads) void k_imap_fwd(FwdArgs a) {
  extern __shared__ float smem[];
  float* X = smem;                 // [256][128]
  float* sx = smem + kImg;         // [3][128]
  int* sin_ = reinterpret_cast<int*>(sx + 3 * kTP);  // [128] inside
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int64_t tile = blockIdx.x;
  if (tid < kTP) {
    const IPt p = imap_point(a.q, tile * kTP + tid, a.n);
    sx[tid] = p.x[0];
    sx[kTP + tid] = p.x[1];
    sx[2 * kTP + tid] = p.x[2];
    sin_[tid] = p.inside ? 1 : 0;
  }
  __syncthreads();
  {  // e = sin(x B): thread (point, k mod 4)
    const int p = tid & (kTP - 1), kq = tid >> 7;
    const float x0 = sx[p], x1 = sx[kTP + p], x2 = sx[2 * kTP + p];
    for (int k = kq; k < kEP; k += 4) X[k * kTP + p] = k < kE ? fsin(emb_arg(x0, x1, x2, a.P.B, k)) : 0.f;
  }
  __syncthreads();
  const int h = lane >> 5, pl = lane & 31;
  for (int l = 0; l < 4; ++l) {
    const int K8 = l == 0 ? kEP / 8 : kH / 8;
    const float* frag = a.packed + (l == 0 ? kF0 : kF1 + (l - 1) * kFsz) + w * K8 * 256;
    f32x16 acc[4];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float b = a.P.b[l][32 * w + fidx(r, h)];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[pt][r] = b;
    }
    tile_gemm(acc, frag, K8, X, lane);
    __syncthreads();  // every wave has read the input image
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const f32x16 v = relu16(acc[pt]);
#pragma unroll
      for (int r = 0; r < 16; ++r) X[(32 * w + fidx(r, h)) * kTP + pt * 32 + pl] = v[r];
    }
    __syncthreads();
    if (a.tape) image_store(a.tape + (tile * 4 + l) * (int64_t)kImg, X, kH);
  }
  {  // raw = Wo h4 + bo: thread (point, channel)
    const int p = tid & (kTP - 1), c = tid >> 7;
    float s = a.P.bo[c];
    const float* wo = a.P.wo + c * kH;
    for (int k = 0; k < kH; ++k) s = fmaf(wo[k], X[k * kTP + p], s);
    if (c == 3 && !sin_[p]) s = 100.f;  // Renderer.py:57
    const int64_t idx = tile * kTP + p;
    if (idx < a.n) a.raw[idx * 4 + c] = s;
  }
}

// ------------------------------------------------------------------------------------------------
struct BwdArgs {
  nslam_imap_params P;
  const float* packed;
  nslam_imap_query q;
  int64_t n;
  int64_t ntiles;
  const float* g_raw;
  const float* tape;
  float* G;       // [ntiles][kGTile]
  double* g_pts;
  float* part;    // [nslabs][kPart]
  int nslabs;
};

__global__ __launch_bounds__(kThreads) void k_imap_chain(BwdArgs a) {
  extern __shared__ float smem[];
  float* X = smem;                  // [256][128]
  float* sx = smem + kImg;          // [3][128]
  float* sg = sx + 3 * kTP;         // [4][128] g_raw (density column zeroed out of bound)
  float* sdp = sg + 4 * kTP;        // [4][3][128] partial dp
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int64_t tile = blockIdx.x;
  const float* tape = a.tape + tile * 4 * (int64_t)kImg;
  float* G = a.G + tile * (int64_t)kGTile;
  if (tid < kTP) {
    const int64_t idx = tile * kTP + tid;
    const IPt p = imap_point(a.q, idx, a.n);
    sx[tid] = p.x[0];
    sx[kTP + tid] = p.x[1];
    sx[2 * kTP + tid] = p.x[2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float g = p.valid ? a.g_raw[idx * 4 + c] : 0.f;
      if (c == 3 && !p.inside) g = 0.f;
      sg[c * kTP + tid] = g;
    }
  }
  __syncthreads();
  // G_3 = (Wo^T g) * [h4 > 0]
  for (int i = tid; i < kImg; i += kThreads) {
    const int k = i >> 7, p = i & (kTP - 1);
    float v = sg[p] * a.P.wo[k];
    v = fmaf(sg[kTP + p], a.P.wo[kH + k], v);
    v = fmaf(sg[2 * kTP + p], a.P.wo[2 * kH + k], v);
    v = fmaf(sg[3 * kTP + p], a.P.wo[3 * kH + k], v);
    X[i] = tape[3 * (int64_t)kImg + i] > 0.f ? v : 0.f;
  }
  __syncthreads();
  image_store(G + 3 * kImg, X, kH);
  const int h = lane >> 5, pl = lane & 31;
  for (int l = 3; l >= 1; --l) {  // G_(l-1) = (W_l^T G_l) * [h_l > 0]   (h_l = tape image l-1)
    f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
    tile_gemm(acc, a.packed + kT1 + (l - 1) * kFsz + w * 32 * 256, 32, X, lane);
    __syncthreads();
    const float* hl = tape + (l - 1) * (int64_t)kImg;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = (32 * w + fidx(r, h)) * kTP + pt * 32 + pl;
        X[o] = hl[o] > 0.f ? acc[pt][r] : 0.f;
      }
    }
    __syncthreads();
    image_store(G + (l - 1) * kImg, X, kH);
  }
  {  // de = W_0^T G_0: 96 rows, waves 0..2
    f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
    if (w < 3) tile_gemm(acc, a.packed + kT0 + w * 32 * 256, 32, X, lane);
    __syncthreads();
    if (w < 3) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) X[(32 * w + fidx(r, h)) * kTP + pt * 32 + pl] = acc[pt][r];
      }
    }
    __syncthreads();
  }
  {  // X[k][p] = de * cos(x B);  dp = B (de * cos)
    const int p = tid & (kTP - 1), kq = tid >> 7;
    const float x0 = sx[p], x1 = sx[kTP + p], x2 = sx[2 * kTP + p];
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    for (int k = kq; k < kE; k += 4) {
      const float v = X[k * kTP + p] * fcos(emb_arg(x0, x1, x2, a.P.B, k));
      X[k * kTP + p] = v;
      d0 = fmaf(a.P.B[k], v, d0);
      d1 = fmaf(a.P.B[kE + k], v, d1);
      d2 = fmaf(a.P.B[2 * kE + k], v, d2);
    }
    sdp[(kq * 3 + 0) * kTP + p] = d0;
    sdp[(kq * 3 + 1) * kTP + p] = d1;
    sdp[(kq * 3 + 2) * kTP + p] = d2;
  }
  __syncthreads();
  image_store(G + 4 * kImg, X, kEP);
  if (a.g_pts && tid < kTP) {
    const int64_t idx = tile * kTP + tid;
    if (idx < a.n) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float s = ((sdp[j * kTP + tid] + sdp[(3 + j) * kTP + tid]) + sdp[(6 + j) * kTP + tid]) +
                        sdp[(9 + j) * kTP + tid];
        a.g_pts[idx * 3 + j] = (double)s;
      }
    }
  }
}

// stage 64 points (chunk c of the tile) of a [rows][128] global image as [rows][kPitch]
__device__ __forceinline__ void stage_chunk(float* dst, const float* __restrict__ img, int rows, int c) {
#pragma unroll 4
  for (int i = threadIdx.x; i < rows * kCP; i += kThreads) {
    const int f = i >> 6, p = i & (kCP - 1);
    dst[f * kPitch + p] = img[f * kTP + c * kCP + p];
  }
}

// dW_y += G_y^T-chunk x H-chunk for KB input blocks: wave w owns output rows 32w..32w+31
template <int KB>
__device__ __forceinline__ void wgrad_chunk(f32x16 (&acc)[KB], const float* sA, const float* sH, int w, int lane) {
  const float* pa = sA + (32 * w + (lane & 31)) * kPitch + (lane >> 5);
  const float* pb = sH + (lane & 31) * kPitch + (lane >> 5);
#pragma unroll 2
  for (int s = 0; s < kCP / 2; ++s) {
    const float av = pa[2 * s];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) acc[kb] = mfma32(av, pb[kb * 32 * kPitch + 2 * s], acc[kb]);
  }
}

// input blocks kb0 .. kb0+KB-1 of layer y; the workgroup with kb0 = 0 also sums the bias gradient
template <int KB>
__device__ __forceinline__ void wgrad_layer(const BwdArgs& a, int y, int kb0, float* sA, float* sH, float* sx) {
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  f32x16 acc[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) acc[kb] = zero16();
  float bsum = 0.f;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += a.nslabs) {
    const float* G = a.G + tile * (int64_t)kGTile + y * kImg;
    for (int c = 0; c < kTP / kCP; ++c) {
      __syncthreads();  // the previous chunk's reads are done
      stage_chunk(sA, G, kH, c);
      if (y > 0) {
        stage_chunk(sH, a.tape + (tile * 4 + (y - 1)) * (int64_t)kImg + kb0 * 32 * kTP, KB * 32, c);
      } else {  // the layer's input is the embedding, recomputed
        if (tid < kCP) {
          const IPt p = imap_point(a.q, tile * kTP + c * kCP + tid, a.n);
          sx[tid] = p.x[0];
          sx[kCP + tid] = p.x[1];
          sx[2 * kCP + tid] = p.x[2];
        }
        __syncthreads();
        const int p = tid & (kCP - 1), kq = tid >> 6;
        const float x0 = sx[p], x1 = sx[kCP + p], x2 = sx[2 * kCP + p];
        for (int k = kq; k < kEP; k += 8) sH[k * kPitch + p] = k < kE ? fsin(emb_arg(x0, x1, x2, a.P.B, k)) : 0.f;
      }
      __syncthreads();
      wgrad_chunk<KB>(acc, sA, sH, w, lane);
      if (kb0 == 0 && tid < kH) {
        const float* row = sA + tid * kPitch;
#pragma unroll 4
        for (int p = 0; p < kCP; ++p) bsum += row[p];
      }
    }
  }
  float* part = a.part + blockIdx.x * (int64_t)kPart;
  asm volatile("" : "+v"(part));  // the 16 KB store addresses are formed here, not hoisted above the GEMM loop
  const int h = lane >> 5, j = lane & 31;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) part[kPW + y * kH * kH + (32 * w + fidx(r, h)) * kH + (kb0 + kb) * 32 + j] = acc[kb][r];
  }
  if (kb0 == 0 && tid < kH) part[kPB + y * kH + tid] = bsum;
}

// output layer (dWo = sum_p g h4, dbo = sum_p g) and the embedding matrix (dB[j][k] = sum_p x_j de_k cos_k)
__device__ __forceinline__ void wgrad_tail(const BwdArgs& a, float* sA, float* sH, float* sx) {
  const int tid = threadIdx.x;
  const int k = tid & (kH - 1), c0 = (tid >> 8) * 2;
  float a0 = 0.f, a1 = 0.f, bo = 0.f, fb = 0.f;
  const int fj = tid / kE, fk = tid % kE;  // tid < 279: dB[fj][fk]
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += a.nslabs) {
    for (int c = 0; c < kTP / kCP; ++c) {
      __syncthreads();
      stage_chunk(sH, a.tape + (tile * 4 + 3) * (int64_t)kImg, kH, c);
      if (tid < kCP) {
        const int64_t idx = tile * kTP + c * kCP + tid;
        const IPt p = imap_point(a.q, idx, a.n);
        sx[tid] = p.x[0];
        sx[kCP + tid] = p.x[1];
        sx[2 * kCP + tid] = p.x[2];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
          float g = p.valid ? a.g_raw[idx * 4 + ch] : 0.f;
          if (ch == 3 && !p.inside) g = 0.f;
          sA[ch * kPitch + tid] = g;
        }
      }
      __syncthreads();
      {
        const float* hr = sH + k * kPitch;
        const float* g0 = sA + c0 * kPitch;
        const float* g1 = g0 + kPitch;
#pragma unroll 4
        for (int p = 0; p < kCP; ++p) {
          a0 = fmaf(g0[p], hr[p], a0);
          a1 = fmaf(g1[p], hr[p], a1);
        }
      }
      if (tid < 4) {
        const float* g = sA + tid * kPitch;
#pragma unroll 4
        for (int p = 0; p < kCP; ++p) bo += g[p];
      }
      __syncthreads();
      stage_chunk(sH, a.G + tile * (int64_t)kGTile + 4 * kImg, kEP, c);  // de * cos
      __syncthreads();
      if (tid < 3 * kE) {
        const float* dr = sH + fk * kPitch;
        const float* xr = sx + fj * kCP;
#pragma unroll 4
        for (int p = 0; p < kCP; ++p) fb = fmaf(xr[p], dr[p], fb);
      }
    }
  }
  float* part = a.part + blockIdx.x * (int64_t)kPart;
  part[kPWo + c0 * kH + k] = a0;
  part[kPWo + (c0 + 1) * kH + k] = a1;
  if (tid < 4) part[kPBo + tid] = bo;
  if (tid < 3 * kE) part[kPFB + tid] = fb;
}

// grid (nslabs, 8): y = 0 layer 0; y = 1..6 the two 128-column halves of layers 1..3; y = 7 the output layer and B
__global__ __launch_bounds__(kThreads) void k_imap_wgrad(BwdArgs a) {
  extern __shared__ float smem[];
  float* sA = smem;                    // [256][kPitch]
  float* sH = sA + kH * kPitch;        // [256][kPitch]
  float* sx = sH + kH * kPitch;        // [3][64]
  const int y = blockIdx.y;
  if (y == 0)
    wgrad_layer<3>(a, 0, 0, sA, sH, sx);
  else if (y < 7)
    wgrad_layer<4>(a, 1 + (y - 1) / 2, 4 * ((y - 1) & 1), sA, sH, sx);
  else
    wgrad_tail(a, sA, sH, sx);
}

// grads += sum over slabs (in slab order) of the partials
__global__ __launch_bounds__(256) void k_imap_reduce(const float* __restrict__ part, int nslabs, nslam_imap_grads g) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kPart) return;
  float* dst = nullptr;
  if (idx < kPB) {
    const int y = idx >> 16, o = (idx >> 8) & 255, k = idx & 255;
    if (y == 0) {
      if (k < kE) dst = g.w[0] + o * kE + k;
    } else {
      dst = g.w[y] + o * kH + k;
    }
  } else if (idx < kPWo) {
    const int e = idx - kPB;
    dst = g.b[e >> 8] + (e & 255);
  } else if (idx < kPBo) {
    dst = g.wo + (idx - kPWo);
  } else if (idx < kPFB) {
    if (idx - kPBo < 4) dst = g.bo + (idx - kPBo);
  } else {
    if (idx - kPFB < 3 * kE) dst = g.B + (idx - kPFB);
  }
  if (!dst) return;
  float s = 0.f;
  for (int i = 0; i < nslabs; ++i) s += part[(int64_t)i * kPart + idx];
  *dst += s;
}

constexpr size_t kFwdLds = (size_t)(kImg + 3 * kTP + kTP) * 4;
constexpr size_t kChainLds = (size_t)(kImg + 3 * kTP + 4 * kTP + 12 * kTP) * 4;
constexpr size_t kWgradLds = (size_t)(2 * kH * kPitch + 3 * kCP) * 4;

int64_t tiles_of(int64_t n) { return (n + kTP - 1) / kTP; }
int slabs_of(int64_t ntiles) { return (int)std::min<int64_t>(ntiles, kMaxSlabs); }

bool params_ok(const nslam_imap_params* p) {
  if (!p || !p->B || !p->wo || !p->bo) return false;
  for (int i = 0; i < 4; ++i)
    if (!p->w[i] || !p->b[i]) return false;
  return true;
}
bool query_ok(const nslam_imap_query* q) {
  if (!q) return false;
  if (q->pts) return true;
  return q->rays_o && q->rays_d && q->z_vals && q->n_samples > 0;
}
bool set_lds(const void* fn, size_t bytes) {
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

}  // namespace

extern "C" size_t nslam_imap_packed_size(void) { return (size_t)kPacked * sizeof(float); }

extern "C" int nslam_imap_pack(const nslam_imap_params* params, float* packed, void* stream) {
  if (!params_ok(params) || !packed) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_imap_pack, dim3((kPacked + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     *params, packed);
  return hip_status();
}

extern "C" size_t nslam_imap_tape_size(int64_t n) {
  return n <= 0 ? 0 : (size_t)tiles_of(n) * 4 * kImg * sizeof(float);
}

extern "C" int nslam_imap_fwd(const nslam_imap_params* params, const float* packed, const nslam_imap_query* q,
                              int64_t n, float* raw, void* tape, void* stream) {
  if (n < 0 || !params_ok(params) || !packed) return NSLAM_EINVAL;
  if (n >= ((int64_t)1 << 31)) return NSLAM_EUNSUPPORTED;
  if (n == 0) return NSLAM_OK;
  if (!query_ok(q) || !raw) return NSLAM_EINVAL;
  if (!set_lds(reinterpret_cast<const void*>(k_imap_fwd), kFwdLds)) return hip_status();
  FwdArgs a{*params, packed, *q, n, raw, reinterpret_cast<float*>(tape)};
  hipLaunchKernelGGL(k_imap_fwd, dim3((unsigned)tiles_of(n)), dim3(kThreads), kFwdLds,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" size_t nslam_imap_bwd_workspace_size(int64_t n) {
  if (n <= 0) return 0;
  const int64_t nt = tiles_of(n);
  return ((size_t)nt * kGTile + (size_t)slabs_of(nt) * kPart) * sizeof(float);
}

extern "C" int nslam_imap_bwd(const nslam_imap_params* params, const float* packed, const nslam_imap_query* q,
                              int64_t n, const float* g_raw, const void* tape, const nslam_imap_grads* grads,
                              double* g_pts, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || !params_ok(params) || !packed) return NSLAM_EINVAL;
  if (n >= ((int64_t)1 << 31)) return NSLAM_EUNSUPPORTED;
  if (n == 0) return NSLAM_OK;
  if (!query_ok(q) || !g_raw || !tape) return NSLAM_EINVAL;
  if (grads) {
    if (!grads->B || !grads->wo || !grads->bo) return NSLAM_EINVAL;
    for (int i = 0; i < 4; ++i)
      if (!grads->w[i] || !grads->b[i]) return NSLAM_EINVAL;
  }
  if (!ws || ws_bytes < nslam_imap_bwd_workspace_size(n)) return NSLAM_EWORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BwdArgs a{};
  a.P = *params;
  a.packed = packed;
  a.q = *q;
  a.n = n;
  a.ntiles = tiles_of(n);
  a.g_raw = g_raw;
  a.tape = reinterpret_cast<const float*>(tape);
  a.G = reinterpret_cast<float*>(ws);
  a.g_pts = g_pts;
  a.nslabs = slabs_of(a.ntiles);
  a.part = a.G + a.ntiles * (int64_t)kGTile;
  if (!set_lds(reinterpret_cast<const void*>(k_imap_chain), kChainLds)) return hip_status();
  hipLaunchKernelGGL(k_imap_chain, dim3((unsigned)a.ntiles), dim3(kThreads), kChainLds, s, a);
  if (grads) {
    if (!set_lds(reinterpret_cast<const void*>(k_imap_wgrad), kWgradLds)) return hip_status();
    hipLaunchKernelGGL(k_imap_wgrad, dim3((unsigned)a.nslabs, 8), dim3(kThreads), kWgradLds, s, a);
    hipLaunchKernelGGL(k_imap_reduce, dim3((kPart + 255) / 256), dim3(256), 0, s, a.part, a.nslabs, *grads);
  }
  return hip_status();
}
