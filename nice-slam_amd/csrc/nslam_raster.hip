// nslam_raster.hip — the depth images of eval_recon.py's 2D metric (calc_2d_metric, :131-210): a triangle mesh seen
// from a batch of pinhole cameras, in place of the reference's open3d OpenGL window
// (capture_depth_float_buffer(True) with mesh_show_back_face).
//   nslam_raster_depth            float32 [B][H][W]: camera-space z of the nearest triangle along the ray through
//                                 each pixel centre, 0 where nothing is hit
//   nslam_raster_workspace_size   bytes of a workspace whose list of large items holds `capacity` entries
// Work: one thread per (face, view) transforms the face's vertices (float64), rejects it or takes the pixel box
// of its near-clipped projection, tests a box of at most small_max_pixels pixels itself and appends a larger one
// to a list (one returning atomic per wave); a second launch gives every listed item a workgroup.  A full list
// drops nothing: the producing thread tests its box itself.  Every hit is rounded to float32 once and combined
// with an integer atomicMin on the float's bits (positive floats order as their bits): min does not depend on
// the order, so the image is bit-identical from run to run and across the paths — the one use of atomics in the
// evaluation module.  The build has -ffp-contract=off: b x c is the exact negation of c x b, so the two
// triangles at a shared edge see the same edge function with opposite signs and leave no crack.
#include <math.h>

#include "nslam_dev.h"

namespace {

constexpr int kRasterThreads = 256;
constexpr uint32_t kInfBits = 0x7f800000u;  // +inf: above every depth
constexpr double kBoxPad = 1e-4;            // pixels added round the box: its rounding must not cost a pixel centre
constexpr int kBigBlocks = 8192;            // workgroups of the list pass (each strides over the list)

struct RasterHead {  // the first 16 bytes of the workspace
  unsigned long long count;  // items appended (may pass the capacity: the excess was drawn by its producer)
  unsigned long long pad_;
};
struct RasterItem {
  int32_t face, view;
};

struct RasterArgs {
  const double* verts;   // [nv][3]
  const int32_t* faces;  // [nf][3]
  const double* w2c;     // [B][12] row-major [3][4]
  int64_t nv, nf;
  int32_t B, H, W;
  double fx, fy, cx, cy, zn, zf;
  int64_t small_max;
  uint32_t* depth;  // [B][H][W] float bits
  RasterHead* head;
  RasterItem* items;
  unsigned long long cap;
};

// one face under one view: the edge functions' normals (b x c, c x a, a x b of the camera-space vertices: the
// ray direction d gives the unnormalised barycentrics d . n), the vertices' z and the pixel box
struct Tri {
  double na[3], nb[3], nc[3];
  double az, bz, cz;
  int32_t x0, x1, y0, y1;
};

__device__ __forceinline__ bool finite3(const double* p) {
  return (p[0] - p[0] == 0.0) & (p[1] - p[1] == 0.0) & (p[2] - p[2] == 0.0);
}

__device__ __forceinline__ void cross3(const double* p, const double* q, double* o) {
  o[0] = p[1] * q[2] - p[2] * q[1];
  o[1] = p[2] * q[0] - p[0] * q[2];
  o[2] = p[0] * q[1] - p[1] * q[0];
}

// false: the face draws nothing in this view (bad index, non-finite vertex, zero area, outside the depth range,
// or its box holds no pixel).  Both passes call this and shade(), so they compute the same numbers.
__device__ __forceinline__ bool setup(const RasterArgs& a, int64_t f, int32_t view, Tri& t) {
  const gptr_t<int32_t> idx = as_global(a.faces) + 3 * f;
  const int32_t i0 = idx[0], i1 = idx[1], i2 = idx[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.nv || i1 >= a.nv || i2 >= a.nv) return false;
  double p[3][3];
  const gptr_t<double> v = as_global(a.verts);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    p[0][d] = v[3 * (int64_t)i0 + d];
    p[1][d] = v[3 * (int64_t)i1 + d];
    p[2][d] = v[3 * (int64_t)i2 + d];
  }
  if (!(finite3(p[0]) && finite3(p[1]) && finite3(p[2]))) return false;
  {  // zero area, in world space: exact for coincident and exactly collinear vertices
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    double n[3];
    cross3(e1, e2, n);
    if (!((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2] > 0.0)) return false;
  }
  const gptr_t<double> m = as_global(a.w2c) + 12 * (int64_t)view;
  double c[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      c[k][r] = ((m[4 * r] * p[k][0] + m[4 * r + 1] * p[k][1]) + m[4 * r + 2] * p[k][2]) + m[4 * r + 3];
  if (!(finite3(c[0]) && finite3(c[1]) && finite3(c[2]))) return false;
  const double zmin = fmin(fmin(c[0][2], c[1][2]), c[2][2]), zmax = fmax(fmax(c[0][2], c[1][2]), c[2][2]);
  if (!(zmax > a.zn) || !(zmin <= a.zf)) return false;  // a hit needs zn < z <= zf
  // the pixel box of the part of the triangle at z >= zn: its vertices there, and where its edges cross zn
  double minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* s = c[k];
    const double* e = c[(k + 1) % 3];
    const bool s_in = s[2] >= a.zn, e_in = e[2] >= a.zn;
    double px, py;
    if (s_in) {
      px = a.fx * (s[0] / s[2]) + a.cx;
      py = a.fy * (s[1] / s[2]) + a.cy;
      nan |= (px != px) | (py != py);
      minx = fmin(minx, px), maxx = fmax(maxx, px), miny = fmin(miny, py), maxy = fmax(maxy, py);
    }
    if (s_in != e_in) {
      const double w = (a.zn - s[2]) / (e[2] - s[2]);
      px = a.fx * ((s[0] + w * (e[0] - s[0])) / a.zn) + a.cx;
      py = a.fy * ((s[1] + w * (e[1] - s[1])) / a.zn) + a.cy;
      nan |= (px != px) | (py != py);
      minx = fmin(minx, px), maxx = fmax(maxx, px), miny = fmin(miny, py), maxy = fmax(maxy, py);
    }
  }
  if (nan) {  // no usable projection (zn = 0 with a vertex on the camera plane): the whole image
    minx = miny = -INFINITY;
    maxx = maxy = INFINITY;
  }
  // clamped in double BEFORE the conversion: after this 0 <= lo <= hi <= size - 1 whatever the coordinates were
  double fx0 = ceil(minx - kBoxPad), fx1 = floor(maxx + kBoxPad);
  double fy0 = ceil(miny - kBoxPad), fy1 = floor(maxy + kBoxPad);
  fx0 = !(fx0 > 0.0) ? 0.0 : fx0;
  fy0 = !(fy0 > 0.0) ? 0.0 : fy0;
  fx1 = !(fx1 < (double)(a.W - 1)) ? (double)(a.W - 1) : fx1;
  fy1 = !(fy1 < (double)(a.H - 1)) ? (double)(a.H - 1) : fy1;
  if (!(fx0 <= fx1) || !(fy0 <= fy1)) return false;  // covers no pixel centre (most faces end here)
  t.x0 = (int32_t)fx0;
  t.x1 = (int32_t)fx1;
  t.y0 = (int32_t)fy0;
  t.y1 = (int32_t)fy1;
  cross3(c[1], c[2], t.na);
  cross3(c[2], c[0], t.nb);
  cross3(c[0], c[1], t.nc);
  t.az = c[0][2];
  t.bz = c[1][2];
  t.cz = c[2][2];
  return true;
}

// the ray through the centre of pixel (x, y) against the triangle: inside when the three edge functions share a
// sign (zero included: both faces are visible, edges are inclusive), z = the barycentric mean of the vertices' z
__device__ __forceinline__ void shade(const RasterArgs& a, const Tri& t, uint32_t* img, int32_t x, int32_t y) {
  const double dx = ((double)x - a.cx) / a.fx, dy = ((double)y - a.cy) / a.fy;
  const double wa = (dx * t.na[0] + dy * t.na[1]) + t.na[2];
  const double wb = (dx * t.nb[0] + dy * t.nb[1]) + t.nb[2];
  const double wc = (dx * t.nc[0] + dy * t.nc[1]) + t.nc[2];
  const double sum = (wa + wb) + wc;
  const bool pos = (wa >= 0.0) & (wb >= 0.0) & (wc >= 0.0), neg = (wa <= 0.0) & (wb <= 0.0) & (wc <= 0.0);
  if (!(pos | neg) || sum == 0.0) return;  // NaN is neither
  const double z = ((wa * t.az + wb * t.bz) + wc * t.cz) / sum;
  if (!(z > a.zn) || !(z <= a.zf)) return;
  const uint32_t bits = __float_as_uint((float)z);
  uint32_t* p = img + ((int64_t)y * a.W + x);
  // the stored depth only ever falls, so a value read before the atomic can only be too large: a hit that is
  // not below it is not below the current one either
  if (bits < *as_global(p)) atomicMin(p, bits);
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_clear(uint32_t* depth, int64_t n, RasterHead* head) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i < n) depth[i] = kInfBits;
  if (i == 0) head->count = 0;
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_small(RasterArgs a) {
  const int64_t f = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  const int32_t view = blockIdx.y;
  Tri t;
  bool live = f < a.nf && setup(a, f, view, t);
  const int64_t npx = live ? (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) : 0;
  const bool big = live && npx > a.small_max;
  // every lane of the wave reaches the ballot (no lane has returned): one returning atomic for all its appends
  const unsigned long long mask = __ballot(big);
  if (mask != 0) {
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll(mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&a.head->count, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (big) {
      const unsigned long long slot = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
      if (slot < a.cap) {
        RasterItem it;
        it.face = (int32_t)f;
        it.view = view;
        a.items[slot] = it;
        live = false;  // the list pass draws it
      }  // else the list is full: drawn here, slowly, but drawn
    }
  }
  if (!live) return;
  uint32_t* img = a.depth + (int64_t)view * a.H * a.W;
  for (int32_t y = t.y0; y <= t.y1; ++y)
    for (int32_t x = t.x0; x <= t.x1; ++x) shade(a, t, img, x, y);
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_big(RasterArgs a) {
  unsigned long long n = a.head->count;  // written by the launch before this one
  if (n > a.cap) n = a.cap;
  for (unsigned long long i = blockIdx.x; i < n; i += gridDim.x) {
    const RasterItem it = a.items[i];
    if (it.face < 0 || it.face >= a.nf || it.view < 0 || it.view >= a.B) continue;
    Tri t;
    if (!setup(a, it.face, it.view, t)) continue;  // the same answer in every thread
    const int32_t bw = t.x1 - t.x0 + 1;
    const int32_t npx = bw * (t.y1 - t.y0 + 1);  // <= H W < 2^31 (checked by the entry point)
    uint32_t* img = a.depth + (int64_t)it.view * a.H * a.W;
    for (int32_t p = threadIdx.x; p < npx; p += kRasterThreads) shade(a, t, img, t.x0 + p % bw, t.y0 + p / bw);
  }
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_resolve(uint32_t* depth, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i < n && depth[i] >= kInfBits) depth[i] = 0u;  // no hit (or a depth that overflowed float32): background
}

inline bool finite_h(double v) { return v - v == 0.0; }

}  // namespace

extern "C" size_t nslam_raster_workspace_size(int64_t capacity) {
  if (capacity < 1) capacity = 1;
  return sizeof(RasterHead) + (size_t)capacity * sizeof(RasterItem);
}

extern "C" int nslam_raster_depth(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                  const double* w2c, int32_t n_views, int32_t H, int32_t W, double fx, double fy,
                                  double cx, double cy, double z_near, double z_far, int64_t small_max_pixels,
                                  int32_t passes, float* depth, void* ws, size_t ws_bytes, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_views < 0 || H <= 0 || W <= 0 || small_max_pixels < 0) return NSLAM_EINVAL;
  if (!(fx > 0.0) || !(fy > 0.0) || !finite_h(fx) || !finite_h(fy) || !finite_h(cx) || !finite_h(cy))
    return NSLAM_EINVAL;
  if (!(z_near >= 0.0) || !(z_near < z_far)) return NSLAM_EINVAL;  // NaN fails both
  if (passes < 0 || passes > NSLAM_RASTER_ALL) return NSLAM_EINVAL;
  if ((int64_t)H * W >= (int64_t(1) << 31) || n_verts >= (int64_t(1) << 31) || n_faces >= (int64_t(1) << 31))
    return NSLAM_EINVAL;
  if (n_views == 0 || n_faces == 0) return NSLAM_OK;  // nothing to draw: no launch, depth is not written
  if (!verts || !faces || !w2c || !depth || !ws || n_verts == 0) return NSLAM_EINVAL;
  if (ws_bytes < nslam_raster_workspace_size(1)) return NSLAM_EINVAL;
  if (n_views > 65535) return NSLAM_EUNSUPPORTED;  // one grid row per view
  RasterArgs a{};
  a.verts = verts;
  a.faces = faces;
  a.w2c = w2c;
  a.nv = n_verts;
  a.nf = n_faces;
  a.B = n_views;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.zn = z_near;
  a.zf = z_far;
  a.small_max = small_max_pixels;
  a.depth = reinterpret_cast<uint32_t*>(depth);
  a.head = reinterpret_cast<RasterHead*>(ws);
  a.items = reinterpret_cast<RasterItem*>(reinterpret_cast<char*>(ws) + sizeof(RasterHead));
  a.cap = (ws_bytes - sizeof(RasterHead)) / sizeof(RasterItem);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t n_pix = (int64_t)n_views * H * W;
  const int64_t pix_blocks = (n_pix + kRasterThreads - 1) / kRasterThreads;
  const int64_t face_blocks = (n_faces + kRasterThreads - 1) / kRasterThreads;
  if (pix_blocks >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  if (passes & NSLAM_RASTER_CLEAR)
    hipLaunchKernelGGL(k_raster_clear, dim3((unsigned)pix_blocks), dim3(kRasterThreads), 0, s, a.depth, n_pix, a.head);
  if (passes & NSLAM_RASTER_SMALL)
    hipLaunchKernelGGL(k_raster_small, dim3((unsigned)face_blocks, (unsigned)n_views), dim3(kRasterThreads), 0, s, a);
  if (passes & NSLAM_RASTER_BIG) {
    const unsigned blocks = (unsigned)(a.cap < (unsigned long long)kBigBlocks ? a.cap : kBigBlocks);
    hipLaunchKernelGGL(k_raster_big, dim3(blocks), dim3(kRasterThreads), 0, s, a);
  }
  if (passes & NSLAM_RASTER_RESOLVE)
    hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)pix_blocks), dim3(kRasterThreads), 0, s, a.depth, n_pix);
  return hip_status();
}
