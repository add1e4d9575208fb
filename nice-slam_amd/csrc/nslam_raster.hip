// nslam_raster.hip — the depth images of eval_recon.py's 2D metric (calc_2d_metric, :131-210): a triangle mesh seen
// from a batch of pinhole cameras, in place of the reference's open3d OpenGL window
// (capture_depth_float_buffer(True) with mesh_show_back_face).
//   nslam_raster_depth            float32 [B][H][W]: camera-space z of the nearest triangle along the ray through
//                                 each pixel centre, 0 where nothing is hit
//   nslam_raster_workspace_size   bytes of a workspace whose list of large items holds `capacity` entries
//   nslam_scene_render            visualizer.py's frames (src/tools/viz.py) in place of its open3d window: the mesh
//                                 with vertex colours under a head light plus depth-tested point sprites, uint8
//                                 [B][H][W][3]; the faces take the depth rasteriser's path, a hit is the 64-bit
//                                 key (float32 bits of z) << 32 | id, combined with a 64-bit atomicMin (below)
//   nslam_scene_workspace_size    that workspace: the list plus one key per pixel
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
  // nslam_scene_render only
  unsigned long long* keys;  // [B][H][W]
  int32_t cull;
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
// sign (zero included: both faces are visible, edges are inclusive), z = the barycentric mean of the vertices' z.
// The edge functions over their sum are the barycentrics of the hit (of vertex a, b, c).
struct Hit {
  double wa, wb, wc, sum, z;
};
__device__ __forceinline__ bool hit(const RasterArgs& a, const Tri& t, int32_t x, int32_t y, Hit& h) {
  const double dx = ((double)x - a.cx) / a.fx, dy = ((double)y - a.cy) / a.fy;
  h.wa = (dx * t.na[0] + dy * t.na[1]) + t.na[2];
  h.wb = (dx * t.nb[0] + dy * t.nb[1]) + t.nb[2];
  h.wc = (dx * t.nc[0] + dy * t.nc[1]) + t.nc[2];
  h.sum = (h.wa + h.wb) + h.wc;
  const bool pos = (h.wa >= 0.0) & (h.wb >= 0.0) & (h.wc >= 0.0), neg = (h.wa <= 0.0) & (h.wb <= 0.0) & (h.wc <= 0.0);
  if (!(pos | neg) || h.sum == 0.0) return false;  // NaN is neither
  h.z = ((h.wa * t.az + h.wb * t.bz) + h.wc * t.cz) / h.sum;
  return (h.z > a.zn) && (h.z <= a.zf);
}

// the smaller key wins: the nearer float32 z, at equal z the lower id.  The stored key only ever falls, so a value
// read before the atomic can only be too large: a hit that is not below it is not below the current one either
__device__ __forceinline__ void key_min(unsigned long long* p, unsigned long long key) {
  if (key < *as_global(p)) atomicMin(p, key);
}

// one pixel of one face.  KEY false: the depth image (atomicMin on the float's bits).  KEY true: the scene's key
// image; the sign of the edge-function sum is the side the camera sees (sum = d . (b - a) x (c - a): negative
// when the right-hand normal faces the camera, the front)
template <bool KEY>
__device__ __forceinline__ void shade(const RasterArgs& a, const Tri& t, int64_t base, int32_t x, int32_t y,
                                      int32_t face) {
  Hit h;
  if (!hit(a, t, x, y, h)) return;
  const uint32_t bits = __float_as_uint((float)h.z);
  const int64_t px = base + ((int64_t)y * a.W + x);
  if (KEY) {
    if ((a.cull == NSLAM_CULL_BACK && h.sum > 0.0) || (a.cull == NSLAM_CULL_FRONT && h.sum < 0.0)) return;
    key_min(a.keys + px, ((unsigned long long)bits << 32) | (uint32_t)face);
  } else {
    uint32_t* p = a.depth + px;
    // the stored depth only ever falls, so a value read before the atomic can only be too large: a hit that is
    // not below it is not below the current one either
    if (bits < *as_global(p)) atomicMin(p, bits);
  }
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_clear(uint32_t* depth, int64_t n, RasterHead* head) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i < n) depth[i] = kInfBits;
  if (i == 0) head->count = 0;
}

template <bool KEY>
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
  const int64_t base = (int64_t)view * a.H * a.W;
  for (int32_t y = t.y0; y <= t.y1; ++y)
    for (int32_t x = t.x0; x <= t.x1; ++x) shade<KEY>(a, t, base, x, y, (int32_t)f);
}

template <bool KEY>
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
    const int64_t base = (int64_t)it.view * a.H * a.W;
    for (int32_t p = threadIdx.x; p < npx; p += kRasterThreads)
      shade<KEY>(a, t, base, t.x0 + p % bw, t.y0 + p / bw, it.face);
  }
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_resolve(uint32_t* depth, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i < n && depth[i] >= kInfBits) depth[i] = 0u;  // no hit (or a depth that overflowed float32): background
}

// ---- the scene renderer: the same face passes on a key image, point sprites, and a resolve that shades ----
constexpr unsigned long long kNoKey = ~0ull;  // above every key
constexpr uint32_t kPointBit = 0x80000000u;   // ids of points: above every face index, so a face wins a tie

struct SceneArgs {
  const uint8_t* vcol;  // [nv][3] or null: grey
  const void* vnrm;     // [nv][3] float32 or float64
  int32_t nrm_f64;
  const double* pts;    // [np][3]
  const uint8_t* pcol;  // [np][3]
  int64_t np;
  double half;  // half the sprite's edge in pixels
  double ambient;
  uint8_t grey[3], bg[3];
  uint8_t* color;  // [B][H][W][3]
  float* depth;    // [B][H][W] or null
  int32_t* ids;    // [B][H][W] or null
};

__global__ __launch_bounds__(kRasterThreads) void k_scene_clear(unsigned long long* keys, int64_t n, RasterHead* head) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i < n) keys[i] = kNoKey;
  if (i == 0) head->count = 0;
}

// one thread per (point, view): the square of pixel centres round the projection, all at the point's z
__global__ __launch_bounds__(kRasterThreads) void k_scene_points(RasterArgs a, SceneArgs s) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  const int32_t view = blockIdx.y;
  if (i >= s.np) return;
  const gptr_t<double> q = as_global(s.pts) + 3 * i;
  const double p[3] = {q[0], q[1], q[2]};
  if (!finite3(p)) return;
  const gptr_t<double> m = as_global(a.w2c) + 12 * (int64_t)view;
  double c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
  if (!finite3(c) || !(c[2] > a.zn) || !(c[2] <= a.zf)) return;
  const double px = a.fx * (c[0] / c[2]) + a.cx, py = a.fy * (c[1] / c[2]) + a.cy;
  if (px != px || py != py) return;
  // pixel centres x with px - s/2 <= x < px + s/2; clamped in double BEFORE the conversion (setup's rule)
  double fx0 = ceil(px - s.half), fx1 = ceil(px + s.half) - 1.0;
  double fy0 = ceil(py - s.half), fy1 = ceil(py + s.half) - 1.0;
  fx0 = !(fx0 > 0.0) ? 0.0 : fx0;
  fy0 = !(fy0 > 0.0) ? 0.0 : fy0;
  fx1 = !(fx1 < (double)(a.W - 1)) ? (double)(a.W - 1) : fx1;
  fy1 = !(fy1 < (double)(a.H - 1)) ? (double)(a.H - 1) : fy1;
  if (!(fx0 <= fx1) || !(fy0 <= fy1)) return;
  const uint32_t bits = __float_as_uint((float)c[2]);
  const unsigned long long key = ((unsigned long long)bits << 32) | (kPointBit | (uint32_t)i);
  unsigned long long* img = a.keys + (int64_t)view * a.H * a.W;
  const int32_t x0 = (int32_t)fx0, x1 = (int32_t)fx1, y0 = (int32_t)fy0, y1 = (int32_t)fy1;
  for (int32_t y = y0; y <= y1; ++y)
    for (int32_t x = x0; x <= x1; ++x) key_min(img + ((int64_t)y * a.W + x), key);
}

__device__ __forceinline__ uint8_t level(double v) {  // round half up, NaN and negatives to 0
  const double r = floor(v + 0.5);
  return !(r > 0.0) ? (uint8_t)0 : (r >= 255.0 ? (uint8_t)255 : (uint8_t)r);
}

// one thread per pixel: the key's colour, depth and id
__global__ __launch_bounds__(kRasterThreads) void k_scene_resolve(RasterArgs a, SceneArgs s, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = a.keys[i];
  const uint32_t bits = (uint32_t)(key >> 32), low = (uint32_t)key;
  uint8_t rgb[3] = {s.bg[0], s.bg[1], s.bg[2]};
  uint32_t zbits = 0u;
  int32_t id = -1;
  if (key != kNoKey && bits < kInfBits) {  // else no hit (or a depth that overflowed float32): background
    zbits = bits;
    if (low & kPointBit) {
      const int64_t pi = (int64_t)(low & ~kPointBit);
      id = -2 - (int32_t)pi;
      const gptr_t<uint8_t> pc = as_global(s.pcol) + 3 * pi;
      rgb[0] = pc[0], rgb[1] = pc[1], rgb[2] = pc[2];
    } else {
      id = (int32_t)low;
      const int64_t hw = (int64_t)a.H * a.W;
      const int32_t view = (int32_t)(i / hw);
      const int64_t rem = i - (int64_t)view * hw;
      const int32_t y = (int32_t)(rem / a.W), x = (int32_t)(rem - (int64_t)y * a.W);
      Tri t;
      Hit h;
      // the visibility pass's numbers again: it drew this pixel, so both succeed
      if (setup(a, id, view, t) && hit(a, t, x, y, h)) {
        const double b[3] = {h.wa / h.sum, h.wb / h.sum, h.wc / h.sum};
        const gptr_t<int32_t> idx = as_global(a.faces) + 3 * (int64_t)id;
        double col[3] = {0.0, 0.0, 0.0}, nrm[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int64_t v = idx[k];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const double cv = s.vcol ? (double)as_global(s.vcol)[3 * v + d] : (double)s.grey[d];
            const double nv = s.nrm_f64 ? as_global((const double*)s.vnrm)[3 * v + d]
                                        : (double)as_global((const float*)s.vnrm)[3 * v + d];
            col[d] = col[d] + b[k] * cv;
            nrm[d] = nrm[d] + b[k] * nv;
          }
        }
        // the ray's direction in the world: the transpose of the view's rotation on (dx, dy, 1)
        const double dx = ((double)x - a.cx) / a.fx, dy = ((double)y - a.cy) / a.fy;
        const gptr_t<double> m = as_global(a.w2c) + 12 * (int64_t)view;
        double dw[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) dw[j] = (m[j] * dx + m[4 + j] * dy) + m[8 + j];
        const double nn = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2];
        const double dd = (dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2];
        double cosv = 1.0;  // a zero-length (or NaN) normal: fully lit
        if (nn > 0.0 && dd > 0.0) {
          cosv = fabs((nrm[0] * dw[0] + nrm[1] * dw[1]) + nrm[2] * dw[2]) / (sqrt(nn) * sqrt(dd));
          if (!(cosv <= 1.0)) cosv = 1.0;
        }
        const double k = s.ambient + (1.0 - s.ambient) * cosv;
#pragma unroll
        for (int d = 0; d < 3; ++d) rgb[d] = level(col[d] * k);
      }
    }
  }
  uint8_t* o = s.color + 3 * i;
  o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
  if (s.depth) s.depth[i] = __uint_as_float(zbits);
  if (s.ids) s.ids[i] = id;
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
    hipLaunchKernelGGL(k_raster_small<false>, dim3((unsigned)face_blocks, (unsigned)n_views), dim3(kRasterThreads), 0, s, a);
  if (passes & NSLAM_RASTER_BIG) {
    const unsigned blocks = (unsigned)(a.cap < (unsigned long long)kBigBlocks ? a.cap : kBigBlocks);
    hipLaunchKernelGGL(k_raster_big<false>, dim3(blocks), dim3(kRasterThreads), 0, s, a);
  }
  if (passes & NSLAM_RASTER_RESOLVE)
    hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)pix_blocks), dim3(kRasterThreads), 0, s, a.depth, n_pix);
  return hip_status();
}

extern "C" size_t nslam_scene_workspace_size(int64_t capacity, int32_t n_views, int32_t H, int32_t W) {
  const int64_t n_pix = (n_views > 0 && H > 0 && W > 0) ? (int64_t)n_views * H * W : 0;
  return nslam_raster_workspace_size(capacity) + (size_t)n_pix * sizeof(unsigned long long);
}

extern "C" int nslam_scene_render(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                  const uint8_t* vert_colors, const void* normals, int32_t normals_f64,
                                  const uint8_t grey[3], const double* points, const uint8_t* point_colors,
                                  int64_t n_points, double point_size, const double* w2c, int32_t n_views, int32_t H,
                                  int32_t W, double fx, double fy, double cx, double cy, double z_near, double z_far,
                                  int32_t cull, const uint8_t background[3], double ambient,
                                  int64_t small_max_pixels, int32_t passes, uint8_t* color, float* depth, int32_t* ids,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_points < 0 || n_views < 0 || H <= 0 || W <= 0 || small_max_pixels < 0)
    return NSLAM_EINVAL;
  if (!(fx > 0.0) || !(fy > 0.0) || !finite_h(fx) || !finite_h(fy) || !finite_h(cx) || !finite_h(cy))
    return NSLAM_EINVAL;
  if (!(z_near >= 0.0) || !(z_near < z_far)) return NSLAM_EINVAL;  // NaN fails both
  if (passes < 0 || passes > NSLAM_SCENE_ALL) return NSLAM_EINVAL;
  if (cull != NSLAM_CULL_NONE && cull != NSLAM_CULL_BACK && cull != NSLAM_CULL_FRONT) return NSLAM_EINVAL;
  if (!(ambient >= 0.0) || !(ambient <= 1.0) || !(point_size > 0.0) || !background) return NSLAM_EINVAL;
  if (point_size > 64.0) return NSLAM_EUNSUPPORTED;
  if ((int64_t)H * W >= (int64_t(1) << 31) || n_verts >= (int64_t(1) << 31) || n_faces >= (int64_t(1) << 31) ||
      n_points >= (int64_t(1) << 31))
    return NSLAM_EINVAL;
  if (n_views == 0) return NSLAM_OK;  // no image: no launch
  if (!w2c || !color || !ws) return NSLAM_EINVAL;
  if (n_faces > 0 && (!verts || !faces || !normals || n_verts == 0 || (!vert_colors && !grey))) return NSLAM_EINVAL;
  if (n_points > 0 && (!points || !point_colors)) return NSLAM_EINVAL;
  if (ws_bytes < nslam_scene_workspace_size(1, n_views, H, W)) return NSLAM_EINVAL;
  if (n_views > 65535) return NSLAM_EUNSUPPORTED;  // one grid row per view
  const int64_t n_pix = (int64_t)n_views * H * W;
  const int64_t pix_blocks = (n_pix + kRasterThreads - 1) / kRasterThreads;
  const int64_t face_blocks = (n_faces + kRasterThreads - 1) / kRasterThreads;
  const int64_t point_blocks = (n_points + kRasterThreads - 1) / kRasterThreads;
  if (pix_blocks >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
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
  a.cull = cull;
  // the workspace: the list's head, one key per pixel, the list's items
  char* w = reinterpret_cast<char*>(ws);
  const size_t key_bytes = (size_t)n_pix * sizeof(unsigned long long);
  a.head = reinterpret_cast<RasterHead*>(w);
  a.keys = reinterpret_cast<unsigned long long*>(w + sizeof(RasterHead));
  a.items = reinterpret_cast<RasterItem*>(w + sizeof(RasterHead) + key_bytes);
  a.cap = (ws_bytes - sizeof(RasterHead) - key_bytes) / sizeof(RasterItem);
  SceneArgs sc{};
  sc.vcol = vert_colors;
  sc.vnrm = normals;
  sc.nrm_f64 = normals_f64;
  sc.pts = points;
  sc.pcol = point_colors;
  sc.np = n_points;
  sc.half = point_size * 0.5;
  sc.ambient = ambient;
  for (int d = 0; d < 3; ++d) {
    sc.grey[d] = grey ? grey[d] : (uint8_t)0;
    sc.bg[d] = background[d];
  }
  sc.color = color;
  sc.depth = depth;
  sc.ids = ids;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (passes & NSLAM_RASTER_CLEAR)
    hipLaunchKernelGGL(k_scene_clear, dim3((unsigned)pix_blocks), dim3(kRasterThreads), 0, s, a.keys, n_pix, a.head);
  if ((passes & NSLAM_RASTER_SMALL) && n_faces > 0)
    hipLaunchKernelGGL(k_raster_small<true>, dim3((unsigned)face_blocks, (unsigned)n_views), dim3(kRasterThreads), 0, s,
                       a);
  if ((passes & NSLAM_RASTER_BIG) && n_faces > 0) {
    const unsigned blocks = (unsigned)(a.cap < (unsigned long long)kBigBlocks ? a.cap : kBigBlocks);
    hipLaunchKernelGGL(k_raster_big<true>, dim3(blocks), dim3(kRasterThreads), 0, s, a);
  }
  if ((passes & NSLAM_SCENE_POINTS) && n_points > 0)
    hipLaunchKernelGGL(k_scene_points, dim3((unsigned)point_blocks, (unsigned)n_views), dim3(kRasterThreads), 0, s, a,
                       sc);
  if (passes & NSLAM_RASTER_RESOLVE)
    hipLaunchKernelGGL(k_scene_resolve, dim3((unsigned)pix_blocks), dim3(kRasterThreads), 0, s, a, sc, n_pix);
  return hip_status();
}
