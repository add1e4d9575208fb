// nslam_mesh.hip — the per-point, per-cell and per-face work of Mesher.get_mesh (src/utils/Mesher.py):
//   nslam_point_masks      seen / forecast / unseen masks of points against K keyframes (Mesher.py:53-212)
//   nslam_mc_count / emit  marching cubes of a float32 volume into an indexed mesh (replaces skimage, :437-467)
//   nslam_points_in_hull   points against the half-spaces of a convex hull (replaces trimesh contains, :469-485)
//   nslam_mesh_face_cull   faces whose three vertices are all masked (:484-496)
//   nslam_mesh_components  connected components and their areas (replaces trimesh split, :498-508)
//   nslam_mesh_select / nslam_mesh_remap  the component choice and the re-indexing of the kept faces
// All of it is HBM / latency-bound elementwise work: one thread per point, lattice point or face, neighbours
// read through the caches, wave reductions in front of every atomic.  The build has -ffp-contract=off and the
// projection below is written without FMAs, so it rounds where the reference's float32 torch ops round.
#include <math.h>

#include "nslam_dev.h"
#include "nslam_mc_fan.h"

namespace {

constexpr int kMeshThreads = 256;

inline int64_t blocks_for(int64_t n) { return (n + kMeshThreads - 1) / kMeshThreads; }

// ------------------------------------------------------------------------------------------------
// point masks
// ------------------------------------------------------------------------------------------------
struct MaskArgs {
  const float* pts;    // [N][3]
  const float* w2c;    // [K][16] row-major
  const float* depth;  // [K][H][W] or NULL (use_all_frames)
  int64_t n, pbs, bpc;  // points, points per chunk, blocks per chunk
  int32_t K, H, W;
  float fx, fy, cx, cy;
  int32_t depth_test, use_all;
  uint32_t* dmax;  // depth_test: [chunks][K]; else [K] (float bits)
  uint8_t *seen, *forecast, *unseen;
};

struct Proj {
  float u, v, z, pd;  // pixel, z = uv_z + 1e-8, pd = -cam_z
};

// cam = w2c . [p, 1] (four float32 products summed left to right), x flipped, uv = K . cam, z = uv_z + 1e-8
__device__ __forceinline__ Proj project(const MaskArgs& a, const float* __restrict__ m, float x, float y, float z) {
  const float cx_ = -(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
  const float cy_ = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  const float cz_ = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
  const float ux = a.fx * cx_ + a.cx * cz_;
  const float uy = a.fy * cy_ + a.cy * cz_;
  Proj p;
  p.z = cz_ + 1e-8f;
  p.u = ux / p.z;
  p.v = uy / p.z;
  p.pd = -cz_;
  return p;
}

__device__ __forceinline__ float tap(const float* __restrict__ img, int32_t H, int32_t W, float xf, float yf) {
  // bounds are tested in float: the coordinates of points behind the camera do not fit an int
  if (!(xf >= 0.f && xf <= (float)(W - 1) && yf >= 0.f && yf <= (float)(H - 1))) return 0.f;
  return img[(int64_t)yf * W + (int64_t)xf];
}

// F.grid_sample(depth, uv normalised, bilinear, padding 'zeros', align_corners=True) through the
// reference's own normalisation (Mesher.py:161-162) and grid_sample's un-normalisation
__device__ __forceinline__ float sample_depth(const float* __restrict__ img, int32_t H, int32_t W, float u, float v) {
  const float xn = u / (float)(W - 1) * 2.0f - 1.0f, yn = v / (float)(H - 1) * 2.0f - 1.0f;
  const float ix = ((xn + 1.f) / 2.f) * (float)(W - 1), iy = ((yn + 1.f) / 2.f) * (float)(H - 1);
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
  const float nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy);
  const float sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0);
  float out = 0.f;
  const float t00 = tap(img, H, W, x0, y0), t01 = tap(img, H, W, x1, y0);
  const float t10 = tap(img, H, W, x0, y1), t11 = tap(img, H, W, x1, y1);
  // a tap outside the image adds nothing (its weight may be inf or NaN far outside)
  if (t00 != 0.f) out += t00 * nw;
  if (t01 != 0.f) out += t01 * ne;
  if (t10 != 0.f) out += t10 * sw;
  if (t11 != 0.f) out += t11 * se;
  return out;
}

__device__ __forceinline__ void wave_atomic_max(uint32_t* dst, float d) {
  // samples are >= 0: the bit pattern orders like the value
  const uint32_t m = wave_max_u32(__float_as_uint(fmaxf(d, 0.f)));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(dst, m);
}

// pass 1, depth_test: dmax[chunk][k] = max over the chunk's points of the sampled depth (Mesher.py:166),
// points behind the camera and outside the image included
__global__ __launch_bounds__(kMeshThreads) void k_mask_chunk_max(MaskArgs a) {
  const int64_t chunk = blockIdx.x / a.bpc;
  const int64_t local = (int64_t)(blockIdx.x % a.bpc) * kMeshThreads + threadIdx.x;
  const int64_t i = chunk * a.pbs + local;
  const bool live = local < a.pbs && i < a.n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    x = a.pts[3 * i];
    y = a.pts[3 * i + 1];
    z = a.pts[3 * i + 2];
  }
  for (int32_t k = 0; k < a.K; ++k) {
    float d = 0.f;
    if (live) {
      const Proj p = project(a, a.w2c + 16 * k, x, y, z);
      d = sample_depth(a.depth + (int64_t)k * a.H * a.W, a.H, a.W, p.u, p.v);
    }
    wave_atomic_max(a.dmax + chunk * a.K + k, d);
  }
}

// pass 1, no depth_test: dmax[k] = max(depth[k])
__global__ __launch_bounds__(kMeshThreads) void k_mask_image_max(const float* depth, int64_t hw, uint32_t* dmax) {
  const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  const int32_t k = blockIdx.y;
  wave_atomic_max(dmax + k, i < hw ? depth[(int64_t)k * hw + i] : 0.f);
}

__global__ __launch_bounds__(kMeshThreads) void k_mask_points(MaskArgs a) {
  const int64_t chunk = blockIdx.x / a.bpc;
  const int64_t local = (int64_t)(blockIdx.x % a.bpc) * kMeshThreads + threadIdx.x;
  const int64_t i = chunk * a.pbs + local;
  const bool live = local < a.pbs && i < a.n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    x = a.pts[3 * i];
    y = a.pts[3 * i + 1];
    z = a.pts[3 * i + 2];
  }
  bool seen = false, fore = false;
  const float Wf = (float)a.W, Hf = (float)a.H;
  for (int32_t k = 0; k < a.K; ++k) {
    // forecast &= ~seen at the end: a seen lane has nothing left to learn; leave once the whole wave is
    if (__ballot(live && !seen) == 0) break;
    if (!live || seen) continue;
    const Proj p = project(a, a.w2c + 16 * k, x, y, z);
    const bool front = p.z < 0.f;
    bool s = (p.u < Wf) & (p.u > 0.f) & (p.v < Hf) & (p.v > 0.f) & front;
    bool f = (p.u < Wf + 1000.f) & (p.u > -1000.f) & (p.v < Hf + 1000.f) & (p.v > -1000.f) & front;
    if (!a.use_all) {
      if (a.depth_test) {
        const float md = __uint_as_float(a.dmax[chunk * a.K + k]);
        f = f && p.pd < md;
        if (s) {
          const float ds = sample_depth(a.depth + (int64_t)k * a.H * a.W, a.H, a.W, p.u, p.v);
          s = (p.pd < ds + 2.4f) & (ds - 2.4f < p.pd);
        }
      } else {
        const float md = __uint_as_float(a.dmax[k]) * 1.1f;
        f = f && p.pd < md;
        s = s && p.pd < md;
      }
    }
    seen |= s;
    fore |= f;
  }
  if (live) {
    fore = fore && !seen;
    a.seen[i] = seen ? 1 : 0;
    a.forecast[i] = fore ? 1 : 0;
    a.unseen[i] = (seen || fore) ? 0 : 1;
  }
}

// ------------------------------------------------------------------------------------------------
// marching cubes
// ------------------------------------------------------------------------------------------------
struct McArgs {
  const float* vol;  // [nx][ny][nz]
  int32_t nx, ny, nz;
  float level;
  double origin[3], spacing[3];
  uint8_t* flags;           // [N][3]: the +x, +y, +z edge of a lattice point crosses
  uint8_t* ntri;            // [N]: triangles of the cell whose low corner the point is
  const int32_t* vert_off;  // [N][3] exclusive scan of flags
  const int32_t* face_off;  // [N] exclusive scan of ntri
  double* verts;            // [V][3]
  int32_t* faces;           // [F][3]
};

__device__ __forceinline__ bool below(float v, float level) { return v < level; }

__device__ __forceinline__ int cell_case(const McArgs& a, int64_t p, int64_t sx, int64_t sy) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t q = p + (k & 1) * sx + ((k >> 1) & 1) * sy + ((k >> 2) & 1);
    c |= below(a.vol[q], a.level) ? (1 << k) : 0;
  }
  return c;
}

__global__ __launch_bounds__(kMeshThreads) void k_mc_count(McArgs a) {
  const int64_t n = (int64_t)a.nx * a.ny * a.nz;
  const int64_t p = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (p >= n) return;
  const int64_t sy = a.nz, sx = (int64_t)a.ny * a.nz;
  const int32_t k = (int32_t)(p % a.nz), j = (int32_t)((p / a.nz) % a.ny), i = (int32_t)(p / sx);
  const bool b0 = below(a.vol[p], a.level);
  const bool hx = i + 1 < a.nx, hy = j + 1 < a.ny, hz = k + 1 < a.nz;
  a.flags[3 * p] = (hx && below(a.vol[p + sx], a.level) != b0) ? 1 : 0;
  a.flags[3 * p + 1] = (hy && below(a.vol[p + sy], a.level) != b0) ? 1 : 0;
  a.flags[3 * p + 2] = (hz && below(a.vol[p + 1], a.level) != b0) ? 1 : 0;
  a.ntri[p] = (hx && hy && hz) ? kMcNumTri[cell_case(a, p, sx, sy)] : 0;
}

__global__ __launch_bounds__(kMeshThreads) void k_mc_emit(McArgs a) {
  const int64_t n = (int64_t)a.nx * a.ny * a.nz;
  const int64_t p = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (p >= n) return;
  const int64_t sy = a.nz, sx = (int64_t)a.ny * a.nz;
  const int32_t idx[3] = {(int32_t)(p / sx), (int32_t)((p / a.nz) % a.ny), (int32_t)(p % a.nz)};
  const int32_t dims[3] = {a.nx, a.ny, a.nz};
  const int64_t step[3] = {sx, sy, 1};
  const float v0 = a.vol[p];
  const bool b0 = below(v0, a.level);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    if (idx[ax] + 1 >= dims[ax]) continue;
    const float v1 = a.vol[p + step[ax]];
    if (below(v1, a.level) == b0) continue;
    const float t = (a.level - v0) / (v1 - v0);
    double* o = a.verts + 3 * (int64_t)a.vert_off[3 * p + ax];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o[c] = a.origin[c] + ((double)idx[c] + (c == ax ? (double)t : 0.0)) * a.spacing[c];
  }
  if (idx[0] + 1 >= a.nx || idx[1] + 1 >= a.ny || idx[2] + 1 >= a.nz) return;
  const int cs = cell_case(a, p, sx, sy);
  const int nt = kMcNumTri[cs];
  if (nt == 0) return;
  int32_t* f = a.faces + 3 * (int64_t)a.face_off[p];
  const McRow row = row_pack(cs);
  // every loop of the row fanned from its apex (nslam_mc_fan.h), in the table's winding
  int tr = 0;
  while (tr < nt) {
    uint32_t loop;
    int n;
    const int next = row_loop(row, nt, tr, loop, n);
    const int apex = loop_apex(loop, n);
    for (int i = 1; i < n - 1; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int e = fan_edge(loop, n, apex, i, k);
        const int c = edge_owner(e);  // the lattice point that owns edge e, as a corner of this cell
        const int64_t q = p + (c & 1) * sx + ((c >> 1) & 1) * sy + ((c >> 2) & 1);
        f[3 * (tr + i - 1) + k] = a.vert_off[3 * q + (e >> 2)];
      }
    }
    tr = next;
  }
}

// ------------------------------------------------------------------------------------------------
// hull, cull, components
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kMeshThreads) void k_in_hull(const T* pts, int64_t n, const double* planes, int32_t m,
                                                          uint8_t* inside) {
  const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (i >= n) return;
  const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
  bool in = true;
  for (int32_t k = 0; k < m && in; ++k) {  // planes are wave-uniform: scalar loads
    const double* pl = planes + 4 * k;
    in = ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3] <= 0.0;
  }
  inside[i] = in ? 1 : 0;
}

__global__ __launch_bounds__(kMeshThreads) void k_face_cull(const int32_t* faces, int64_t nf, const uint8_t* vmask,
                                                            uint8_t* keep) {
  const int64_t f = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (f >= nf) return;
  const int32_t* t = faces + 3 * f;
  keep[f] = (vmask[t[0]] && vmask[t[1]] && vmask[t[2]]) ? 0 : 1;
}

__global__ __launch_bounds__(kMeshThreads) void k_label_init(int32_t* label, int64_t nv, double* area) {
  const int64_t v = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (v >= nv) return;
  label[v] = (int32_t)v;
  area[v] = 0.0;
}

// hook: every face pulls the roots of its three labels, and the labels themselves, down to their minimum
__global__ __launch_bounds__(kMeshThreads) void k_label_hook(const int32_t* faces, int64_t nf, int32_t* label,
                                                             int32_t* changed) {
  const int64_t f = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  bool ch = false;
  if (f < nf) {
    const int32_t* t = faces + 3 * f;
    const int32_t l0 = label[t[0]], l1 = label[t[1]], l2 = label[t[2]];
    const int32_t m = min(l0, min(l1, l2));
    if (l0 != m || l1 != m || l2 != m) {
      ch = true;
      if (l0 != m) atomicMin(label + l0, m), atomicMin(label + t[0], m);
      if (l1 != m) atomicMin(label + l1, m), atomicMin(label + t[1], m);
      if (l2 != m) atomicMin(label + l2, m), atomicMin(label + t[2], m);
    }
  }
  if (__ballot(ch) != 0 && (threadIdx.x & 63) == 0) *changed = 1;
}

// compress: pointer jumping to the root (labels only ever decrease, label[v] <= v: the walk ends)
__global__ __launch_bounds__(kMeshThreads) void k_label_jump(int32_t* label, int64_t nv) {
  const int64_t v = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (v >= nv) return;
  int32_t l = label[v];
  for (;;) {
    const int32_t up = label[l];
    if (up == l) break;
    l = up;
  }
  label[v] = l;
}

__global__ __launch_bounds__(kMeshThreads) void k_face_area(const double* verts, const int32_t* faces, int64_t nf,
                                                            const int32_t* label, double* area) {
  const int64_t f = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  double ar = 0.0;
  int32_t l = -1;
  if (f < nf) {
    const int32_t* t = faces + 3 * f;
    const double *p = verts + 3 * (int64_t)t[0], *q = verts + 3 * (int64_t)t[1], *r = verts + 3 * (int64_t)t[2];
    const double ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
    const double vx = r[0] - p[0], vy = r[1] - p[1], vz = r[2] - p[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    ar = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
    l = label[t[0]];
  }
  // faces in cell order mostly share their wave's component: one atomic per wave then, else one per face
  const int32_t l0 = __shfl(l, 0, 64);
  if (__ballot(l != l0 && l >= 0) == 0 && l0 >= 0) {
    ar = wave_sum(ar);
    if ((threadIdx.x & 63) == 0) atomicAdd(area + l0, ar);
  } else if (l >= 0) {
    atomicAdd(area + l, ar);
  }
}

// keep[f] = the face's component is the chosen one (largest >= 0) or its area passes the threshold;
// used[v] = 1 for the vertices of kept faces (all writers store the same byte)
__global__ __launch_bounds__(kMeshThreads) void k_face_select(const int32_t* faces, int64_t nf, const int32_t* label,
                                                              const double* area, const int64_t* largest,
                                                              double threshold, uint8_t* keep, uint8_t* used) {
  const int64_t f = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (f >= nf) return;
  const int32_t* t = faces + 3 * f;
  const int32_t l = label[t[0]];
  const bool k = largest ? (int64_t)l == *largest : area[l] > threshold;
  keep[f] = k ? 1 : 0;
  if (k) used[t[0]] = 1, used[t[1]] = 1, used[t[2]] = 1;
}

__global__ __launch_bounds__(kMeshThreads) void k_face_remap(const int32_t* faces, int64_t n3, const int32_t* new_id,
                                                             int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (i < n3) out[i] = new_id[faces[i]];
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C entry points (include/nslam.h)
// ------------------------------------------------------------------------------------------------
extern "C" size_t nslam_point_masks_workspace_size(int64_t n, int32_t n_frames, int64_t points_batch_size) {
  if (n <= 0 || n_frames <= 0 || points_batch_size <= 0) return 0;
  const int64_t chunks = (n + points_batch_size - 1) / points_batch_size;
  return align256((size_t)chunks * n_frames * 4);
}

extern "C" int nslam_point_masks(const float* pts, int64_t n, const float* w2c, int32_t n_frames, const float* depth,
                                 int32_t H, int32_t W, float fx, float fy, float cx, float cy, int32_t depth_test,
                                 int32_t use_all_frames, int64_t points_batch_size, uint8_t* seen, uint8_t* forecast,
                                 uint8_t* unseen, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || n_frames < 0 || H <= 1 || W <= 1 || points_batch_size <= 0) return NSLAM_EINVAL;
  if (n == 0) return NSLAM_OK;
  if (!pts || !seen || !forecast || !unseen || (n_frames > 0 && !w2c)) return NSLAM_EINVAL;
  if (!use_all_frames && n_frames > 0 && !depth) return NSLAM_EINVAL;
  if ((int64_t)H * W >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  const int64_t pbs = points_batch_size < n ? points_batch_size : n;
  const int64_t chunks = (n + pbs - 1) / pbs, bpc = blocks_for(pbs);
  if (chunks * bpc >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  const bool need_max = !use_all_frames && n_frames > 0;
  if (need_max && (!ws || ws_bytes < nslam_point_masks_workspace_size(n, n_frames, pbs))) return NSLAM_EWORKSPACE;
  MaskArgs a{};
  a.pts = pts;
  a.w2c = w2c;
  a.depth = depth;
  a.n = n;
  a.pbs = pbs;
  a.bpc = bpc;
  a.K = n_frames;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.depth_test = depth_test ? 1 : 0;
  a.use_all = use_all_frames ? 1 : 0;
  a.dmax = static_cast<uint32_t*>(ws);
  a.seen = seen;
  a.forecast = forecast;
  a.unseen = unseen;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 g((unsigned)(chunks * bpc)), b(kMeshThreads);
  if (need_max) {
    const size_t words = a.depth_test ? (size_t)chunks * n_frames : (size_t)n_frames;
    if (hipMemsetAsync(a.dmax, 0, words * 4, s) != hipSuccess) return NSLAM_EHIP - (int)hipGetLastError();
    if (a.depth_test) {
      hipLaunchKernelGGL(k_mask_chunk_max, g, b, 0, s, a);
    } else {
      const int64_t hw = (int64_t)H * W;
      hipLaunchKernelGGL(k_mask_image_max, dim3((unsigned)blocks_for(hw), (unsigned)n_frames), b, 0, s, depth, hw,
                         a.dmax);
    }
  }
  hipLaunchKernelGGL(k_mask_points, g, b, 0, s, a);
  return hip_status();
}

extern "C" size_t nslam_mc_workspace_size(int32_t nx, int32_t ny, int32_t nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  return (size_t)nx * ny * nz * 4;  // flags [N][3] then ntri [N]
}

static int mc_args(McArgs& a, const float* vol, int32_t nx, int32_t ny, int32_t nz, float level) {
  if (!vol || nx <= 0 || ny <= 0 || nz <= 0) return NSLAM_EINVAL;
  if ((int64_t)nx * ny * nz * 3 >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;  // int32 vertex ids
  a.vol = vol;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.level = level;
  return NSLAM_OK;
}

extern "C" int nslam_mc_count(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, void* ws,
                              size_t ws_bytes, void* stream) {
  McArgs a{};
  const int rc = mc_args(a, vol, nx, ny, nz, level);
  if (rc != NSLAM_OK) return rc;
  if (!ws || ws_bytes < nslam_mc_workspace_size(nx, ny, nz)) return NSLAM_EWORKSPACE;
  const int64_t n = (int64_t)nx * ny * nz;
  a.flags = static_cast<uint8_t*>(ws);
  a.ntri = a.flags + 3 * n;
  if (nx < 2 || ny < 2 || nz < 2) {  // no cell: no face could use a vertex, so none is flagged
    if (hipMemsetAsync(ws, 0, 4 * (size_t)n, reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
      return NSLAM_EHIP - (int)hipGetLastError();
    return NSLAM_OK;
  }
  hipLaunchKernelGGL(k_mc_count, dim3((unsigned)blocks_for(n)), dim3(kMeshThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_mc_emit(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, const double* origin,
                             const double* spacing, const int32_t* vert_off, const int32_t* face_off, int64_t n_verts,
                             int64_t n_faces, double* verts, int32_t* faces, void* stream) {
  McArgs a{};
  const int rc = mc_args(a, vol, nx, ny, nz, level);
  if (rc != NSLAM_OK) return rc;
  if (!origin || !spacing || !vert_off || !face_off || n_verts < 0 || n_faces < 0) return NSLAM_EINVAL;
  if (n_verts == 0 && n_faces == 0) return NSLAM_OK;
  if (!verts || !faces || nx < 2 || ny < 2 || nz < 2) return NSLAM_EINVAL;  // a volume without a cell has no mesh
  for (int c = 0; c < 3; ++c) {
    a.origin[c] = origin[c];
    a.spacing[c] = spacing[c];
  }
  a.vert_off = vert_off;
  a.face_off = face_off;
  a.verts = verts;
  a.faces = faces;
  const int64_t n = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(k_mc_emit, dim3((unsigned)blocks_for(n)), dim3(kMeshThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}

extern "C" int nslam_points_in_hull(const void* pts, int32_t is_double, int64_t n, const double* planes, int32_t m,
                                    uint8_t* inside, void* stream) {
  if (n < 0 || m < 0) return NSLAM_EINVAL;
  if (n == 0) return NSLAM_OK;
  if (!pts || !inside || (m > 0 && !planes)) return NSLAM_EINVAL;
  if (blocks_for(n) >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 g((unsigned)blocks_for(n)), b(kMeshThreads);
  if (is_double)
    hipLaunchKernelGGL(k_in_hull<double>, g, b, 0, s, static_cast<const double*>(pts), n, planes, m, inside);
  else
    hipLaunchKernelGGL(k_in_hull<float>, g, b, 0, s, static_cast<const float*>(pts), n, planes, m, inside);
  return hip_status();
}

extern "C" int nslam_mesh_face_cull(const int32_t* faces, int64_t n_faces, const uint8_t* vmask, int64_t n_verts,
                                    uint8_t* keep, void* stream) {
  if (n_faces < 0 || n_verts < 0 || n_verts >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  if (n_faces == 0) return NSLAM_OK;
  if (!faces || !vmask || !keep || n_verts == 0) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_face_cull, dim3((unsigned)blocks_for(n_faces)), dim3(kMeshThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), faces, n_faces, vmask, keep);
  return hip_status();
}

extern "C" int nslam_mesh_components(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                     int32_t* label, double* area, int32_t* flag, void* stream) {
  if (n_faces < 0 || n_verts < 0 || n_verts >= (int64_t(1) << 31)) return NSLAM_EINVAL;
  if (n_verts == 0) return NSLAM_OK;
  if (!verts || !label || !area || !flag || (n_faces > 0 && !faces)) return NSLAM_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 gv((unsigned)blocks_for(n_verts)), gf((unsigned)blocks_for(n_faces)), b(kMeshThreads);
  hipLaunchKernelGGL(k_label_init, gv, b, 0, s, label, n_verts, area);
  if (n_faces == 0) return hip_status();
  for (int64_t it = 0; it <= n_verts; ++it) {  // every round that changes something lowers a label
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) return NSLAM_EHIP - (int)hipGetLastError();
    hipLaunchKernelGGL(k_label_hook, gf, b, 0, s, faces, n_faces, label, flag);
    hipLaunchKernelGGL(k_label_jump, gv, b, 0, s, label, n_verts);
    int32_t h = 0;
    if (hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return NSLAM_EHIP - (int)hipGetLastError();
    if (!h) break;
  }
  hipLaunchKernelGGL(k_face_area, gf, b, 0, s, verts, faces, n_faces, label, area);
  return hip_status();
}

extern "C" int nslam_mesh_select(const int32_t* faces, int64_t n_faces, const int32_t* label, const double* area,
                                 const int64_t* largest, double threshold, uint8_t* keep, uint8_t* used,
                                 void* stream) {
  if (n_faces < 0) return NSLAM_EINVAL;
  if (n_faces == 0) return NSLAM_OK;
  if (!faces || !label || !area || !keep || !used) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_face_select, dim3((unsigned)blocks_for(n_faces)), dim3(kMeshThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), faces, n_faces, label, area, largest, threshold, keep,
                     used);
  return hip_status();
}

extern "C" int nslam_mesh_remap(const int32_t* faces, int64_t n_faces, const int32_t* new_id, int32_t* out,
                                void* stream) {
  if (n_faces < 0) return NSLAM_EINVAL;
  if (n_faces == 0) return NSLAM_OK;
  if (!faces || !new_id || !out) return NSLAM_EINVAL;
  hipLaunchKernelGGL(k_face_remap, dim3((unsigned)blocks_for(3 * n_faces)), dim3(kMeshThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), faces, 3 * n_faces, new_id, out);
  return hip_status();
}
