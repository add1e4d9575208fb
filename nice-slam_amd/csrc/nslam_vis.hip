// nslam_vis.hip — the visualiser's image mosaic (src/utils/Visualizer.py:57-100) on gfx950:
//   k_vis_panels : the six panels of one visualisation as ONE uint8 image [2H][3W][3],
//                  row 0 = input depth | generated depth | depth residual  (plasma, vmin 0, vmax = max gt depth)
//                  row 1 = input RGB   | generated RGB   | RGB residual
// The contract is in include/nslam.h (nslam_vis_panels); visualizer.vis_panels_np is its numpy twin, bit for bit.
// Elementwise and bandwidth-bound: one thread per output pixel, three byte stores each, so a wave writes 192
// consecutive bytes of the output; the 768-byte colour table is a device constant (nslam_plasma_lut.h, generated).
// No tuning.
#include <math.h>

#include "nslam_dev.h"
#include "nslam_plasma_lut.h"

namespace {

struct VisArgs {
  const float* gt_depth;   // [H][W]
  const float* gt_color;   // [H][W][3]
  const double* depth;     // [H][W]
  const float* color;      // [H][W][3]
  const float* vmax;       // device scalar
  uint8_t* out;            // [2H][3W][3]
  int32_t H, W;
};

// matplotlib's Normalize(0, vmax) then Colormap.__call__: the table row of a depth value, or -1 for "bad" (NaN)
__device__ __forceinline__ int plasma_row(double x, double vmax) {
  double t = vmax == 0.0 ? 0.0 : x / vmax;  // (vmin == vmax: Normalize fills zeros, NaN included)
  t = t * 256.0;
  if (t != t) return -1;
  if (t < 0.0) return 0;            // under: the map's first colour
  if (t >= 256.0) return 255;       // 1.0 itself, and over: the map's last colour
  return (int)t;                    // truncation, as astype(int)
}

// our own rule for the RGB panels: floor(255 * clip(x, 0, 1) + 0.5) in float32, NaN as 0
__device__ __forceinline__ uint8_t rgb_byte(float x) {
  const float c = x > 0.0f ? fminf(x, 1.0f) : 0.0f;
  return (uint8_t)floorf(255.0f * c + 0.5f);
}

__global__ __launch_bounds__(256) void k_vis_panels(VisArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row_px = 3 * (int64_t)a.W;
  if (p >= 2 * (int64_t)a.H * row_px) return;
  const int32_t r = (int32_t)(p / row_px), cc = (int32_t)(p - (int64_t)r * row_px);
  const int32_t panel = cc / a.W, x = cc - panel * a.W;
  const int32_t y = r < a.H ? r : r - a.H;
  const int64_t s = (int64_t)y * a.W + x;  // < H*W
  const float gd = a.gt_depth[s];
  uint8_t* o = a.out + p * 3;
  if (r < a.H) {
    const double vmax = (double)a.vmax[0];
    double v;
    if (panel == 0) {
      v = (double)gd;
    } else if (panel == 1) {
      v = a.depth[s];
    } else {
      v = gd == 0.0f ? 0.0 : fabs((double)gd - a.depth[s]);
    }
    const int k = plasma_row(v, vmax);
    o[0] = k < 0 ? (uint8_t)0 : kPlasma[k][0];
    o[1] = k < 0 ? (uint8_t)0 : kPlasma[k][1];
    o[2] = k < 0 ? (uint8_t)0 : kPlasma[k][2];
  } else {
    for (int c = 0; c < 3; ++c) {
      const float g = a.gt_color[s * 3 + c];
      float v;
      if (panel == 0) {
        v = g;
      } else if (panel == 1) {
        v = a.color[s * 3 + c];
      } else {
        v = gd == 0.0f ? 0.0f : fabsf(g - a.color[s * 3 + c]);
      }
      o[c] = rgb_byte(v);
    }
  }
}

}  // namespace

extern "C" int nslam_vis_panels(const float* gt_depth, const float* gt_color, const double* depth, const float* color,
                                int32_t H, int32_t W, const float* vmax, uint8_t* out, void* stream) {
  if (!gt_depth || !gt_color || !depth || !color || !vmax || !out || H < 0 || W < 0) return NSLAM_EINVAL;
  const int64_t n = 6 * (int64_t)H * W;  // output pixels
  if (n == 0) return NSLAM_OK;           // an empty image: no launch
  if (n >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  VisArgs a{gt_depth, gt_color, depth, color, vmax, out, H, W};
  hipLaunchKernelGGL(k_vis_panels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}
