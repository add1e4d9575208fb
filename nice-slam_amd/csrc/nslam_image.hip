// nslam_image.hip — image preparation of the frame sources (datasets.py) on gfx950:
//   k_undistort_u8 : cv2.undistort(src, K, dist) with its defaults (new camera matrix K, bilinear, constant
//                    zero border) on an interleaved uint8 image, the colour frame of a TUM-RGBD sequence
//                    (src/utils/datasets.py:85-88).
// The contract (include/nslam.h nslam_undistort_u8) is exact integer arithmetic after one rounding step: the
// source position of a destination pixel is formed in float64 without FMA contraction, rounded to 1/32 pixel
// (the convention nslam_frustum_rows uses for cv2.remap), and the four taps are mixed with 10-bit integer
// weights.  One thread per destination pixel over all its channels; launch-bound at 480×640, so no tiling.
#include <math.h>

#include "nslam_dev.h"

namespace {

struct UndistortArgs {
  const uint8_t* src;
  uint8_t* dst;
  int32_t H, W, C;
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
};

// a 1/32-pixel position as an integer: round half to even; a position beyond ±2^30 (or NaN) is far outside any
// image either way, so it is clamped there before the conversion (and its taps read the zero border)
__device__ __forceinline__ int32_t fixed5(double v) {
  const double lim = 1073741824.0;
  if (!(v >= -lim)) return -(int32_t)1073741824;  // (NaN too)
  if (v > lim) return (int32_t)1073741824;
  return (int32_t)rint(v);
}

__global__ __launch_bounds__(256) void k_undistort_u8(UndistortArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.H * a.W) return;
  const int32_t v = (int32_t)(i / a.W), u = (int32_t)(i - (int64_t)v * a.W);
  const double x = ((double)u - a.cx) / a.fx, y = ((double)v - a.cy) / a.fy;
  const double r2 = x * x + y * y;
  const double rad = 1.0 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2;
  const double xd = x * rad + 2.0 * a.p1 * x * y + a.p2 * (r2 + 2.0 * x * x);
  const double yd = y * rad + a.p1 * (r2 + 2.0 * y * y) + 2.0 * a.p2 * x * y;
  const int32_t X = fixed5((xd * a.fx + a.cx) * 32.0), Y = fixed5((yd * a.fy + a.cy) * 32.0);
  const int32_t x0 = X >> 5, y0 = Y >> 5, ax = X & 31, ay = Y & 31;  // (arithmetic shift: floor)
  const int32_t w00 = (32 - ax) * (32 - ay), w10 = ax * (32 - ay), w01 = (32 - ax) * ay, w11 = ax * ay;
  const bool xin0 = x0 >= 0 && x0 < a.W, xin1 = x0 + 1 >= 0 && x0 + 1 < a.W;
  const bool yin0 = y0 >= 0 && y0 < a.H, yin1 = y0 + 1 >= 0 && y0 + 1 < a.H;
  // taps outside the image are never dereferenced: their offsets stay those of a pixel inside
  const int64_t r0 = (int64_t)(yin0 ? y0 : 0) * a.W, r1 = (int64_t)(yin1 ? y0 + 1 : 0) * a.W;
  const int64_t c0 = xin0 ? x0 : 0, c1 = xin1 ? x0 + 1 : 0;
  const uint8_t* s00 = a.src + (r0 + c0) * a.C;
  const uint8_t* s10 = a.src + (r0 + c1) * a.C;
  const uint8_t* s01 = a.src + (r1 + c0) * a.C;
  const uint8_t* s11 = a.src + (r1 + c1) * a.C;
  uint8_t* d = a.dst + i * a.C;
  for (int c = 0; c < a.C; ++c) {
    const int32_t t00 = xin0 && yin0 ? s00[c] : 0, t10 = xin1 && yin0 ? s10[c] : 0;
    const int32_t t01 = xin0 && yin1 ? s01[c] : 0, t11 = xin1 && yin1 ? s11[c] : 0;
    d[c] = (uint8_t)((w00 * t00 + w10 * t10 + w01 * t01 + w11 * t11 + 512) >> 10);
  }
}

}  // namespace

extern "C" int nslam_undistort_u8(const uint8_t* src, int32_t H, int32_t W, int32_t C, double fx, double fy, double cx,
                                  double cy, const double* dist, uint8_t* dst, void* stream) {
  if (!src || !dst || !dist || src == dst || H < 0 || W < 0 || C < 1 || C > 4) return NSLAM_EINVAL;
  if (!(fabs(fx) > 0.0) || !(fabs(fy) > 0.0)) return NSLAM_EINVAL;  // (zero, or NaN: no comparison holds)
  const int64_t n = (int64_t)H * W;
  if (n == 0) return NSLAM_OK;  // an empty image: no launch
  if (n >= (int64_t(1) << 31)) return NSLAM_EUNSUPPORTED;
  UndistortArgs a{src, dst, H, W, C, fx, fy, cx, cy, dist[0], dist[1], dist[2], dist[3], dist[4]};
  hipLaunchKernelGGL(k_undistort_u8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return hip_status();
}
