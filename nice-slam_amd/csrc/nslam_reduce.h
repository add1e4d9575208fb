// nslam_reduce.h — the ordered float64 sums of the evaluation, metric and odometry units (nslam_eval.hip,
// nslam_metrics.hip, nslam_odometry.hip).  No atomics and no tickets: the order of the additions is fixed, so a
// sum has the same bits on every run.  The order, which tests/ordered_sum_ref.py restates:
//   1. a thread adds its own terms in ascending order (the caller's loop);
//   2. a wave's 64 values by the tree 32, 16, .. 1 (wave_sum: in lane 0 the additions of a __shfl_down tree);
//   3. the workgroup's waves in wave order, starting from wave 0's value (group_sum);
//   4. where several workgroups share a sum, a second launch adds their partials in index order, starting
//      from +0 (wave_ordered_sum).
#pragma once

#include "nslam_dev.h"

// Steps 2 and 3 for K values per thread of a workgroup of kThreads: thread j < K returns the workgroup's total
// of value j; what the other threads return is not a result (they read value 0's row, so that the only branch is
// the caller's `if (threadIdx.x < K)` around its store).  lds: one row of K per wave, the caller's.  There is one
// barrier inside, between the waves' writes and the reads: every thread of the workgroup has to call, and a
// kernel that uses lds again (a second group_sum included) needs a __syncthreads() of its own before it does.
template <int kThreads, int K>
__device__ __forceinline__ double group_sum(const double (&v)[K], double (*lds)[K]) {
  static_assert(kThreads % 64 == 0 && K <= kThreads, "whole waves, and a thread for every value");
  const int w = wave_id();
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {  // one guarded block of K stores, not K guarded stores
#pragma unroll
    for (int k = 0; k < K; ++k) lds[w][k] = s[k];
  }
  __syncthreads();
  const int j = threadIdx.x < K ? threadIdx.x : 0;
  double t = lds[0][j];
#pragma unroll
  for (int k = 1; k < kThreads / 64; ++k) t += lds[k][j];
  return t;
}

// lane i's value of v as a wave-uniform value (i: a constant once the caller's loop is unrolled): two v_readlane
__device__ __forceinline__ double lane_value(double v, int i) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, i);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), i);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Step 4: Σ_j p[j·stride], j ascending, by one wave: its lanes load 64 consecutive partials at once, then the 64
// values are added in lane order, so the additions are the serial ones while the loads take n / 64 rounds, not
// n.  Lanes past n hold +0, which leaves the sum's value as it is.  The values come through v_readlane, not a
// shuffle: the chain is 64 dependent v_add_f64, with no LDS round trip inside it (with __shfl the 798 partials
// of a 680 x 1200 SSIM level took 41 us, most of it that latency).  Every lane returns the sum.
__device__ __forceinline__ double wave_ordered_sum(gptr_t<double> p, int32_t n, int64_t stride) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int32_t base = 0; base < n; base += 64) {  // uniform
    const int32_t j = base + lane;
    const double v = j < n ? p[(int64_t)j * stride] : 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i) s += lane_value(v, i);
  }
  return s;
}
