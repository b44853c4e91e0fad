// Reproducible per-entry sums for the slice-statistics kernels (svr.hip, robust.hip, assess.hip, structural.hip): N sums over the
// pixels of every entry (a slice, a slice pair, a (slice, pose)), bit-identical from run to run.
//
// The order, which tests/test_gpu_ordered_sums.py rebuilds on the host:
//   1. A workgroup is 256 threads, one pixel each; a thread off the mask or past the edge contributes 0.  A wave adds its 64
//      lanes with wave_sum_dpp (common.h): a balanced pairwise tree in fp32.
//   2. Lane 0 of each wave parks the N wave sums in LDS; after one barrier threads < N add the four waves as (0 + 1) + (2 + 3)
//      in double and store the result to the workgroup's row of the workspace, (entries, wgs, N) doubles.
//   3. A second small launch adds the wgs rows of an entry one after the other from 0 in double.
// Why fp32 inside a wave and double beyond.  Step 1 is where the adds are (63 per wave and sum, on the VALU next to the
// per-pixel arithmetic): in fp32 the tree is six adds deep, so a wave sum is within 6 * 2^-24 of the absolute sum of its 64
// terms, of the size of the roundings the fp32 terms carry already.  From step 2 on the number of addends grows with the
// slice, not with the wave, and there are only N adds per workgroup: in double they cost nothing and add nothing to the error.
// A kernel held to a tighter bound runs the same tree in double (wave_sum_f64: structural.hip says why).  Counts are exact: a
// wave adds at most 64 ones in fp32, and integers below 2^53 are exact in double.  No atomics, no memset: every row of the
// workspace is written by exactly one workgroup before the second launch reads it, so neither an order of arrival nor a
// stale value can enter a sum, and the workspace needs no initialisation.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "common.h"

// (unnamed: every translation unit gets kernels and host stubs of its own, as its other kernels are)
namespace {
namespace slice_sums {

// Step 2.  `s`: the wave-uniform sums of this thread's wave; `row`: the N doubles of this workgroup.  Every thread of the
// 256-thread workgroup must call (barrier).  (svr.hip and structural.hip write the step out and say why.)
template <typename T, int N>
__device__ __forceinline__ void store_workgroup_sums(const T (&s)[N], double* row) {
  __shared__ T red[4][N];
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) red[tid >> 6][j] = s[j];
  }
  __syncthreads();
  if (tid < N) row[tid] = ((double)red[0][tid] + (double)red[1][tid]) + ((double)red[2][tid] + (double)red[3][tid]);
}

// Step 3.  sums[e][j] = the partials of entry e added in workgroup order; total = entries * N.
template <int N>
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ partial, int64_t total, int wgs,
                                                     double* __restrict__ sums) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t e = t / N;
  const int j = (int)(t - e * N);
  double s = 0.0;
  for (int g = 0; g < wgs; ++g) s += partial[((size_t)e * wgs + g) * N + j];
  sums[t] = s;
}

inline int64_t pixel_workgroups(int h, int w) { return ((int64_t)h * w + 255) / 256; }  // one per 256 pixels of a slice
inline int64_t tile_workgroups(int h, int w) { return (((int64_t)h + 15) / 16) * (((int64_t)w + 15) / 16); }  // one per 16 x 16 tile

// The host side of one call: `entries` rows of N sums, each over `wgs` workgroups.
template <int N>
struct Plan {
  int64_t entries, wgs;
  int64_t workspace_bytes() const { return (int64_t)sizeof(double) * N * entries * wgs; }
  // The refusals the launchers share: pixel indices inside a slice are ints (a workgroup may index 255 past the last), the
  // first launch's `grid` fits an int, and the workspace is there and long enough.
  bool accepts(int h, int w, int64_t grid, const void* workspace, size_t bytes) const {
    if ((int64_t)h * w > INT_MAX - 256 || grid > INT_MAX) return false;
    return workspace != nullptr && (int64_t)bytes >= workspace_bytes();
  }
  void reduce(const void* workspace, double* sums, hipStream_t st) const {
    const int64_t total = entries * N;
    hipLaunchKernelGGL(reduce_kernel<N>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)workspace, total,
                       (int)wgs, sums);
  }
};

}  // namespace slice_sums
}  // namespace
