// Masked moments of slice pairs for the stack quality assessment (gfx950): six sums per pair in one pass.
//
// A per-stack motion score (nesvor_amd/assess.py) is a function of the moments of slice pairs: adjacent pairs for the NCC
// score, all pairs of a stack for the low-rank score (the Gram matrix of the stack's data matrix).  For pair p = (a, b) of
// the list and the pixels valid in BOTH slices (mask byte set in a and in b, or no mask)
//   moments[p] = { count, sum a, sum b, sum a^2, sum b^2, sum a b }.
// Composed from torch operators a pair list means P x h x w gathered temporaries (or a matmul, which cannot honour the
// pairwise mask intersection); here one workgroup per (pair, 256-pixel chunk) reads the two slices where they lie - the
// working set, some 60 slices of 128^2, lives in L2 - and a small second launch adds the partials.
//
// Arithmetic, as in robust.hip and svr.hip: the products are fp32 (the build has -ffp-contract=off); fp32 sums only inside one
// wave's DPP reduction (64 terms), then double; every workgroup stores its six partials to the workspace and a second small
// launch adds them in workgroup order.  No atomics, no memset: the results are bit-identical from run to run.  The count is
// exact (at most 64 ones per wave in fp32, integers in double from there).  Every operation is symmetric in (a, b), so the
// pair (b, a) yields the bits of (a, b) with columns 1 <-> 2 and 3 <-> 4 swapped; self-pairs and repeated pairs are legal.
//
// The pair indices are NOT checked on the device: range-checking them (0 <= index < n) is the caller's job, on the host copy
// before the upload (nesvor_amd/assess.py::pair_moments does).
#include <hip/hip_runtime.h>
#include <limits.h>
#include "common.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kMoments = 6;

// grid: P * wgs workgroups of 256 pixels, wgs = ceil(hw / 256) per pair.  partial: (P, wgs, 6) doubles.
__global__ __launch_bounds__(256) void pair_moments_kernel(const float* __restrict__ slices, const uint8_t* __restrict__ mask,
                                                           const int32_t* __restrict__ pairs, int hw, int wgs,
                                                           double* __restrict__ partial) {
  __shared__ float red[4][kMoments];
  const int ip = blockIdx.x / wgs, wg = blockIdx.x - ip * wgs;
  const int pix = wg * 256 + (int)threadIdx.x;  // the host checked hw <= INT_MAX - 256
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ia = pairs[2 * ip], ib = pairs[2 * ip + 1];  // workgroup-uniform: the scalar path
  const bool inside = pix < hw;
  const size_t idx_a = (size_t)ia * hw + (inside ? pix : 0), idx_b = (size_t)ib * hw + (inside ? pix : 0);
  const bool on = inside && (mask == nullptr || (mask[idx_a] && mask[idx_b]));
  float a = 0.f, b = 0.f;
  if (on) {
    a = slices[idx_a];
    b = slices[idx_b];
  }
  const float s0 = wave_sum_dpp(on ? 1.f : 0.f), s1 = wave_sum_dpp(a), s2 = wave_sum_dpp(b), s3 = wave_sum_dpp(a * a),
              s4 = wave_sum_dpp(b * b), s5 = wave_sum_dpp(a * b);
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; red[wave][4] = s4; red[wave][5] = s5;
  }
  __syncthreads();
  if (threadIdx.x < kMoments) {
    const int j = threadIdx.x;
    const double t = ((double)red[0][j] + (double)red[1][j]) + ((double)red[2][j] + (double)red[3][j]);
    partial[((size_t)ip * wgs + wg) * kMoments + j] = t;
  }
}

// moments[p][j] = the partials of pair p added in workgroup order
__global__ __launch_bounds__(256) void pair_moments_reduce_kernel(const double* __restrict__ partial, int64_t total, int wgs,
                                                                  double* __restrict__ moments) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t p = t / kMoments;
  const int j = (int)(t - p * kMoments);
  double s = 0.0;
  for (int g = 0; g < wgs; ++g) s += partial[((size_t)p * wgs + g) * kMoments + j];
  moments[t] = s;
}

}  // namespace

extern "C" int64_t nesvor_pair_moments_workspace_bytes(int P, int h, int w) {
  if (P < 1 || h < 1 || w < 1) return 0;
  const int64_t wgs = ((int64_t)h * w + 255) / 256;
  return (int64_t)sizeof(double) * kMoments * P * wgs;
}

extern "C" int nesvor_pair_moments(const float* slices, const uint8_t* mask, int n, int h, int w, const int32_t* pairs, int P,
                                   double* moments, void* workspace, size_t workspace_bytes, void* stream) {
  if (P == 0) return 0;
  if (P < 0 || n < 1 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (slices == nullptr || pairs == nullptr || moments == nullptr) return (int)hipErrorInvalidValue;
  // pixel indices inside a slice are ints; one workgroup per 256 pixels of a pair
  if ((int64_t)h * w > INT_MAX - 256) return (int)hipErrorInvalidValue;
  const int64_t wgs = ((int64_t)h * w + 255) / 256;
  if (wgs * P > INT_MAX) return (int)hipErrorInvalidValue;
  const int64_t need = nesvor_pair_moments_workspace_bytes(P, h, w);
  if (workspace == nullptr || (int64_t)workspace_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(pair_moments_kernel, dim3((unsigned)(wgs * P)), dim3(256), 0, st, slices, mask, pairs, h * w, (int)wgs, partial);
  const int64_t total = (int64_t)P * kMoments;
  hipLaunchKernelGGL(pair_moments_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)partial,
                     total, (int)wgs, moments);
  return (int)hipGetLastError();
}
