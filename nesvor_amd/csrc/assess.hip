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
// Arithmetic: the products are fp32 (the build has -ffp-contract=off) and the six sums are added in the reproducible order of
// slice_sums.h: bit-identical from run to run, the count exact.  Every operation is symmetric in (a, b), so the pair (b, a)
// yields the bits of (a, b) with columns 1 <-> 2 and 3 <-> 4 swapped; self-pairs and repeated pairs are legal.
//
// The pair indices are NOT checked on the device: range-checking them (0 <= index < n) is the caller's job, on the host copy
// before the upload (nesvor_amd/assess.py::pair_moments does).
#include <hip/hip_runtime.h>
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kMoments = 6;

// grid: P * wgs workgroups of 256 pixels, wgs = ceil(hw / 256) per pair.  partial: (P, wgs, 6) doubles.
__global__ __launch_bounds__(256) void pair_moments_kernel(const float* __restrict__ slices, const uint8_t* __restrict__ mask,
                                                           const int32_t* __restrict__ pairs, int hw, int wgs,
                                                           double* __restrict__ partial) {
  const int ip = blockIdx.x / wgs, wg = blockIdx.x - ip * wgs;
  const int pix = wg * 256 + (int)threadIdx.x;  // the host checked hw <= INT_MAX - 256
  const int ia = pairs[2 * ip], ib = pairs[2 * ip + 1];  // workgroup-uniform: the scalar path
  const bool inside = pix < hw;
  const size_t idx_a = (size_t)ia * hw + (inside ? pix : 0), idx_b = (size_t)ib * hw + (inside ? pix : 0);
  const bool on = inside && (mask == nullptr || (mask[idx_a] && mask[idx_b]));
  float a = 0.f, b = 0.f;
  if (on) {
    a = slices[idx_a];
    b = slices[idx_b];
  }
  const float sums[kMoments] = {wave_sum_dpp(on ? 1.f : 0.f), wave_sum_dpp(a),     wave_sum_dpp(b),
                                wave_sum_dpp(a * a),          wave_sum_dpp(b * b), wave_sum_dpp(a * b)};
  slice_sums::store_workgroup_sums(sums,partial + ((size_t)ip * wgs + wg) * kMoments);
}

}  // namespace

extern "C" int64_t nesvor_pair_moments_workspace_bytes(int P, int h, int w) {
  if (P < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kMoments>{P, slice_sums::pixel_workgroups(h, w)}.workspace_bytes();
}

extern "C" int nesvor_pair_moments(const float* slices, const uint8_t* mask, int n, int h, int w, const int32_t* pairs, int P,
                                   double* moments, void* workspace, size_t workspace_bytes, void* stream) {
  if (P == 0) return 0;
  if (P < 0 || n < 1 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (slices == nullptr || pairs == nullptr || moments == nullptr) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kMoments> plan{P, slice_sums::pixel_workgroups(h, w)};
  if (!plan.accepts(h, w, plan.wgs * P, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pair_moments_kernel, dim3((unsigned)(plan.wgs * P)), dim3(256), 0, st, slices, mask, pairs, h * w, (int)plan.wgs,
                     (double*)workspace);
  plan.reduce(workspace, moments, st);
  return (int)hipGetLastError();
}
