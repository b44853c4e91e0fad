// Joint histograms for the mutual-information similarity of the stack registration (gfx950): the sibling of vvr.hip whose statistic
// per pose is not five moment sums but a B x B histogram of (sampled source, target) intensities, and the samples themselves.
//
// The definition is nesvor_amd/nmi.py's, the one csrc/svr_nmi.hip implements for slices: every point of the target's list - ALL of
// them: a point that leaves the source samples I = 0 and counts, as it does in vvr.hip's sums - adds the four integer products of
// its I weights and its J weights (nmi_hist.h: axis_place, add_sample) to the cells (bI, bJ), 65536 units in all.  I is
// vvr_sample.h's sample_point in both kernels here - the operations of vvr_similarity_kernel, every one rounded on its own (the
// build does not contract) - so a (point, pose) has one value bit for bit; J is the target's value; both affine maps are the
// host's, one per call.
//
// Shape.  The point list is cut into segments (nmi_hist.h: segment_pixels, with the poses of the call as its entries); one workgroup
// serves one (pose, segment): it keeps the histogram in LDS (B B 32-bit cells, at most 16 KB), walks its points 256 at a time, adds
// with integer LDS atomics and stores the cells to its own rows of the workspace with plain stores; a second launch
// (joint_histogram_reduce_kernel) adds the segments of a pose in 64 bits and writes every cell of the result.  One pose per
// workgroup: several would reuse the three coordinate reads and the target read of a point - 16 of the 48 bytes a (point, pose)
// touches, and L2 hits after the first pose - at the price of one LDS histogram each, and 13 poses of 64 bins do not fit.  The 13
// poses of a gradient get long segments, the K = 1 accept test enough of them to fill the chip ("Mutual-information
// stack registration", has the measurements).  No float atomic, no global atomic, no memset; nothing depends on the order of the
// adds.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "nmi_hist.h"
#include "vvr_sample.h"
#include "../../include/nesvor_hip.h"

namespace {
using namespace nmi_hist;
using namespace vvr;

// grid: K S workgroups, S = ceil(M / seg) segments of `seg` points per pose; block k S + s serves segment s of pose k.
// partial: (K, S, B, B) 32-bit cells, row = I bin.
__global__ __launch_bounds__(256) void vvr_joint_histogram_kernel(const float* __restrict__ src, int D, int H, int W,
                                                                  const float* __restrict__ pts, const float* __restrict__ tgt,
                                                                  const float* __restrict__ mats, float ux, float uy, float uz, int M,
                                                                  int S, int seg, float i_lo, float i_scale, float j_lo, float j_scale,
                                                                  int B, uint32_t* __restrict__ partial) {
  __shared__ uint32_t hist[kMaxNmiBins * kMaxNmiBins];
  const int k = blockIdx.x / S, s = blockIdx.x - k * S;
  const int cells = B * B;
  for (int c = threadIdx.x; c < cells; c += 256) hist[c] = 0u;
  float m[12];  // wave-uniform: the scalar path
#pragma unroll
  for (int e = 0; e < 12; ++e) m[e] = mats[(size_t)k * 12 + e];
  __syncthreads();
  const float hx = 0.5f * (W - 1), hy = 0.5f * (H - 1), hz = 0.5f * (D - 1);
  const int64_t first = (int64_t)s * seg;  // (below M: S = ceil(M / seg))
  const int64_t last = min(first + seg, (int64_t)M);
  for (int64_t i = first + threadIdx.x; i < last; i += 256) {
    const float I = sample_point(src, D, H, W, m, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], ux, uy, uz, hx, hy, hz);
    add_sample(axis_place(I, i_lo, i_scale, B), axis_place(tgt[i], j_lo, j_scale, B), B,
               [&](int cell, uint32_t p) { atomicAdd(&hist[cell], p); });
  }
  __syncthreads();
  uint32_t* row = partial + (size_t)blockIdx.x * cells;
  for (int c = threadIdx.x; c < cells; c += 256) row[c] = hist[c];
}

// grid: K P workgroups, P = ceil(M / 256); block k P + p samples points 256 p .. of pose k.  out (K, M).
__global__ __launch_bounds__(256) void vvr_sample_kernel(const float* __restrict__ src, int D, int H, int W, const float* __restrict__ pts,
                                                         const float* __restrict__ mats, float ux, float uy, float uz, int64_t M, int P,
                                                         float* __restrict__ out) {
  const int k = blockIdx.x / P, p = blockIdx.x - k * P;
  float m[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) m[e] = mats[(size_t)k * 12 + e];
  const int64_t i = (int64_t)p * 256 + threadIdx.x;
  if (i >= M) return;
  const float hx = 0.5f * (W - 1), hy = 0.5f * (H - 1), hz = 0.5f * (D - 1);
  out[(size_t)k * M + i] = sample_point(src, D, H, W, m, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], ux, uy, uz, hx, hy, hz);
}

}  // namespace

extern "C" int64_t nesvor_vvr_joint_histogram_workspace_bytes(int64_t M, int K, int bins) {
  if (M < 1 || M > INT_MAX || K < 1 || bins < 2 || bins > kMaxNmiBins) return 0;
  return (int64_t)sizeof(uint32_t) * K * segments(K, M) * bins * bins;
}

extern "C" int nesvor_vvr_joint_histogram(const float* source, int D, int H, int W, const float* points, const float* target,
                                          const float* mats, const float* to_unit_xyz, int64_t M, int K, float i_lo, float i_scale,
                                          float j_lo, float j_scale, int bins, int64_t* hist, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (M <= 0 || K <= 0) return 0;
  if (D < 1 || H < 1 || W < 1 || bins < 2 || bins > kMaxNmiBins || M > INT_MAX) return (int)hipErrorInvalidValue;
  const int64_t S = segments(K, M), cells = (int64_t)bins * bins;
  if (K * S > INT_MAX || K * cells / 256 >= INT_MAX) return (int)hipErrorInvalidValue;  // both grids fit an int
  if (workspace == nullptr || (int64_t)workspace_bytes < (int64_t)sizeof(uint32_t) * K * S * cells) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* partial = (uint32_t*)workspace;
  hipLaunchKernelGGL(vvr_joint_histogram_kernel, dim3((unsigned)(K * S)), dim3(256), 0, st, source, D, H, W, points, target, mats,
                     to_unit_xyz[0], to_unit_xyz[1], to_unit_xyz[2], (int)M, (int)S, segment_pixels(K, M), i_lo, i_scale, j_lo, j_scale, bins,
                     partial);
  const int64_t total = K * cells;
  hipLaunchKernelGGL(joint_histogram_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)partial,
                     total, (int)cells, (int)S, hist);
  return (int)hipGetLastError();
}

extern "C" int nesvor_vvr_sample(const float* source, int D, int H, int W, const float* points, const float* mats,
                                 const float* to_unit_xyz, int64_t M, int K, float* out, void* stream) {
  if (M <= 0 || K <= 0) return 0;
  if (D < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const int64_t P = (M + 255) / 256;
  if (K * P > INT_MAX) return (int)hipErrorInvalidValue;  // the grid fits an int
  hipLaunchKernelGGL(vvr_sample_kernel, dim3((unsigned)(K * P)), dim3(256), 0, (hipStream_t)stream, source, D, H, W, points, mats,
                     to_unit_xyz[0], to_unit_xyz[1], to_unit_xyz[2], M, (int)P, out);
  return (int)hipGetLastError();
}
