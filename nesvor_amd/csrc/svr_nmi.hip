// Joint histograms for the mutual-information similarity of the slice-to-volume registration (gfx950): the sibling of svr.hip
// whose statistic per (slice, pose) is not six moments but a B x B histogram of (simulated, acquired) intensities.
//
// The definition (nesvor_amd/nmi.py states it once; the composed path and the tests use that statement).  Each axis maps a value
// to bin coordinates with an affine map (lo, scale) the host computed in fp32:
//   u = clamp((v - lo) * scale, 0, B - 1),  b0 = min((int)u, B - 2),  f = u - b0,  q = (int)(f * 256 + 0.5)  in [0, 256]
// (fp32, every operation rounded on its own: the build does not contract); the value gives weight 256 - q to bin b0 and q to bin
// b0 + 1.  A valid pixel (mask set and PSF weight > 0: svr_similarity's valid set) adds the four integer products of its I weights
// and its J weights to the cells (bI, bJ), 65536 units in all, zero products skipped.  Integer adds: the histogram does not depend
// on the order of addition, so LDS atomics are reproducible here and no float atomic is used.
//
// nmi_hist.h holds what this file shares with the stack registration's histograms (vvr_nmi.hip): axis_place, the four adds of a
// sample, the segment rule and the 64-bit reduction of the segments.
//
// A pixel's value under a pose is acq_taps.h's simulate_pixel, as svr_similarity_kernel's: the functions slice_acq_fwd<float, false,
// true> calls and the same val / wsum, so I and the valid set are that operator's bit for bit.
//
// Shape.  A slice's pixels are cut into segments; one workgroup serves one (slice, pose, segment): it keeps the histogram in LDS
// (B B 32-bit cells, at most 16 KB, next to the 16 KB tap list), walks its pixels 256 at a time, adds with integer LDS atomics and
// stores the cells to its own rows of the workspace with plain stores; a second launch adds the segments of a (slice, pose) in
// 64 bits.  The segment length is the launch's (segment_pixels): a call with many (slice, pose) entries - the 13 poses of a
// gradient - takes whole slices, one workgroup per entry, which pays the tap list and the histogram's clear and store once per
// entry; a call with few entries - the K = 1 accept test - cuts its slices until about kTargetWorkgroups workgroups fill the chip
// ("Mutual-information similarity", has the measurements behind both).  No cell can overflow: a segment holds at most
// kMaxSegmentPixels <= 65535 pixels of at most 65536 units each, below 2^32; the result in memory is 64-bit.  No global atomics, no
// memset: every row of the workspace is written by exactly one workgroup before the second launch reads it.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "acq_taps.h"
#include "nmi_hist.h"
#include "../../include/nesvor_hip.h"

namespace {
using namespace acq;
using namespace nmi_hist;

// grid: n K S workgroups, S = ceil(h w / seg) segments of `seg` pixels per (slice, pose); block e S + s serves segment s of entry
// e = slice K + pose.  partial: (n K, S, B, B) 32-bit cells, row = I bin.
template <typename PSF>
__global__ __launch_bounds__(256) void svr_joint_histogram_kernel(const float* __restrict__ vol, int D, int H, int W, const PSF psfs,
                                                                  const float* __restrict__ transforms, const float* __restrict__ slices,
                                                                  const uint8_t* __restrict__ slices_mask, int K, int h, int w, int S,
                                                                  int seg, float res_slice, float i_lo, float i_scale,
                                                                  const float* __restrict__ j_map, int B, uint32_t* __restrict__ partial) {
  __shared__ Tap<float> taps[kMaxTaps];
  __shared__ int n_taps;
  __shared__ uint32_t hist[kMaxNmiBins * kMaxNmiBins];
  const int e = blockIdx.x / S, s = blockIdx.x - e * S;
  const int in = e / K;
  const int cells = B * B;
  for (int c = threadIdx.x; c < cells; c += 256) hist[c] = 0u;
  workgroup_taps(psfs, true, in, taps, n_taps);
  __syncthreads();
  const float* t = transforms + (size_t)e * 12;  // wave-uniform: the scalar path
  const float j_lo = j_map[2 * in], j_scale = j_map[2 * in + 1];
  const int nt = n_taps;
  const int first = s * seg;  // (below h w: S = ceil(h w / seg))
  const int last = (int)min((int64_t)first + seg, (int64_t)h * w);
  for (int pix = first + (int)threadIdx.x; pix < last; pix += 256) {
    const size_t idx = (size_t)in * h * w + pix;
    if (slices_mask != nullptr && !slices_mask[idx]) continue;
    float I;
    if (!simulate_pixel(vol, D, H, W, t, pix % w, pix / w, h, w, res_slice, taps, nt, I)) continue;
    const AxisPlace a = axis_place(I, i_lo, i_scale, B), b = axis_place(slices[idx], j_lo, j_scale, B);
    add_sample(a, b, B, [&](int cell, uint32_t p) { atomicAdd(&hist[cell], p); });
  }
  __syncthreads();
  uint32_t* row = partial + (size_t)blockIdx.x * cells;
  for (int c = threadIdx.x; c < cells; c += 256) row[c] = hist[c];
}

// The segments a slice of h w pixels is cut into in a launch of `entries` (slice, pose) pairs (nmi_hist.h has the rule).
inline int64_t segments(int64_t entries, int h, int w) { return nmi_hist::segments(entries, (int64_t)h * w); }

// The launches of both entry points, behind their checks of the PSF source.
template <typename PSF>
int svr_joint_histogram_launch(const float* vol, int D, int H, int W, const PSF& psfs, const float* transforms, const float* slices,
                               const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, float i_lo, float i_scale,
                               const float* j_map, int bins, int64_t* hist, void* workspace, size_t workspace_bytes, void* stream) {
  if (D < 1 || H < 1 || W < 1 || h < 1 || w < 1 || n < 1) return (int)hipErrorInvalidValue;
  if (bins < 2 || bins > kMaxNmiBins || j_map == nullptr) return (int)hipErrorInvalidValue;
  // voxel and pixel indices are ints (a workgroup's last trip may index 255 past a slice's end), an entry is a (slice, pose)
  if ((int64_t)D * H * W > INT_MAX || (int64_t)n * K > INT_MAX || (int64_t)h * w > INT_MAX - 256) return (int)hipErrorInvalidValue;
  const int64_t entries = (int64_t)n * K, S = segments(entries, h, w), cells = (int64_t)bins * bins;
  if (entries * S > INT_MAX || entries * cells / 256 >= INT_MAX) return (int)hipErrorInvalidValue;  // both grids fit an int
  if (workspace == nullptr || (int64_t)workspace_bytes < (int64_t)sizeof(uint32_t) * entries * S * cells) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* partial = (uint32_t*)workspace;
  hipLaunchKernelGGL((svr_joint_histogram_kernel<PSF>), dim3((unsigned)(entries * S)), dim3(256), 0, st, vol, D, H, W, psfs, transforms,
                     slices, slices_mask, K, h, w, (int)S, segment_pixels(entries, (int64_t)h * w), res_slice, i_lo, i_scale, j_map, bins, partial);
  const int64_t total = entries * cells;
  hipLaunchKernelGGL(joint_histogram_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)partial,
                     total, (int)cells, (int)S, hist);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t nesvor_svr_joint_histogram_workspace_bytes(int n, int K, int h, int w, int bins) {
  if (n < 1 || K < 1 || h < 1 || w < 1 || bins < 2 || bins > kMaxNmiBins) return 0;
  return (int64_t)sizeof(uint32_t) * n * K * segments((int64_t)n * K, h, w) * bins * bins;
}

extern "C" int nesvor_svr_joint_histogram(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                                          const float* transforms, const float* slices, const uint8_t* slices_mask, int n, int K,
                                          int h, int w, float res_slice, float i_lo, float i_scale, const float* j_map, int bins,
                                          int64_t* hist, void* workspace, size_t workspace_bytes, void* stream) {
  if (K <= 0 || n == 0) return 0;
  OnePsf<float> one;
  if (!lds_one_psf(psf, d_p, h_p, w_p, D, H, W, one)) return (int)hipErrorInvalidValue;
  return svr_joint_histogram_launch(vol, D, H, W, one, transforms, slices, slices_mask, n, K, h, w, res_slice, i_lo, i_scale, j_map,
                                    bins, hist, workspace, workspace_bytes, stream);
}

// The same histograms with a PSF bank: slice i is simulated with PSF psf_id[i].  Refused if ANY member has more than kMaxTaps elements.
extern "C" int nesvor_svr_joint_histogram_bank(const float* vol, int D, int H, int W, const float* psf_bank, const int32_t* psf_table,
                                               int P, const int32_t* psf_id, const float* transforms, const float* slices,
                                               const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, float i_lo,
                                               float i_scale, const float* j_map, int bins, int64_t* hist, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  BankPsf<float> bank;
  if (!lds_bank_psf(psf_bank, psf_table, P, psf_id, n, D, H, W, bank)) return (int)hipErrorInvalidValue;
  if (K <= 0 || n == 0) return 0;
  return svr_joint_histogram_launch(vol, D, H, W, bank, transforms, slices, slices_mask, n, K, h, w, res_slice, i_lo, i_scale, j_map,
                                    bins, hist, workspace, workspace_bytes, stream);
}
