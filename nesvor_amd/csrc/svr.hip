// Similarity sums for slice-to-volume rigid registration (gfx950): the batched, PSF-aware sibling of vvr.hip.
//
// One finite-difference gradient of the slice registration needs, for every slice, the acquisition operator A applied
// under K = 1 + 2 x 6 poses and the masked moment sums of (simulated, acquired) per (slice, pose).  Composed from the
// existing operators that is K slice_acq_fwd launches plus a few dozen small reductions; here one launch simulates every
// pixel under all K poses of its slice - the acquired value, the mask byte and the LDS tap list are read once - and
// returns per (slice, pose), over the VALID pixels (mask set and PSF weight > 0),
//   { count, sum I, sum I^2, sum I J, sum J, sum J^2 },   I = simulated, J = acquired,
// from which NCC and MSE follow.
//
// A pixel's value under a pose is acq_taps.h's simulate_pixel: the functions slice_acq_fwd<float, false, true> calls and the same
// val / wsum, so value and valid set are that operator's bit for bit.
//
// The sums are added in the reproducible order of slice_sums.h.  A workgroup serves all poses of its 256 pixels, so it parks
// the wave sums per pose inside the pose loop and combines them after one barrier at the end, in that header's order.
//
// Package registration (GroupSVR) moves GROUPS of slices together: svr_similarity_groups_kernel takes one correction per (group,
// pose) and a CSR grouping, composes the correction with each slice's base pose once per workgroup and runs the same pixel loop
// (similarity_pixels); svr_groups_reduce_kernel adds a group's per-slice sums in CSR order.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "acq_taps.h"
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {
using namespace acq;

constexpr int kSums = 6;

// The pixel loop of both kernels: the workgroup's 256 pixels of slice `in` under the KT poses pose_of(0 .. KT-1) (12 floats each,
// wave-uniform), the six sums per pose added in slice_sums.h's steps 1-2 and stored to rows (entry K + k0 + k) wgs + wg of
// `partial`.  `entry` is the slice itself (svr_similarity_kernel) or the slice's place in a grouping (svr_similarity_groups_kernel);
// `live` false: no pixel of the workgroup counts and nothing is indexed by `in`.  Every thread must call (barrier).
template <int KT, typename PoseOf>
__device__ __forceinline__ void similarity_pixels(const float* __restrict__ vol, int D, int H, int W, const Tap<float>* taps, const int& n_taps,
                                                  float (&red)[4][KT][kSums], PoseOf pose_of, const float* __restrict__ slices,
                                                  const uint8_t* __restrict__ slices_mask, bool live, int in, int64_t entry, int wg,
                                                  int K, int k0, int h, int w, int wgs, float res_slice,
                                                  double* __restrict__ partial) {
  const int pix = wg * 256 + (int)threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool inside = live && pix < h * w;
  const size_t idx = (size_t)in * h * w + (inside ? pix : 0);
  const bool on = inside && (slices_mask == nullptr || slices_mask[idx]);
  const float J = on ? slices[idx] : 0.f;
  const int ix = pix % w, iy = pix / w;
  const int nt = n_taps;
#pragma unroll 1
  for (int k = 0; k < KT; ++k) {
    float I = 0.f;
    bool valid = false;
    if (on) {  // (a wave without a masked-in pixel branches over its tap loops: its exec mask is empty)
      valid = simulate_pixel(vol, D, H, W, pose_of(k) /* wave-uniform */, ix, iy, h, w, res_slice, taps, nt, I);
    }
    // this pose's six values leave the registers at once: wave sums, parked in LDS per (wave, pose)
    const float Jv = valid ? J : 0.f;
    const float s0 = wave_sum_dpp(valid ? 1.f : 0.f), s1 = wave_sum_dpp(I), s2 = wave_sum_dpp(I * I), s3 = wave_sum_dpp(I * Jv),
                s4 = wave_sum_dpp(Jv), s5 = wave_sum_dpp(Jv * Jv);
    if (lane == 0) {
      red[wave][k][0] = s0; red[wave][k][1] = s1; red[wave][k][2] = s2;
      red[wave][k][3] = s3; red[wave][k][4] = s4; red[wave][k][5] = s5;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < KT * kSums; e += blockDim.x) {
    const int k = e / kSums, j = e - k * kSums;
    const double s = ((double)red[0][k][j] + (double)red[1][k][j]) + ((double)red[2][k][j] + (double)red[3][k][j]);
    partial[(((size_t)entry * K + k0 + k) * wgs + wg) * kSums + j] = s;
  }
}

// grid: n * wgs workgroups of 256 pixels, wgs = ceil(h w / 256) per slice.  transforms: (n, K, 3, 4), this pass covers poses
// k0 .. k0 + KT - 1.  partial: (n, K, wgs, 6) doubles.  PSF: OnePsf<float>, or BankPsf<float> - the workgroup's slice then compacts
// its own PSF (acq_taps.h).
template <int KT, typename PSF>
__global__ __launch_bounds__(256) void svr_similarity_kernel(const float* __restrict__ vol, int D, int H, int W, const PSF psfs,
                                                             const float* __restrict__ transforms, const float* __restrict__ slices,
                                                             const uint8_t* __restrict__ slices_mask, int K, int k0, int h, int w,
                                                             int wgs, float res_slice, double* __restrict__ partial) {
  __shared__ Tap<float> taps[kMaxTaps];
  __shared__ int n_taps;
  __shared__ float red[4][KT][kSums];
  const int in = blockIdx.x / wgs, wg = blockIdx.x - in * wgs;
  workgroup_taps(psfs, true, in, taps, n_taps);
  __syncthreads();
  similarity_pixels<KT>(vol, D, H, W, taps, n_taps, red,
                        [&](int k) { return transforms + ((size_t)in * K + k0 + k) * 12; },  // the scalar path
                        slices, slices_mask, true, in, in, wg, K, k0, h, w, wgs, res_slice, partial);
}

// ---- grouped sums: one correction per (group, pose), composed with every slice's base pose in the kernel ----
// Element j of  correction o base  (RigidTransform.compose: R' = Rc R, t' = t + R^T uc; both 3 x 4 row-major, translation first),
// in double from the fp32 inputs, every sum of products added left to right (the build does not contract), rounded once.
__device__ __forceinline__ float composed_element(const float* __restrict__ c, const float* __restrict__ b, int j) {
  const int i = j >> 2, col = j & 3;
  if (col < 3)
    return (float)((double)c[4 * i] * (double)b[col] + (double)c[4 * i + 1] * (double)b[4 + col] + (double)c[4 * i + 2] * (double)b[8 + col]);
  const double rtu = (double)b[i] * (double)c[3] + (double)b[4 + i] * (double)c[7] + (double)b[8 + i] * (double)c[11];
  return (float)((double)b[4 * i + 3] + rtu);
}

// The group of entry e: offsets[g] <= e < offsets[g + 1] (offsets non-decreasing from 0, e < offsets[G]; empty groups are skipped).
__device__ __forceinline__ int group_of_entry(const int* __restrict__ offsets, int G, int e) {
  int lo = 0, hi = G;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// grid: E * wgs workgroups, one entry of the grouping (a slice of a group) per wgs of them.  base: (n, 3, 4), corrections: (G, K, 3, 4),
// partial: (E, K, wgs, 6) doubles.  The KT composed poses are wave-uniform: threads < 12 KT compose one element each into LDS, once
// per workgroup, and the pixel loop reads them there.  A slice index outside [0, n) (the caller's error: ops.py refuses it on
// the host) indexes nothing and gives the entry six zeros.
template <int KT, typename PSF>
__global__ __launch_bounds__(256) void svr_similarity_groups_kernel(const float* __restrict__ vol, int D, int H, int W, const PSF psfs,
                                                                    const float* __restrict__ base, const float* __restrict__ corrections,
                                                                    const int* __restrict__ group_offsets, int G,
                                                                    const int* __restrict__ group_slices, const float* __restrict__ slices,
                                                                    const uint8_t* __restrict__ slices_mask, int n, int K, int k0, int h,
                                                                    int w, int wgs, float res_slice, double* __restrict__ partial) {
  __shared__ Tap<float> taps[kMaxTaps];
  __shared__ int n_taps;
  __shared__ float red[4][KT][kSums];
  __shared__ float poses[KT][12];
  const int e = blockIdx.x / wgs, wg = blockIdx.x - e * wgs;
  const int listed = group_slices[e];
  const bool live = listed >= 0 && listed < n;
  const int in = live ? listed : 0;
  workgroup_taps(psfs, live, in, taps, n_taps);
  if (live && threadIdx.x < KT * 12) {
    const int k = threadIdx.x / 12, j = threadIdx.x - k * 12;
    const int g = group_of_entry(group_offsets, G, e);
    poses[k][j] = composed_element(corrections + ((size_t)g * K + k0 + k) * 12, base + (size_t)in * 12, j);
  }
  __syncthreads();
  similarity_pixels<KT>(vol, D, H, W, taps, n_taps, red, [&](int k) { return (const float*)poses[k]; }, slices, slices_mask, live, in,
                        e, wg, K, k0, h, w, wgs, res_slice, partial);
}

// sums[g][k][j] = the entries of group g one after the other from 0, in CSR order; an entry's sum is its wgs rows added from 0 in
// workgroup order (slice_sums.h's step 3, per entry).  One thread per (g, k, j); an empty group stores 0.
__global__ __launch_bounds__(256) void svr_groups_reduce_kernel(const double* __restrict__ partial, const int* __restrict__ group_offsets,
                                                                int G, int K, int wgs, double* __restrict__ sums) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)G * K * kSums) return;
  const int64_t gk = t / kSums;
  const int j = (int)(t - gk * kSums);
  const int g = (int)(gk / K), k = (int)(gk - (int64_t)g * K);
  double s = 0.0;
  for (int e = group_offsets[g]; e < group_offsets[g + 1]; ++e) {
    double se = 0.0;
    for (int r = 0; r < wgs; ++r) se += partial[(((size_t)e * K + k) * wgs + r) * kSums + j];
    s += se;
  }
  sums[t] = s;
}

}  // namespace

extern "C" int64_t nesvor_svr_similarity_workspace_bytes(int n, int K, int h, int w) {
  if (n < 1 || K < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kSums>{(int64_t)n * K, slice_sums::pixel_workgroups(h, w)}.workspace_bytes();
}

namespace {
// The K poses of a call in passes: 13 poses per pass (one finite-difference gradient), single poses otherwise.
// pass(std::integral_constant<int, KT>, k0) launches poses k0 .. k0 + KT - 1.
template <typename Pass> void for_pose_passes(int K, Pass pass) {
  for (int k = 0; k < K;) {
    if (K - k >= 13) {
      pass(std::integral_constant<int, 13>{}, k);
      k += 13;
    } else {
      pass(std::integral_constant<int, 1>{}, k);
      k += 1;
    }
  }
}

// The launches of both entry points, behind their checks of the PSF source.
template <typename PSF>
int svr_similarity_launch(const float* vol, int D, int H, int W, const PSF& psfs, const float* transforms, const float* slices,
                          const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, double* sums, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (D < 1 || H < 1 || W < 1 || h < 1 || w < 1 || n < 1) return (int)hipErrorInvalidValue;
  // voxel indices are ints; an entry is a (slice, pose), a workgroup serves all poses of its 256 pixels
  if ((int64_t)D * H * W > INT_MAX || (int64_t)n * K > INT_MAX) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kSums> plan{(int64_t)n * K, slice_sums::pixel_workgroups(h, w)};
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int64_t wgs = plan.wgs;
  const dim3 grid((unsigned)(wgs * n)), block(256);
  for_pose_passes(K, [&](auto kt, int k0) {
    hipLaunchKernelGGL((svr_similarity_kernel<decltype(kt)::value, PSF>), grid, block, 0, st, vol, D, H, W, psfs, transforms, slices,
                       slices_mask, K, k0, h, w, (int)wgs, res_slice, partial);
  });
  plan.reduce(workspace, sums, st);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int nesvor_svr_similarity(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                                     const float* transforms, const float* slices, const uint8_t* slices_mask, int n, int K,
                                     int h, int w, float res_slice, double* sums, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (K <= 0 || n == 0) return 0;
  OnePsf<float> one;
  if (!lds_one_psf(psf, d_p, h_p, w_p, D, H, W, one)) return (int)hipErrorInvalidValue;
  return svr_similarity_launch(vol, D, H, W, one, transforms, slices, slices_mask, n, K, h, w, res_slice, sums, workspace,
                               workspace_bytes, stream);
}

// The same sums with a PSF bank: slice i is simulated with PSF psf_id[i].  Refused if ANY member has more than kMaxTaps elements.
extern "C" int nesvor_svr_similarity_bank(const float* vol, int D, int H, int W, const float* psf_bank, const int32_t* psf_table,
                                          int P, const int32_t* psf_id, const float* transforms, const float* slices,
                                          const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, double* sums,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  BankPsf<float> bank;
  if (!lds_bank_psf(psf_bank, psf_table, P, psf_id, n, D, H, W, bank)) return (int)hipErrorInvalidValue;
  if (K <= 0 || n == 0) return 0;
  return svr_similarity_launch(vol, D, H, W, bank, transforms, slices, slices_mask, n, K, h, w, res_slice, sums, workspace,
                               workspace_bytes, stream);
}

// ---- grouped sums (package registration): the same pixels, poses composed in the kernel, sums per (group, pose) ----
extern "C" int64_t nesvor_svr_similarity_groups_workspace_bytes(int E, int K, int h, int w) {
  return nesvor_svr_similarity_workspace_bytes(E, K, h, w);  // (an entry in the place of a slice)
}

namespace {
// What both grouped entry points refuse about the grouping itself.
inline bool grouping_accepted(const int32_t* group_offsets, const int32_t* group_slices, int G, int E) {
  return G >= 1 && E >= 0 && group_offsets != nullptr && (E == 0 || group_slices != nullptr);
}

template <typename PSF>
int svr_similarity_groups_launch(const float* vol, int D, int H, int W, const PSF& psfs, const float* base, const float* corrections,
                                 const int32_t* group_offsets, const int32_t* group_slices, int G, int E, const float* slices,
                                 const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, double* sums, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (D < 1 || H < 1 || W < 1 || h < 1 || w < 1 || n < 1) return (int)hipErrorInvalidValue;
  if ((int64_t)D * H * W > INT_MAX || (int64_t)E * K > INT_MAX || (int64_t)G * K > INT_MAX / kSums) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kSums> plan{(int64_t)E * K, slice_sums::pixel_workgroups(h, w)};
  if (!plan.accepts(h, w, plan.wgs * E, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int wgs = (int)plan.wgs;
  const dim3 grid((unsigned)(plan.wgs * E)), block(256);  // over the entries: a subset costs what it holds
  for_pose_passes(K, [&](auto kt, int k0) {
    hipLaunchKernelGGL((svr_similarity_groups_kernel<decltype(kt)::value, PSF>), grid, block, 0, st, vol, D, H, W, psfs, base, corrections,
                       group_offsets, G, group_slices, slices, slices_mask, n, K, k0, h, w, wgs, res_slice, partial);
  });
  const int64_t total = (int64_t)G * K * kSums;
  hipLaunchKernelGGL(svr_groups_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)partial,
                     group_offsets, G, K, wgs, sums);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int nesvor_svr_similarity_groups(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                                            const float* base, const float* corrections, const int32_t* group_offsets,
                                            const int32_t* group_slices, int G, int E, const float* slices,
                                            const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, double* sums,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!grouping_accepted(group_offsets, group_slices, G, E)) return (int)hipErrorInvalidValue;
  if (K <= 0 || E == 0) return 0;
  OnePsf<float> one;
  if (!lds_one_psf(psf, d_p, h_p, w_p, D, H, W, one)) return (int)hipErrorInvalidValue;
  return svr_similarity_groups_launch(vol, D, H, W, one, base, corrections, group_offsets, group_slices, G, E, slices, slices_mask, n, K,
                                      h, w, res_slice, sums, workspace, workspace_bytes, stream);
}

extern "C" int nesvor_svr_similarity_groups_bank(const float* vol, int D, int H, int W, const float* psf_bank,
                                                 const int32_t* psf_table, int P, const int32_t* psf_id, const float* base,
                                                 const float* corrections, const int32_t* group_offsets, const int32_t* group_slices,
                                                 int G, int E, const float* slices, const uint8_t* slices_mask, int n, int K, int h,
                                                 int w, float res_slice, double* sums, void* workspace, size_t workspace_bytes,
                                                 void* stream) {
  if (!grouping_accepted(group_offsets, group_slices, G, E)) return (int)hipErrorInvalidValue;
  BankPsf<float> bank;
  if (!lds_bank_psf(psf_bank, psf_table, P, psf_id, n, D, H, W, bank)) return (int)hipErrorInvalidValue;
  if (K <= 0 || E == 0) return 0;
  return svr_similarity_groups_launch(vol, D, H, W, bank, base, corrections, group_offsets, group_slices, G, E, slices, slices_mask, n, K,
                                      h, w, res_slice, sums, workspace, workspace_bytes, stream);
}
