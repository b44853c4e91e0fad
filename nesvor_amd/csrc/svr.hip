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
// A pixel's value under a pose comes from the functions slice_acq_fwd<float, false, true> calls (acq_taps.h: pixel_geom, the LDS
// tap list, the inside test, linear_tap without a volume mask) and the same val / wsum, so value and valid set are that
// operator's bit for bit.
//
// The sums are added in the reproducible order of slice_sums.h.  A workgroup serves all poses of its 256 pixels, so it parks
// the wave sums per pose inside the pose loop and combines them after one barrier at the end, in that header's order.
#include <hip/hip_runtime.h>
#include "acq_taps.h"
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {
using namespace acq;

constexpr int kSums = 6;

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
  if (threadIdx.x == 0) {
    const PsfView<float> pk = psfs.at(in);
    n_taps = compact_taps(pk.psf, pk.d, pk.h, pk.w, taps);
  }
  __syncthreads();
  const int pix = wg * 256 + (int)threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool inside = pix < h * w;
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
      const float* t = transforms + ((size_t)in * K + k0 + k) * 12;  // wave-uniform: the scalar path
      const PixelGeom<float> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
      float val = 0.f, wsum = 0.f;
      for_lds_taps(t, g, taps, nt, D, H, W, [&](float, float, float, float pv, float x, float y, float z) {
        linear_tap(vol, (const uint8_t*)nullptr, trilinear_cell(x, y, z, H, W), pv, val, wsum);
      });
      if (wsum > 0) { I = val / wsum; valid = true; }
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
    partial[(((size_t)in * K + k0 + k) * wgs + wg) * kSums + j] = s;
  }
}

}  // namespace

extern "C" int64_t nesvor_svr_similarity_workspace_bytes(int n, int K, int h, int w) {
  if (n < 1 || K < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kSums>{(int64_t)n * K, slice_sums::pixel_workgroups(h, w)}.workspace_bytes();
}

namespace {
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
  int k = 0;
  while (k < K) {  // 13 poses per pass (one finite-difference gradient), single poses otherwise
    if (K - k >= 13) {
      hipLaunchKernelGGL((svr_similarity_kernel<13, PSF>), grid, block, 0, st, vol, D, H, W, psfs, transforms, slices, slices_mask, K,
                         k, h, w, (int)wgs, res_slice, partial);
      k += 13;
    } else {
      hipLaunchKernelGGL((svr_similarity_kernel<1, PSF>), grid, block, 0, st, vol, D, H, W, psfs, transforms, slices, slices_mask, K,
                         k, h, w, (int)wgs, res_slice, partial);
      k += 1;
    }
  }
  plan.reduce(workspace, sums, st);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int nesvor_svr_similarity(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                                     const float* transforms, const float* slices, const uint8_t* slices_mask, int n, int K,
                                     int h, int w, float res_slice, double* sums, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (K <= 0 || n == 0) return 0;
  if (d_p < 1 || h_p < 1 || w_p < 1 || (int64_t)d_p * h_p * w_p > kMaxTaps) return (int)hipErrorInvalidValue;
  return svr_similarity_launch(vol, D, H, W, OnePsf<float>{psf, d_p, h_p, w_p}, transforms, slices, slices_mask, n, K, h, w, res_slice,
                               sums, workspace, workspace_bytes, stream);
}

// The same sums with a PSF bank: slice i is simulated with PSF psf_id[i].  Refused if ANY member has more than kMaxTaps elements.
extern "C" int nesvor_svr_similarity_bank(const float* vol, int D, int H, int W, const float* psf_bank, const int32_t* psf_table,
                                          int P, const int32_t* psf_id, const float* transforms, const float* slices,
                                          const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, double* sums,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  BankPsf<float> bank;
  int64_t max_elements;
  if (!make_bank(psf_bank, psf_table, P, psf_id, n, bank, max_elements) || max_elements > kMaxTaps) return (int)hipErrorInvalidValue;
  if ((int64_t)D * H * W > INT_MAX) return (int)hipErrorInvalidValue;
  if (K <= 0 || n == 0) return 0;
  return svr_similarity_launch(vol, D, H, W, bank, transforms, slices, slices_mask, n, K, h, w, res_slice, sums, workspace,
                               workspace_bytes, stream);
}
