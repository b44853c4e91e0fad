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
// The per-pixel arithmetic is that of slice_acq_fwd<float, false, true> (slice_acq.hip; INTERP_PSF off, no volume mask):
// the same affine map in double rounded once, the same tap skip rule, corner order and val / wsum, so the valid set is
// the one that operator produces.  (The skip test is written in its negated form: a NaN coordinate skips the tap instead
// of indexing the volume.)
//
// The sums are added in the reproducible order of slice_sums.h.  A workgroup serves all poses of its 256 pixels, so it parks
// the wave sums per pose inside the pose loop and combines them after one barrier at the end, in that header's order.
#include <hip/hip_runtime.h>
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kMaxTaps = 1024;
constexpr int kSums = 6;

struct Tap { float x, y, z, w; };

// grid: n * wgs workgroups of 256 pixels, wgs = ceil(h w / 256) per slice.  transforms: (n, K, 3, 4), this pass covers poses
// k0 .. k0 + KT - 1.  partial: (n, K, wgs, 6) doubles.
template <int KT>
__global__ __launch_bounds__(256) void svr_similarity_kernel(const float* __restrict__ vol, int D, int H, int W,
                                                             const float* __restrict__ psf, int d_p, int h_p, int w_p,
                                                             const float* __restrict__ transforms, const float* __restrict__ slices,
                                                             const uint8_t* __restrict__ slices_mask, int K, int k0, int h, int w,
                                                             int wgs, float res_slice, double* __restrict__ partial) {
  __shared__ Tap taps[kMaxTaps];
  __shared__ int n_taps;
  __shared__ float red[4][KT][kSums];
  if (threadIdx.x == 0) {
    int cnt = 0, ip = 0;
    for (int iz = -d_p / 2; iz < (d_p + 1) / 2; ++iz)
      for (int iy = -h_p / 2; iy < (h_p + 1) / 2; ++iy)
        for (int ix = -w_p / 2; ix < (w_p + 1) / 2; ++ix, ++ip) {
          const float pv = psf[ip];
          if (pv != 0.f) taps[cnt++] = Tap{(float)ix, (float)iy, (float)iz, pv};  // the host checked d_p h_p w_p <= kMaxTaps
        }
    n_taps = cnt;
  }
  __syncthreads();
  const int in = blockIdx.x / wgs, wg = blockIdx.x - in * wgs;
  const int pix = wg * 256 + (int)threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool inside = pix < h * w;
  const size_t idx = (size_t)in * h * w + (inside ? pix : 0);
  const bool on = inside && (slices_mask == nullptr || slices_mask[idx]);
  const float J = on ? slices[idx] : 0.f;
  const int ix = pix % w, iy = pix / w;
  const int Sy = W, Sz = H * W;
  const int nt = n_taps;
#pragma unroll 1
  for (int k = 0; k < KT; ++k) {
    float I = 0.f;
    bool valid = false;
    if (on) {  // (a wave without a masked-in pixel branches over its tap loops: its exec mask is empty)
      const float* t = transforms + ((size_t)in * K + k0 + k) * 12;  // wave-uniform: the scalar path
      const float r11 = t[0], r12 = t[1], r13 = t[2], r21 = t[4], r22 = t[5], r23 = t[6], r31 = t[8], r32 = t[9], r33 = t[10];
      const float px = (float)((ix - (w - 1) / 2.) * (double)res_slice + (double)t[3]);
      const float py = (float)((iy - (h - 1) / 2.) * (double)res_slice + (double)t[7]);
      const float pz = t[11];
      const float xc = r11 * px + r12 * py + r13 * pz + (W - 1) / 2.0f;
      const float yc = r21 * px + r22 * py + r23 * pz + (H - 1) / 2.0f;
      const float zc = r31 * px + r32 * py + r33 * pz + (D - 1) / 2.0f;
      float val = 0.f, wsum = 0.f;
      for (int j = 0; j < nt; ++j) {
        const Tap tp = taps[j];
        const float x = xc + r11 * tp.x + r12 * tp.y + r13 * tp.z;
        const float y = yc + r21 * tp.x + r22 * tp.y + r23 * tp.z;
        const float z = zc + r31 * tp.x + r32 * tp.y + r33 * tp.z;
        if (!(x >= 0 && y >= 0 && z >= 0 && x < W - 1 && y < H - 1 && z < D - 1)) continue;
        const int xf = (int)floorf(x), yf = (int)floorf(y), zf = (int)floorf(z);
        const float wx = x - xf, wy = y - yf, wz = z - zf;
        const int iv = zf * Sz + yf * Sy + xf;
        // corner order as the operator accumulates: 000,100,010,001,110,101,011,111
        const int off[8] = {0, 1, Sy, Sz, 1 + Sy, 1 + Sz, Sy + Sz, 1 + Sy + Sz};
        const float cw[8] = {(1 - wx) * (1 - wy) * (1 - wz), wx * (1 - wy) * (1 - wz), (1 - wx) * wy * (1 - wz),
                             (1 - wx) * (1 - wy) * wz,       wx * wy * (1 - wz),       wx * (1 - wy) * wz,
                             (1 - wx) * wy * wz,             wx * wy * wz};
        float v8[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v8[c] = vol[iv + off[c]];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float pw = cw[c] * tp.w;
          val += pw * v8[c];
          wsum += pw;
        }
      }
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

extern "C" int nesvor_svr_similarity(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                                     const float* transforms, const float* slices, const uint8_t* slices_mask, int n, int K,
                                     int h, int w, float res_slice, double* sums, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (K <= 0 || n == 0) return 0;
  if (D < 1 || H < 1 || W < 1 || h < 1 || w < 1 || n < 1 || d_p < 1 || h_p < 1 || w_p < 1) return (int)hipErrorInvalidValue;
  if ((int64_t)d_p * h_p * w_p > kMaxTaps) return (int)hipErrorInvalidValue;
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
      hipLaunchKernelGGL((svr_similarity_kernel<13>), grid, block, 0, st, vol, D, H, W, psf, d_p, h_p, w_p, transforms, slices,
                         slices_mask, K, k, h, w, (int)wgs, res_slice, partial);
      k += 13;
    } else {
      hipLaunchKernelGGL((svr_similarity_kernel<1>), grid, block, 0, st, vol, D, H, W, psf, d_p, h_p, w_p, transforms, slices,
                         slices_mask, K, k, h, w, (int)wgs, res_slice, partial);
      k += 1;
    }
  }
  plan.reduce(workspace, sums, st);
  return (int)hipGetLastError();
}
