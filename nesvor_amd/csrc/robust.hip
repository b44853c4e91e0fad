// E-step of the robust statistics of the classical reconstruction (gfx950): pixel posteriors and per-slice sums in one pass.
//
// The EM scheme of Kuklisova-Murgasova et al. 2012 (nesvor_amd/robust.py) models a pixel's residual as a mixture of a
// Gaussian inlier (variance sigma2, proportion c) and a uniform outlier (density m).  For every valid pixel (mask byte set,
// or no mask) of slice k
//   e = scale_k * y - sim,   g = exp(-e^2 / (2 sigma2)) / sqrt(2 pi sigma2),   p = c g / (c g + (1 - c) m)
// and p = 0 elsewhere.  Everything the M-step, the slice potentials and the slice scales need follows from seven sums per
// slice over its valid pixels:
//   { n, sum p, sum p e^2, sum (1 - p)^2, sum p y sim, sum p y^2, sum e^2 }.
// Composed from torch operators one round is about 25 launches over slice-sized temporaries and a dozen reductions; here it is
// one pass that reads sim, y and the mask (9 bytes per pixel) and writes p (4 bytes), and a small reduce launch.  sim = A x is
// an input: the PSF tap loop stays in slice_acq.hip.
//
// The per-pixel arithmetic is that of the torch expression of robust.py::estep_composed in fp32, operation for operation (the
// build has -ffp-contract=off; sqrtf and / are correctly rounded, expf is the library's, the one torch's fp32 exp calls).  {sigma2, c, m} are read from device memory:
// the EM loop never synchronises with the host.
//
// Sums are reproducible, as in svr.hip: fp32 only inside one wave's DPP reduction (64 terms), then double; every workgroup
// stores its seven partials to the workspace and a second small launch adds them in workgroup order.  No atomics, no memset.
// The count is exact (at most 64 ones per wave in fp32, integers in double from there).
#include <hip/hip_runtime.h>
#include <limits.h>
#include "common.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kStats = 7;

// grid: n * wgs workgroups of 256 pixels, wgs = ceil(hw / 256) per slice.  partial: (n, wgs, 7) doubles.
__global__ __launch_bounds__(256) void robust_estep_kernel(const float* __restrict__ sim, const float* __restrict__ y,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                                           const float* __restrict__ model, int hw, int wgs, float* __restrict__ p,
                                                           double* __restrict__ partial) {
  __shared__ float red[4][kStats];
  const int in = blockIdx.x / wgs, wg = blockIdx.x - in * wgs;
  const int pix = wg * 256 + (int)threadIdx.x;  // the host checked hw <= INT_MAX - 256
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool inside = pix < hw;
  const size_t idx = (size_t)in * hw + (inside ? pix : 0);
  const bool on = inside && (mask == nullptr || mask[idx]);
  const float sigma2 = model[0], c = model[1], m = model[2], s = scale[in];  // workgroup-uniform: the scalar path
  float pv = 0.f, e2 = 0.f, q2 = 0.f, pys = 0.f, pyy = 0.f;
  if (on) {
    const float yv = y[idx], sv = sim[idx];
    const float e = s * yv - sv;
    e2 = e * e;
    const float g = expf(-e2 / (2.f * sigma2)) / sqrtf(6.2831853071795864769f * sigma2);
    const float cg = c * g;
    pv = cg / (cg + (1.f - c) * m);
    const float q = 1.f - pv, py = pv * yv;
    q2 = q * q;
    pys = py * sv;
    pyy = py * yv;
  }
  if (inside) p[idx] = pv;
  const float s0 = wave_sum_dpp(on ? 1.f : 0.f), s1 = wave_sum_dpp(pv), s2 = wave_sum_dpp(pv * e2), s3 = wave_sum_dpp(q2),
              s4 = wave_sum_dpp(pys), s5 = wave_sum_dpp(pyy), s6 = wave_sum_dpp(e2);
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3;
    red[wave][4] = s4; red[wave][5] = s5; red[wave][6] = s6;
  }
  __syncthreads();
  if (threadIdx.x < kStats) {
    const int j = threadIdx.x;
    const double t = ((double)red[0][j] + (double)red[1][j]) + ((double)red[2][j] + (double)red[3][j]);
    partial[((size_t)in * wgs + wg) * kStats + j] = t;
  }
}

// stats[k][j] = the partials of slice k added in workgroup order
__global__ __launch_bounds__(256) void robust_reduce_kernel(const double* __restrict__ partial, int64_t total, int wgs,
                                                            double* __restrict__ stats) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t k = t / kStats;
  const int j = (int)(t - k * kStats);
  double s = 0.0;
  for (int g = 0; g < wgs; ++g) s += partial[((size_t)k * wgs + g) * kStats + j];
  stats[t] = s;
}

}  // namespace

extern "C" int64_t nesvor_robust_estep_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  const int64_t wgs = ((int64_t)h * w + 255) / 256;
  return (int64_t)sizeof(double) * kStats * n * wgs;
}

extern "C" int nesvor_robust_estep(const float* sim, const float* y, const uint8_t* mask, const float* scale, const float* model,
                                   int n, int h, int w, float* p, double* stats, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (n == 0) return 0;
  if (n < 0 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (sim == nullptr || y == nullptr || scale == nullptr || model == nullptr || p == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  // pixel indices inside a slice are ints; one workgroup per 256 pixels of a slice
  if ((int64_t)h * w > INT_MAX - 256) return (int)hipErrorInvalidValue;
  const int64_t wgs = ((int64_t)h * w + 255) / 256;
  if (wgs * n > INT_MAX) return (int)hipErrorInvalidValue;
  const int64_t need = nesvor_robust_estep_workspace_bytes(n, h, w);
  if (workspace == nullptr || (int64_t)workspace_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(robust_estep_kernel, dim3((unsigned)(wgs * n)), dim3(256), 0, st, sim, y, mask, scale, model, h * w, (int)wgs, p,
                     partial);
  const int64_t total = (int64_t)n * kStats;
  hipLaunchKernelGGL(robust_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)partial, total,
                     (int)wgs, stats);
  return (int)hipGetLastError();
}
