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
// The seven sums are added in the reproducible order of slice_sums.h: bit-identical from run to run, the count exact.
#include <hip/hip_runtime.h>
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kStats = 7;

// grid: n * wgs workgroups of 256 pixels, wgs = ceil(hw / 256) per slice.  partial: (n, wgs, 7) doubles.
__global__ __launch_bounds__(256) void robust_estep_kernel(const float* __restrict__ sim, const float* __restrict__ y,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                                           const float* __restrict__ model, int hw, int wgs, float* __restrict__ p,
                                                           double* __restrict__ partial) {
  const int in = blockIdx.x / wgs, wg = blockIdx.x - in * wgs;
  const int pix = wg * 256 + (int)threadIdx.x;  // the host checked hw <= INT_MAX - 256
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
  const float sums[kStats] = {wave_sum_dpp(on ? 1.f : 0.f), wave_sum_dpp(pv),  wave_sum_dpp(pv * e2), wave_sum_dpp(q2),
                              wave_sum_dpp(pys),            wave_sum_dpp(pyy), wave_sum_dpp(e2)};
  slice_sums::store_workgroup_sums(sums,partial + ((size_t)in * wgs + wg) * kStats);
}

}  // namespace

extern "C" int64_t nesvor_robust_estep_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kStats>{n, slice_sums::pixel_workgroups(h, w)}.workspace_bytes();
}

extern "C" int nesvor_robust_estep(const float* sim, const float* y, const uint8_t* mask, const float* scale, const float* model,
                                   int n, int h, int w, float* p, double* stats, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (n == 0) return 0;
  if (n < 0 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (sim == nullptr || y == nullptr || scale == nullptr || model == nullptr || p == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kStats> plan{n, slice_sums::pixel_workgroups(h, w)};
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(robust_estep_kernel, dim3((unsigned)(plan.wgs * n)), dim3(256), 0, st, sim, y, mask, scale, model, h * w,
                     (int)plan.wgs, p, (double*)workspace);
  plan.reduce(workspace, stats, st);
  return (int)hipGetLastError();
}
