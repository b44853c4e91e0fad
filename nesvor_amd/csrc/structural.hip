// Structural exclusion of the classical reconstruction (gfx950): the local SSIM map of the acquired slices against the simulated
// ones and the per-slice sums of the slice similarity, in one pass.
//
// Definition (nesvor_amd/structural.py::ssim_composed).  For slice k with I = scale_k y and J = sim on the valid pixels (mask
// byte set, or no mask), 0 elsewhere and outside the image, and v the validity as 0 / 1:
//   S(a)  = the separable 11-tap Gaussian window (sigma 1.5, taps normalised to sum 1) with zero padding: along x first,
//           acc = 0; acc = acc + g[t] * a[x + t - 5] for t = 0 .. 10, then the same along y over the rows of acc;
//   Wt = S(v),  muI = S(I) / Wt,  muJ = S(J) / Wt,  sI = S(I I) / Wt - muI^2,  sJ = S(J J) / Wt - muJ^2,  sIJ = S(I J) / Wt - muI muJ,
//   ssim = (2 muI muJ + C1) (2 sIJ + C2) / ((muI^2 + muJ^2 + C1) (sI + sJ + C2))       at valid pixels, exactly 0 elsewhere.
// The window is renormalised by the mask's share of it (Wt >= g[5]^2 > 0 at a valid pixel).  Eight sums per slice over its valid
// pixels follow:  { n, sum ssim, #(ssim < threshold), sum I, sum J, sum I^2, sum J^2, sum I J }.
//
// Composed from torch operators one round is about 40 launches (six separable filters, twenty elementwise, eight reductions);
// here it is one pass that reads sim, y and the mask (9 bytes per pixel) and writes the map (4 bytes), and a small reduce launch.
//
// Layout.  A 256-thread workgroup owns a 16 x 16 tile of one slice; the window's passes and their LDS layout are window.h's
// (24960 bytes, and 256 for the sums).
//
// The per-pixel arithmetic is that of the torch expression in fp32, operation for operation (the build has -ffp-contract=off; the
// divisions are correctly rounded); the taps are the host's doubles rounded to fp32, as gaussian_taps(torch.float32) gives them.
// scale_k is read from device memory.  The eight sums are added in the reproducible order of slice_sums.h, a workgroup being a
// tile.  The two counts are summed in fp32 inside a wave (at most 64 ones: exact); the six float sums are summed in double from
// the first add (wave_sum_f64): an fp32 wave sum, as robust.hip has it, missed the bound the kernel is held to ("twice the fp32
// expression's error plus one fp32 ulp of the largest sum") on the 17 valid pixels of a 5 x 5 slice, where one ulp of the sum
// is all the expression with its fp64 sums leaves.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "slice_sums.h"
#include "window.h"
#include "../../include/nesvor_hip.h"

namespace {

using window::kHaloPitch;
using window::kRadius;
using window::kTile;

constexpr int kStats = 8;

// grid: n * tiles workgroups, tiles = tiles_y * tiles_x per slice.  partial: (n, tiles, 8) doubles.
__global__ __launch_bounds__(256) void structural_ssim_kernel(const float* __restrict__ sim, const float* __restrict__ y,
                                                              const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                                              int h, int w, int tiles_x, int tiles, window::Taps taps, float c1,
                                                              float c2, float threshold, float* __restrict__ ssim,
                                                              double* __restrict__ partial) {
  __shared__ window::Lds lds;
  __shared__ double red[4][kStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int in = blockIdx.x / tiles, tile = blockIdx.x - in * tiles;
  const int tile_y = tile / tiles_x;
  const int y0 = tile_y * kTile, x0 = (tile - tile_y * tiles_x) * kTile;
  const size_t base = (size_t)in * h * w;  // the host checked h w <= INT_MAX - 256
  const float s = scale[in];               // workgroup-uniform: the scalar path

  // the halo: I = scale_k y, J = sim on the mask
  window::stage_halo(lds, y0, x0, h, w, [&](int gy, int gx, float& iv, float& jv) {
    const size_t idx = base + (size_t)gy * w + gx;
    if (mask != nullptr && !mask[idx]) return false;
    iv = s * y[idx];
    jv = sim[idx];
    return true;
  });
  __syncthreads();
  window::row_pass(lds, taps);
  __syncthreads();

  // along y, and the SSIM arithmetic of this thread's pixel
  const int ty = tid >> 4, tx = tid & 15;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < h && gx < w;
  const int centre = (ty + kRadius) * kHaloPitch + tx + kRadius;
  const float iv = lds.halo[0][centre], jv = lds.halo[1][centre];
  const bool on = lds.halo[2][centre] != 0.f;  // (false outside the image)
  float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  window::column_pass(lds, taps, ty, tx, m);
  const float value = on ? window::ssim_value(m, c1, c2) : 0.f;
  if (inside) ssim[base + (size_t)gy * w + gx] = value;

  // (the products are the expression's fp32 ones; off the mask iv = jv = value = 0)
  const double s0 = (double)wave_sum_dpp(on ? 1.f : 0.f), s2 = (double)wave_sum_dpp(on && value < threshold ? 1.f : 0.f);
  const double s1 = wave_sum_f64(value), s3 = wave_sum_f64(iv), s4 = wave_sum_f64(jv), s5 = wave_sum_f64(iv * iv),
               s6 = wave_sum_f64(jv * jv), s7 = wave_sum_f64(iv * jv);
  // Step 2 of slice_sums.h, written out: through slice_sums::store_workgroup_sums (or any other spelling tried) the compiler's
  // SLP vectoriser repacks the window's tap loops into v_pk_add_f32 / v_pk_mul_f32 - the same values, but the kernel then measured
  // 1 to 4 % slower on 128 x 128 slices in five of five alternating runs.
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3;
    red[wave][4] = s4; red[wave][5] = s5; red[wave][6] = s6; red[wave][7] = s7;
  }
  __syncthreads();
  if (tid < kStats) partial[((size_t)in * tiles + tile) * kStats + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

bool usable(float v) { return v >= 0.f && v <= FLT_MAX; }  // false for a negative, an infinity and a NaN

}  // namespace

extern "C" int64_t nesvor_structural_ssim_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kStats>{n, slice_sums::tile_workgroups(h, w)}.workspace_bytes();
}

extern "C" int nesvor_structural_ssim(const float* sim, const float* y, const uint8_t* mask, const float* scale, int n, int h, int w,
                                      float c1, float c2, float threshold, float* ssim, double* stats, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (sim == nullptr || y == nullptr || scale == nullptr || ssim == nullptr || stats == nullptr) return (int)hipErrorInvalidValue;
  if (!usable(c1) || !usable(c2) || !usable(threshold)) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kStats> plan{n, slice_sums::tile_workgroups(h, w)};  // a workgroup per tile
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  window::Taps taps;
  window::gaussian_taps(1.5, kRadius, taps.g);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(structural_ssim_kernel, dim3((unsigned)(plan.wgs * n)), dim3(256), 0, st, sim, y, mask, scale, h, w,
                     (int)((w + kTile - 1) / kTile), (int)plan.wgs, taps, c1, c2, threshold, ssim, (double*)workspace);
  plan.reduce(workspace, stats, st);
  return (int)hipGetLastError();
}
