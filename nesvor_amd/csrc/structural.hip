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
// Layout.  A 256-thread workgroup owns a 16 x 16 tile of one slice: thread t is pixel (t / 16, t % 16), so a 32-lane half of a
// wave - the group whose ds_read_b32 / ds_write_b32 addresses share 32 banks - is two tile rows.
//   halo  3 x 26 x 48 floats  I, J, v on the tile and 5 pixels around it.  Staged as 8 rows x 32 columns per sweep (26 live):
//         a half-wave writes one row, consecutive banks.  The horizontal pass's half-wave reads columns c + t, c = 0 .. 15, of
//         rows r and r + 1: with the row pitch = 16 mod 32 the two runs of 16 never share a bank (the pitch 26 would put them
//         26 banks apart: 6 two-way conflicts on every read).  48 is the smallest such pitch >= 26.
//   mom   6 x 26 x 16 floats  S_h(v, I, J, I I, J J, I J).  Pitch 16: rows r and r + 1 are 32 consecutive floats, so the horizontal
//         pass's writes and the vertical pass's reads (rows ty + t, ty + 1 + t) are conflict-free.
// 14976 + 9984 + 256 bytes of LDS: six workgroups per CU before LDS limits occupancy.  Two barriers.
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
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kStats = 8;
constexpr int kTile = 16;                      // the tile's edge: 256 threads
constexpr int kRadius = 5, kTaps = 2 * kRadius + 1;
constexpr int kHalo = kTile + 2 * kRadius;     // 26
constexpr int kHaloPitch = 48;                 // = 16 mod 32, >= kHalo
constexpr int kRows = kHalo * kTile;           // 416 horizontally filtered values per moment

struct Taps { float g[kTaps]; };

// grid: n * tiles workgroups, tiles = tiles_y * tiles_x per slice.  partial: (n, tiles, 8) doubles.
__global__ __launch_bounds__(256) void structural_ssim_kernel(const float* __restrict__ sim, const float* __restrict__ y,
                                                              const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                                              int h, int w, int tiles_x, int tiles, Taps taps, float c1, float c2,
                                                              float threshold, float* __restrict__ ssim, double* __restrict__ partial) {
  __shared__ float halo[3][kHalo * kHaloPitch];
  __shared__ float mom[6][kRows];
  __shared__ double red[4][kStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int in = blockIdx.x / tiles, tile = blockIdx.x - in * tiles;
  const int tile_y = tile / tiles_x;
  const int y0 = tile_y * kTile, x0 = (tile - tile_y * tiles_x) * kTile;
  const size_t base = (size_t)in * h * w;  // the host checked h w <= INT_MAX - 256
  const float s = scale[in];               // workgroup-uniform: the scalar path

  // the halo: I, J, v; 0 off the mask and outside the image (the window's zero padding)
  {
    const int c = tid & 31;
    if (c < kHalo) {
      const int gx = x0 + c - kRadius;
      for (int r = tid >> 5; r < kHalo; r += 8) {
        const int gy = y0 + r - kRadius;
        float iv = 0.f, jv = 0.f, vv = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
          const size_t idx = base + (size_t)gy * w + gx;
          if (mask == nullptr || mask[idx]) {
            iv = s * y[idx];
            jv = sim[idx];
            vv = 1.f;
          }
        }
        halo[0][r * kHaloPitch + c] = iv;
        halo[1][r * kHaloPitch + c] = jv;
        halo[2][r * kHaloPitch + c] = vv;
      }
    }
  }
  __syncthreads();

  // along x: the six moments of the 26 rows on the tile's 16 columns
  for (int i = tid; i < kRows; i += 256) {
    const int o = (i >> 4) * kHaloPitch + (i & 15);
    float av = 0.f, ai = 0.f, aj = 0.f, aii = 0.f, ajj = 0.f, aij = 0.f;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
      const float g = taps.g[t], iv = halo[0][o + t], jv = halo[1][o + t], vv = halo[2][o + t];
      av = av + g * vv;
      ai = ai + g * iv;
      aj = aj + g * jv;
      aii = aii + g * (iv * iv);
      ajj = ajj + g * (jv * jv);
      aij = aij + g * (iv * jv);
    }
    mom[0][i] = av; mom[1][i] = ai; mom[2][i] = aj; mom[3][i] = aii; mom[4][i] = ajj; mom[5][i] = aij;
  }
  __syncthreads();

  // along y, and the SSIM arithmetic of this thread's pixel
  const int ty = tid >> 4, tx = tid & 15;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < h && gx < w;
  const float iv = halo[0][(ty + kRadius) * kHaloPitch + tx + kRadius], jv = halo[1][(ty + kRadius) * kHaloPitch + tx + kRadius];
  const bool on = halo[2][(ty + kRadius) * kHaloPitch + tx + kRadius] != 0.f;  // (false outside the image)
  float sv = 0.f, si = 0.f, sj = 0.f, sii = 0.f, sjj = 0.f, sij = 0.f;
#pragma unroll
  for (int t = 0; t < kTaps; ++t) {
    const float g = taps.g[t];
    const int o = (ty + t) * kTile + tx;
    sv = sv + g * mom[0][o];
    si = si + g * mom[1][o];
    sj = sj + g * mom[2][o];
    sii = sii + g * mom[3][o];
    sjj = sjj + g * mom[4][o];
    sij = sij + g * mom[5][o];
  }
  float value = 0.f;
  if (on) {
    const float mu_i = si / sv, mu_j = sj / sv;
    const float var_i = sii / sv - mu_i * mu_i, var_j = sjj / sv - mu_j * mu_j, cov = sij / sv - mu_i * mu_j;
    const float num = (2.f * mu_i * mu_j + c1) * (2.f * cov + c2);
    const float den = (mu_i * mu_i + mu_j * mu_j + c1) * (var_i + var_j + c2);
    value = num / den;
  }
  if (inside) ssim[base + (size_t)gy * w + gx] = value;

  // (the products are the expression's fp32 ones; off the mask iv = jv = value = 0)
  const double s0 = (double)wave_sum_dpp(on ? 1.f : 0.f), s2 = (double)wave_sum_dpp(on && value < threshold ? 1.f : 0.f);
  const double s1 = wave_sum_f64(value), s3 = wave_sum_f64(iv), s4 = wave_sum_f64(jv), s5 = wave_sum_f64(iv * iv),
               s6 = wave_sum_f64(jv * jv), s7 = wave_sum_f64(iv * jv);
  // Step 2 of slice_sums.h, written out: through slice_sums::store_workgroup_sums (or any other spelling tried) the compiler's
  // SLP vectoriser repacks the tap loops above into v_pk_add_f32 / v_pk_mul_f32 - the same values, but the kernel then measured
  // 1 to 4 % slower on 128 x 128 slices in five of five alternating runs.
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3;
    red[wave][4] = s4; red[wave][5] = s5; red[wave][6] = s6; red[wave][7] = s7;
  }
  __syncthreads();
  if (tid < kStats) partial[((size_t)in * tiles + tile) * kStats + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

int64_t tiles_of(int h, int w) { return (((int64_t)h + kTile - 1) / kTile) * (((int64_t)w + kTile - 1) / kTile); }

bool usable(float v) { return v >= 0.f && v <= FLT_MAX; }  // false for a negative, an infinity and a NaN

}  // namespace

extern "C" int64_t nesvor_structural_ssim_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kStats>{n, tiles_of(h, w)}.workspace_bytes();
}

extern "C" int nesvor_structural_ssim(const float* sim, const float* y, const uint8_t* mask, const float* scale, int n, int h, int w,
                                      float c1, float c2, float threshold, float* ssim, double* stats, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (sim == nullptr || y == nullptr || scale == nullptr || ssim == nullptr || stats == nullptr) return (int)hipErrorInvalidValue;
  if (!usable(c1) || !usable(c2) || !usable(threshold)) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kStats> plan{n, tiles_of(h, w)};  // a workgroup per tile
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  // g[t] = exp(-(t - 5)^2 / (2 1.5^2)) normalised to sum 1, in double, rounded to fp32 once
  Taps taps;
  double g[kTaps], sum = 0.0;
  for (int t = 0; t < kTaps; ++t) {
    g[t] = exp(-(double)((t - kRadius) * (t - kRadius)) / (2.0 * 1.5 * 1.5));
    sum += g[t];
  }
  for (int t = 0; t < kTaps; ++t) taps.g[t] = (float)(g[t] / sum);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(structural_ssim_kernel, dim3((unsigned)(plan.wgs * n)), dim3(256), 0, st, sim, y, mask, scale, h, w,
                     (int)((w + kTile - 1) / kTile), (int)plan.wgs, taps, c1, c2, threshold, ssim, (double*)workspace);
  plan.reduce(workspace, stats, st);
  return (int)hipGetLastError();
}
