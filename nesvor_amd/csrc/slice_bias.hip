// Slice bias fields of the classical reconstruction (gfx950): one round of the smooth multiplicative field per slice, estimated
// from the log-ratio of the slice to its simulation, in two passes.
//
// Definition (nesvor_amd/slice_bias.py::field_composed).  For slice k with sim = A x, y the acquired slice, b the current
// log-field, w the pixel weight (1 without one) and lo the intensity floor:
//   e = valid & (y > lo) & (sim > lo)                                      the eligible pixels (valid: mask byte set, or no mask)
//   I = (scale_k y) exp(-b),   r = clamp(log(I / sim), -log 2, log 2),   u = w      on eligible pixels; r = u = 0 elsewhere
//   S(a) = the separable Gaussian window of radius R (2 R + 1 taps normalised to sum 1) with zero padding: along x first,
//          acc = 0; acc = acc + g[t] * a[x + t - R] for t = 0 .. 2 R, then the same along y over the rows of acc;
//   num = S(u r),  den = S(u),  d = num / den where den > 1e-3, else 0,   b_new = b + d                on every pixel.
// Five sums per slice follow:  { #e, sum u, sum u b_new, sum u r, sum (u r) r }  (u = 0 off the eligible pixels).
//
// Composed from torch operators one round is 4 (2 R + 1) shifted-slice multiply-adds over slice-sized temporaries (196 launches
// at R = 24), a dozen elementwise launches and five reductions.  Here it is two passes and a small reduce launch; the slices
// and the two intermediates live in L2, so what is saved is launches and temporaries, not bandwidth.
//
// Row pass.  A 256-thread workgroup owns `rows` rows of a `seg`-pixel row segment, seg = the power of two >= w in 16 .. 256
// (256 for wider slices, which take several segments) and rows = 256 / seg: a 59-pixel row keeps 59 of 64 threads busy instead
// of 59 of 256.  u r and u of the segment and R pixels either side go to LDS, every row with the pitch seg + 2 R; thread
// (row, x) then reads x + t, t = 0 .. 2 R: a 32-lane half of a wave - the group whose ds_read_b32 addresses share 32 banks -
// reads 32 consecutive floats for seg >= 32.  For seg = 16 the half is two rows, and the pitch is raised to the next value
// = 16 mod 32, so that the two runs of 16 never share a bank.  S_x(u r) and S_x(u) are written to the workspace.
// Column pass.  A workgroup owns a 16 x 16 tile (thread t is pixel (t / 16, t % 16), as in structural.hip): the two
// intermediates on the tile's columns and R rows above and below go to LDS with the pitch 16 (rows r and r + 1 are 32
// consecutive floats: conflict-free), the taps are added along y, the division and b_new follow.  The thread then evaluates
// e, r and u of its own pixel again (the same operations on the same inputs: the same values) for the sums.
// 14336 bytes of LDS in either kernel.
//
// The per-pixel arithmetic is that of the torch expression in fp32, operation for operation (the build has -ffp-contract=off;
// the divisions are correctly rounded, expf and logf are the library's, the ones torch's fp32 exp and log call); the taps are the
// host's doubles rounded to fp32, as slice_bias.gaussian_taps(sigma_px, torch.float32) gives them.  The sums are added in the
// reproducible order of slice_sums.h, a workgroup being a tile; the count in fp32 inside a wave (at most 64 ones: exact), the
// four float sums in double from the first add (wave_sum_f64), for the reason structural.hip gives: on a slice of a few dozen
// pixels one fp32 ulp of the sum is all the bound ("twice the fp32 expression's error plus one ulp") leaves.
// Memory safety does not depend on a value: every index is a function of n, h, w and R, which the host checks.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "slice_sums.h"
#include "window.h"  // (gaussian_taps alone)
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kStats = 5;
constexpr int kMaxRadius = 48, kMaxTaps = 2 * kMaxRadius + 1;
constexpr int kTile = 16;                                // the column pass's tile edge: 256 threads
constexpr int kColRows = kTile + 2 * kMaxRadius;         // 112 rows of 16
constexpr int kRowFloats = 16 * (16 + 2 * kMaxRadius);   // the row pass's largest stage: 16 rows of pitch 112 (seg = 16)
constexpr float kClamp = 0.693147180559945309417f;       // log 2
constexpr float kDenMin = 1e-3f;

struct Taps { float g[kMaxTaps]; };

// u r and u of one pixel; both 0 where it is not eligible.  `idx` is inside the arrays.
__device__ __forceinline__ bool pixel_terms(const float* __restrict__ sim, const float* __restrict__ y, const uint8_t* __restrict__ mask,
                                            const float* __restrict__ weight, const float* __restrict__ b, size_t idx, float s, float lo,
                                            float& r, float& u) {
  r = 0.f;
  u = 0.f;
  if (mask != nullptr && !mask[idx]) return false;
  const float yv = y[idx], sv = sim[idx];
  if (!(yv > lo && sv > lo)) return false;
  const float iv = (s * yv) * expf(-b[idx]);
  r = fminf(fmaxf(logf(iv / sv), -kClamp), kClamp);
  u = weight == nullptr ? 1.f : weight[idx];
  return true;
}

// grid: n * row_groups * segs workgroups.  seg = 1 << seg_log2 pixels of 256 >> seg_log2 rows each; pitch >= seg + 2 R.
__global__ __launch_bounds__(256) void slice_bias_rows_kernel(const float* __restrict__ sim, const float* __restrict__ y,
                                                              const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                                              const float* __restrict__ weight, const float* __restrict__ b, int h, int w,
                                                              int seg_log2, int segs, int row_groups, int radius, int pitch, float lo,
                                                              Taps taps, float* __restrict__ row_num, float* __restrict__ row_den) {
  __shared__ float stage[2][kRowFloats];
  const int tid = threadIdx.x;
  const int seg = 1 << seg_log2, rows = 256 >> seg_log2, span = seg + 2 * radius;
  const int per_slice = row_groups * segs;
  const int in = blockIdx.x / per_slice, rest = blockIdx.x - in * per_slice;
  const int group = rest / segs;
  const int y0 = group * rows, x0 = (rest - group * segs) * seg;
  const size_t base = (size_t)in * h * w;  // the host checked h w <= INT_MAX - 256
  const float s = scale[in];               // workgroup-uniform: the scalar path

  for (int i = tid; i < rows * span; i += 256) {
    const int lr = i / span, c = i - lr * span;
    const int gy = y0 + lr, gx = x0 + c - radius;
    float r = 0.f, u = 0.f;
    if (gy < h && gx >= 0 && gx < w) pixel_terms(sim, y, mask, weight, b, base + (size_t)gy * w + gx, s, lo, r, u);
    stage[0][lr * pitch + c] = u * r;
    stage[1][lr * pitch + c] = u;
  }
  __syncthreads();

  const int lr = tid >> seg_log2, lx = tid & (seg - 1);
  const int gy = y0 + lr, gx = x0 + lx;
  const int o = lr * pitch + lx;
  float an = 0.f, ad = 0.f;
  for (int t = 0; t <= 2 * radius; ++t) {
    const float g = taps.g[t];
    an = an + g * stage[0][o + t];
    ad = ad + g * stage[1][o + t];
  }
  if (gy < h && gx < w) {
    const size_t idx = base + (size_t)gy * w + gx;
    row_num[idx] = an;
    row_den[idx] = ad;
  }
}

// grid: n * tiles workgroups, tiles = tiles_y * tiles_x per slice.  partial: (n, tiles, 5) doubles.
__global__ __launch_bounds__(256) void slice_bias_columns_kernel(const float* __restrict__ sim, const float* __restrict__ y,
                                                                 const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                                                 const float* __restrict__ weight, const float* __restrict__ b, int h, int w,
                                                                 int tiles_x, int tiles, int radius, float lo, Taps taps,
                                                                 const float* __restrict__ row_num, const float* __restrict__ row_den,
                                                                 float* __restrict__ b_new, double* __restrict__ partial) {
  __shared__ float stage[2][kColRows * kTile];
  __shared__ double red[4][kStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int in = blockIdx.x / tiles, tile = blockIdx.x - in * tiles;
  const int tile_y = tile / tiles_x;
  const int y0 = tile_y * kTile, x0 = (tile - tile_y * tiles_x) * kTile;
  const size_t base = (size_t)in * h * w;
  const float s = scale[in];

  // the intermediates on the tile's columns and `radius` rows around it; 0 outside the image (the window's zero padding)
  for (int i = tid; i < (kTile + 2 * radius) * kTile; i += 256) {
    const int gy = y0 + (i >> 4) - radius, gx = x0 + (i & 15);
    float vn = 0.f, vd = 0.f;
    if (gy >= 0 && gy < h && gx < w) {
      const size_t idx = base + (size_t)gy * w + gx;
      vn = row_num[idx];
      vd = row_den[idx];
    }
    stage[0][i] = vn;
    stage[1][i] = vd;
  }
  __syncthreads();

  const int ty = tid >> 4, tx = tid & 15;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < h && gx < w;
  float num = 0.f, den = 0.f;
  for (int t = 0; t <= 2 * radius; ++t) {
    const float g = taps.g[t];
    const int o = (ty + t) * kTile + tx;
    num = num + g * stage[0][o];
    den = den + g * stage[1][o];
  }
  float r = 0.f, u = 0.f, ub = 0.f;
  bool on = false;
  if (inside) {
    const size_t idx = base + (size_t)gy * w + gx;
    const float d = den > kDenMin ? num / den : 0.f;
    const float bn = b[idx] + d;
    b_new[idx] = bn;
    on = pixel_terms(sim, y, mask, weight, b, idx, s, lo, r, u);
    if (on) ub = u * bn;  // (not 0 * bn: a field that has run away to infinity off the eligible pixels stays out of the sum)
  }
  const float ur = u * r;
  const double s0 = (double)wave_sum_dpp(on ? 1.f : 0.f);
  const double s1 = wave_sum_f64(u), s2 = wave_sum_f64(ub), s3 = wave_sum_f64(ur), s4 = wave_sum_f64(ur * r);
  // (step 2 of slice_sums.h written out, as structural.hip has it and says why)
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; red[wave][4] = s4;
  }
  __syncthreads();
  if (tid < kStats) partial[((size_t)in * tiles + tile) * kStats + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// the two intermediates follow the partial sums (a multiple of 8 bytes) in the workspace
int64_t intermediate_bytes(int n, int h, int w) { return 2 * (int64_t)sizeof(float) * n * h * w; }

}  // namespace

extern "C" int64_t nesvor_slice_bias_update_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1 || (int64_t)h * w > INT_MAX - 256) return 0;
  return slice_sums::Plan<kStats>{n, slice_sums::tile_workgroups(h, w)}.workspace_bytes() + intermediate_bytes(n, h, w);
}

extern "C" int nesvor_slice_bias_update(const float* sim, const float* y, const uint8_t* mask, const float* scale, const float* weight,
                                        const float* b, int n, int h, int w, double sigma_px, int radius, float min_intensity,
                                        float* b_new, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (sim == nullptr || y == nullptr || scale == nullptr || b == nullptr || b_new == nullptr || stats == nullptr || b_new == b)
    return (int)hipErrorInvalidValue;
  if (radius < 1 || radius > kMaxRadius || !(sigma_px > 0.0 && sigma_px <= DBL_MAX)) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kStats> plan{n, slice_sums::tile_workgroups(h, w)};  // the column pass: a workgroup per tile
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  if ((int64_t)workspace_bytes < plan.workspace_bytes() + intermediate_bytes(n, h, w)) return (int)hipErrorInvalidValue;
  int seg_log2 = 4;
  while (seg_log2 < 8 && (1 << seg_log2) < w) ++seg_log2;
  const int seg = 1 << seg_log2, rows = 256 >> seg_log2;
  const int64_t segs = ((int64_t)w + seg - 1) / seg, row_groups = ((int64_t)h + rows - 1) / rows;
  if (segs * row_groups * n > INT_MAX) return (int)hipErrorInvalidValue;
  // rows of one 32-lane half (seg = 16) start 16 banks apart; otherwise the pitch is the span
  const int pitch = seg == 16 ? ((2 * radius + 31) / 32) * 32 + 16 : seg + 2 * radius;
  Taps taps;
  window::gaussian_taps(sigma_px, radius, taps.g);
  float* row_num = (float*)((char*)workspace + plan.workspace_bytes());
  float* row_den = row_num + (size_t)n * h * w;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(slice_bias_rows_kernel, dim3((unsigned)(segs * row_groups * n)), dim3(256), 0, st, sim, y, mask, scale, weight, b, h,
                     w, seg_log2, (int)segs, (int)row_groups, radius, pitch, min_intensity, taps, row_num, row_den);
  hipLaunchKernelGGL(slice_bias_columns_kernel, dim3((unsigned)(plan.wgs * n)), dim3(256), 0, st, sim, y, mask, scale, weight, b, h, w,
                     (int)((w + kTile - 1) / kTile), (int)plan.wgs, radius, min_intensity, taps, row_num, row_den, b_new,
                     (double*)workspace);
  plan.reduce(workspace, stats, st);
  return (int)hipGetLastError();
}
