// Bias field correction (N4-style, nesvor_amd/bias.py) on gfx950: the three per-iteration passes over a stack's voxels.
//
// One iteration of the correction sharpens the histogram of u = v - f (v = log intensity, f = the log field so far), fits the
// residual r = u - E[u] with a cubic B-spline lattice of C = S + 3 control points per axis (the multilevel B-spline approximation
// of Lee, Wolberg and Shin) and adds the fitted field to f.  Composed from torch operators that is a masked gather, two
// index_adds, eight einsums with dense (n, C) weight tables and a dozen voxel-sized temporaries per iteration, 50 to 200 times
// per stack; here
//   nesvor_n4_histogram  one pass: the fractionally binned histogram of u,
//   nesvor_n4_fit        one pass that forms r from the sharpened histogram's lookup table on the fly and contracts the x axis
//                        per (z, y) row, then two small launches that contract y and z: the lattice and its divisor,
//   nesvor_n4_update     one pass: f += the lattice's field (the lattice collapsed over z and y per row first: four taps per
//                        voxel) and the five statistics the stop test and the next iteration's histogram range need.
//
// Arithmetic.  u, the bin coordinate c and the residual are computed in double per voxel (gfx950 runs fp64 at the fp32 rate), so
// they are the composed fp64 path's values.  The per-axis tables arrive as fp32 (span index and four basis values per voxel
// index).  Sums: fp32 only inside one wave's DPP reduction (64 terms, nesvor_pair_moments' rule), double beyond; every row /
// workgroup stores its partials to the workspace and small follow-up launches add them in a fixed order.  No floating-point
// atomics, no memset: bit-identical results from run to run.
//
// The histogram alone uses INTEGER atomics, in LDS, on fixed-point weights with the quantum 2^-32: a voxel adds
// w1 = round(frac * 2^32) to bin i + 1 and 2^32 - w1 to bin i (so every voxel adds exactly 2^32 and the total is the exact
// count); integer addition is associative, so the order the atomics retire in does not matter.  Each workgroup stores its
// 64-bit bins to the workspace, a second launch adds them and scales by 2^-32.  A bin differs from the fp64 expression by at
// most 2^-33 per voxel that touches it.
//
// Memory safety does not depend on the inputs' values: c is clamped to [0, n_bins - 1] (NaN -> 0), span indices to [0, S - 1].
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kMaxC = 16;        // control points per axis
constexpr int kStats = 5;        // {count, sum g, sum g^2, min u, max u}
constexpr double kFixedOne = 4294967296.0;  // 2^32: one voxel in the histogram's fixed-point weights

// u = v - f and its bin coordinate c = (u - lo) / slope clamped to [0, n_bins - 1]; fmax / fmin drop a NaN (slope 0): c = 0
__device__ __forceinline__ double bin_coord(double u, double lo, double slope, int n_bins) {
  return fmin(fmax((u - lo) / slope, 0.0), (double)(n_bins - 1));
}

__device__ __forceinline__ int clamp_span(int s, int S) { return min(max(s, 0), S - 1); }

// ---------------------------------------------------------------------------------------------------------------------
// histogram.  grid: G <= kHistWgs workgroups striding over the voxels; partial: (G, n_bins) 64-bit fixed-point bins
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_histogram_kernel(const float* __restrict__ v, const float* __restrict__ f,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ range, int N,
                                                           int n_bins, unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long bins[kMaxBins];
  for (int i = threadIdx.x; i < n_bins; i += 256) bins[i] = 0ull;
  __syncthreads();
  const double lo = (double)range[0], slope = ((double)range[1] - lo) / (double)(n_bins - 1);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += stride) {
    if (mask != nullptr && !mask[p]) continue;
    const double c = bin_coord((double)v[p] - (double)f[p], lo, slope, n_bins);
    const int i = min((int)c, n_bins - 2);  // c >= 0: truncation is floor
    const unsigned long long w1 = (unsigned long long)__double2ll_rn((c - (double)i) * kFixedOne);  // in [0, 2^32]
    const unsigned long long w0 = 4294967296ull - w1;
    if (w0) atomicAdd(&bins[i], w0);
    if (w1) atomicAdd(&bins[i + 1], w1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_bins; i += 256) partial[(size_t)blockIdx.x * n_bins + i] = bins[i];
}

__global__ __launch_bounds__(256) void n4_histogram_reduce_kernel(const unsigned long long* __restrict__ partial, int G, int n_bins,
                                                                  double* __restrict__ hist) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_bins) return;
  unsigned long long s = 0ull;  // at most (INT_MAX - 256) * 2^32 < 2^63
  for (int g = 0; g < G; ++g) s += partial[(size_t)g * n_bins + b];
  hist[b] = (double)s * (1.0 / kFixedOne);
}

// ---------------------------------------------------------------------------------------------------------------------
// fit.  x: one wave per (z, y) row, px (rows, C, 2) = {sum_x r wx^3 / s2x, sum_x wx^2} over the row's valid voxels
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_fit_x_kernel(const float* __restrict__ v, const float* __restrict__ f,
                                                       const uint8_t* __restrict__ mask, const float* __restrict__ range,
                                                       const double* __restrict__ lut, int n_bins, const float* __restrict__ tx,
                                                       const int32_t* __restrict__ sx, int rows, int W, int S,
                                                       double* __restrict__ px) {
  __shared__ double slut[kMaxBins];
  for (int i = threadIdx.x; i < n_bins; i += 256) slut[i] = lut[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = S + 3;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;  // whole waves, after the only barrier
  const double lo = (double)range[0], slope = ((double)range[1] - lo) / (double)(n_bins - 1);
  double acc_n = 0.0, acc_d = 0.0;  // lane c holds control point c of the row
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + lane;
    const bool in = x < W;
    const size_t idx = (size_t)row * W + (in ? x : 0);
    const bool on = in && (mask == nullptr || mask[idx]);
    int s = 0;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, rn = 0.f;
    if (in) {
      s = clamp_span(sx[x], S);
      b0 = tx[4 * (size_t)x]; b1 = tx[4 * (size_t)x + 1]; b2 = tx[4 * (size_t)x + 2]; b3 = tx[4 * (size_t)x + 3];
    }
    if (on) {
      const double u = (double)v[idx] - (double)f[idx];
      const double c = bin_coord(u, lo, slope, n_bins);
      const int j = min((int)c, n_bins - 2);
      const double t = c - (double)j;
      const double r = u - (slut[j] * (1.0 - t) + slut[j + 1] * t);
      const double s2 = (double)b0 * b0 + (double)b1 * b1 + (double)b2 * b2 + (double)b3 * b3;
      rn = (float)(r / s2);
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      if (c < C) {  // wave-uniform
        const int k = c - s;
        const float w = k == 0 ? b0 : k == 1 ? b1 : k == 2 ? b2 : k == 3 ? b3 : 0.f;  // 0 outside the row (b = 0)
        const float sn = wave_sum_dpp(rn * (w * w * w)), sd = wave_sum_dpp(on ? w * w : 0.f);
        if (lane == c) {
          acc_n += (double)sn;
          acc_d += (double)sd;
        }
      }
    }
  }
  if (lane < C) {
    px[((size_t)row * C + lane) * 2] = acc_n;
    px[((size_t)row * C + lane) * 2 + 1] = acc_d;
  }
}

// y: py (D, C, C, 2)[z][b][c] = sum_y px[z][y][c] * {wy^3 / s2y, wy^2}, y ascending
__global__ __launch_bounds__(256) void n4_fit_y_kernel(const double* __restrict__ px, const float* __restrict__ ty,
                                                       const int32_t* __restrict__ sy, int64_t total, int H, int S,
                                                       double* __restrict__ py) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int C = S + 3;
  const int c = (int)(id % C), b = (int)((id / C) % C);
  const int64_t z = id / ((int64_t)C * C);
  double num = 0.0, den = 0.0;
  for (int y = 0; y < H; ++y) {
    const int k = b - clamp_span(sy[y], S);
    if (k < 0 || k > 3) continue;
    const float* t = ty + 4 * (size_t)y;
    const double w = (double)t[k];
    const double s2 = (double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2] + (double)t[3] * t[3];
    const double* p = px + (((size_t)z * H + y) * C + c) * 2;
    num += p[0] * (w * w * w / s2);
    den += p[1] * (w * w);
  }
  py[id * 2] = num;
  py[id * 2 + 1] = den;
}

// z: lattice[a][b][c] = num / den (0 where den is 0), weight = den, z ascending
__global__ __launch_bounds__(256) void n4_fit_z_kernel(const double* __restrict__ py, const float* __restrict__ tz,
                                                       const int32_t* __restrict__ sz, int D, int S, double* __restrict__ lattice,
                                                       double* __restrict__ weight) {
  const int C = S + 3;
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= C * C * C) return;
  const int a = id / (C * C), bc = id - a * C * C;
  double num = 0.0, den = 0.0;
  for (int z = 0; z < D; ++z) {
    const int k = a - clamp_span(sz[z], S);
    if (k < 0 || k > 3) continue;
    const float* t = tz + 4 * (size_t)z;
    const double w = (double)t[k];
    const double s2 = (double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2] + (double)t[3] * t[3];
    const double* p = py + ((size_t)z * C * C + bc) * 2;
    num += p[0] * (w * w * w / s2);
    den += p[1] * (w * w);
  }
  lattice[id] = den > 0.0 ? num / den : 0.0;
  weight[id] = den;
}

// ---------------------------------------------------------------------------------------------------------------------
// update.  one wave per (z, y) row; partial (G, 5) per workgroup of four rows
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_update_kernel(const double* __restrict__ lattice, const float* __restrict__ tz,
                                                        const float* __restrict__ ty, const float* __restrict__ tx,
                                                        const int32_t* __restrict__ sz, const int32_t* __restrict__ sy,
                                                        const int32_t* __restrict__ sx, int S, float* __restrict__ f,
                                                        const float* __restrict__ v, const uint8_t* __restrict__ mask, int rows, int H,
                                                        int W, double* __restrict__ partial) {
  __shared__ double lrow[4][kMaxC];
  __shared__ double red[4][kStats];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = S + 3;
  const int row = blockIdx.x * 4 + wave;
  const bool active = row < rows;  // wave-uniform
  if (active && lane < C) {
    // the lattice collapsed over z and y for this row: lrow[c] = sum_{a,b} lattice[sz+a][sy+b][c] bz[a] by[b]
    const int z = row / H, y = row - z * H;
    const int z0 = clamp_span(sz[z], S), y0 = clamp_span(sy[y], S);
    double acc = 0.0;
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b)
        acc += lattice[((size_t)(z0 + a) * C + (y0 + b)) * C + lane] * ((double)tz[4 * (size_t)z + a] * (double)ty[4 * (size_t)y + b]);
    lrow[wave][lane] = acc;
  }
  __syncthreads();
  double cnt = 0.0, sg = 0.0, sgg = 0.0, umin = INFINITY, umax = -INFINITY;
  if (active) {
    for (int x0 = 0; x0 < W; x0 += 64) {
      const int x = x0 + lane;
      const bool in = x < W;
      const size_t idx = (size_t)row * W + (in ? x : 0);
      const bool on = in && (mask == nullptr || mask[idx]);
      float g = 0.f;
      if (in) {
        const int s = clamp_span(sx[x], S);
        const float* t = tx + 4 * (size_t)x;
        const double df = (lrow[wave][s] * (double)t[0] + lrow[wave][s + 1] * (double)t[1]) +
                          (lrow[wave][s + 2] * (double)t[2] + lrow[wave][s + 3] * (double)t[3]);
        const float fn = (float)((double)f[idx] + df);
        f[idx] = fn;
        if (on) {
          g = (float)expm1(df);
          const double un = (double)v[idx] - (double)fn;
          umin = fmin(umin, un);
          umax = fmax(umax, un);
        }
      }
      cnt += (double)wave_sum_dpp(on ? 1.f : 0.f);
      sg += (double)wave_sum_dpp(g);
      sgg += (double)wave_sum_dpp(g * g);
    }
    umin = wave_min_f64(umin);
    umax = wave_max_f64(umax);
  }
  if (lane == 0) {
    red[wave][0] = cnt; red[wave][1] = sg; red[wave][2] = sgg; red[wave][3] = umin; red[wave][4] = umax;
  }
  __syncthreads();
  if (threadIdx.x < kStats) {
    const int j = threadIdx.x;
    double t;
    if (j < 3) t = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    else if (j == 3) t = fmin(fmin(red[0][j], red[1][j]), fmin(red[2][j], red[3][j]));
    else t = fmax(fmax(red[0][j], red[1][j]), fmax(red[2][j], red[3][j]));
    partial[(size_t)blockIdx.x * kStats + j] = t;
  }
}

// stats = the G partials combined in workgroup order: thread t takes a contiguous run of them, thread j < 5 then the 256 runs
__global__ __launch_bounds__(256) void n4_update_reduce_kernel(const double* __restrict__ partial, int G, double* __restrict__ stats) {
  __shared__ double runs[256][kStats];
  const int per = (G + 255) / 256;
  const int g0 = min((int)threadIdx.x * per, G), g1 = min(g0 + per, G);
  double a[kStats] = {0.0, 0.0, 0.0, INFINITY, -INFINITY};
  for (int g = g0; g < g1; ++g) {
    const double* p = partial + (size_t)g * kStats;
    a[0] += p[0]; a[1] += p[1]; a[2] += p[2];
    a[3] = fmin(a[3], p[3]); a[4] = fmax(a[4], p[4]);
  }
  for (int j = 0; j < kStats; ++j) runs[threadIdx.x][j] = a[j];
  __syncthreads();
  if (threadIdx.x < kStats) {
    const int j = threadIdx.x;
    double t = runs[0][j];
    for (int i = 1; i < 256; ++i) t = j < 3 ? t + runs[i][j] : j == 3 ? fmin(t, runs[i][j]) : fmax(t, runs[i][j]);
    stats[j] = t;
  }
}

}  // namespace

extern "C" int64_t nesvor_n4_histogram_workspace_bytes(int D, int H, int W, int n_bins) {
  if (bad_volume(D, H, W) || n_bins < 2 || n_bins > kMaxBins) return 0;
  return (int64_t)sizeof(unsigned long long) * n_bins * hist_wgs((int64_t)D * H * W);
}

extern "C" int nesvor_n4_histogram(const float* v, const float* f, const uint8_t* mask, int D, int H, int W, const float* range,
                                   int n_bins, double* hist, void* workspace, size_t workspace_bytes, void* stream) {
  if (v == nullptr || f == nullptr || range == nullptr || hist == nullptr) return (int)hipErrorInvalidValue;
  if (bad_volume(D, H, W) || n_bins < 2 || n_bins > kMaxBins) return (int)hipErrorInvalidValue;
  const int64_t need = nesvor_n4_histogram_workspace_bytes(D, H, W, n_bins);
  if (workspace == nullptr || (int64_t)workspace_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int N = D * H * W, G = hist_wgs(N);
  unsigned long long* partial = (unsigned long long*)workspace;
  hipLaunchKernelGGL(n4_histogram_kernel, dim3((unsigned)G), dim3(256), 0, st, v, f, mask, range, N, n_bins, partial);
  hipLaunchKernelGGL(n4_histogram_reduce_kernel, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, st,
                     (const unsigned long long*)partial, G, n_bins, hist);
  return (int)hipGetLastError();
}

extern "C" int64_t nesvor_n4_fit_workspace_bytes(int D, int H, int W, int S) {
  if (bad_volume(D, H, W) || S < 1 || S + 3 > kMaxC) return 0;
  const int64_t C = S + 3;
  return (int64_t)sizeof(double) * 2 * C * ((int64_t)D * H + (int64_t)D * C);  // px (D H, C, 2) then py (D, C, C, 2)
}

extern "C" int nesvor_n4_fit(const float* v, const float* f, const uint8_t* mask, const float* range, const double* lut, int n_bins,
                             const float* tz, const float* ty, const float* tx, const int32_t* sz, const int32_t* sy,
                             const int32_t* sx, int D, int H, int W, int S, double* lattice, double* weight, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (v == nullptr || f == nullptr || range == nullptr || lut == nullptr || tz == nullptr || ty == nullptr || tx == nullptr ||
      sz == nullptr || sy == nullptr || sx == nullptr || lattice == nullptr || weight == nullptr)
    return (int)hipErrorInvalidValue;
  if (bad_volume(D, H, W) || S < 1 || S + 3 > kMaxC || n_bins < 2 || n_bins > kMaxBins) return (int)hipErrorInvalidValue;
  const int64_t need = nesvor_n4_fit_workspace_bytes(D, H, W, S);
  if (workspace == nullptr || (int64_t)workspace_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int C = S + 3, rows = D * H;
  double* px = (double*)workspace;
  double* py = px + (size_t)rows * C * 2;
  hipLaunchKernelGGL(n4_fit_x_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, v, f, mask, range, lut, n_bins, tx, sx, rows,
                     W, S, px);
  const int64_t total = (int64_t)D * C * C;
  hipLaunchKernelGGL(n4_fit_y_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)px, ty, sy, total, H, S,
                     py);
  hipLaunchKernelGGL(n4_fit_z_kernel, dim3((unsigned)((C * C * C + 255) / 256)), dim3(256), 0, st, (const double*)py, tz, sz, D, S,
                     lattice, weight);
  return (int)hipGetLastError();
}

extern "C" int64_t nesvor_n4_update_workspace_bytes(int D, int H, int W) {
  if (bad_volume(D, H, W)) return 0;
  return (int64_t)sizeof(double) * kStats * (((int64_t)D * H + 3) / 4);
}

extern "C" int nesvor_n4_update(const double* lattice, const float* tz, const float* ty, const float* tx, const int32_t* sz,
                                const int32_t* sy, const int32_t* sx, int S, float* f, const float* v, const uint8_t* mask, int D,
                                int H, int W, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (lattice == nullptr || tz == nullptr || ty == nullptr || tx == nullptr || sz == nullptr || sy == nullptr || sx == nullptr ||
      f == nullptr || v == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  if (bad_volume(D, H, W) || S < 1 || S + 3 > kMaxC) return (int)hipErrorInvalidValue;
  const int64_t need = nesvor_n4_update_workspace_bytes(D, H, W);
  if (workspace == nullptr || (int64_t)workspace_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int rows = D * H, G = (rows + 3) / 4;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(n4_update_kernel, dim3((unsigned)G), dim3(256), 0, st, lattice, tz, ty, tx, sz, sy, sx, S, f, v, mask, rows, H, W,
                     partial);
  hipLaunchKernelGGL(n4_update_reduce_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, G, stats);
  return (int)hipGetLastError();
}
