// Volume comparison (the ``evaluate`` command, nesvor_amd/evaluate.py) on gfx950: a volume X resampled onto the lattice of a
// reference volume R, and the 3-D SSIM map of the two with the sums of the error measures.
//
// Definition (nesvor_amd/evaluate.py::resample_composed, ssim3d_composed).
//   nesvor_volume_resample.  M (3,4) takes an R voxel index (x, y, z) to the continuous X voxel index, in double and in the
//     written order:  u_a = ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3].  With eps = 2^-20 a voxel is inside where
//     -eps <= u_a <= size_a - 1 + eps on the three axes; u is then clamped to [0, size - 1], i0 = floor(u),
//     f = (float)(u - floor(u)), i1 = min(i0 + 1, size - 1) (its weight is 0 where it was clamped).  lerp(a, b, f) = a + f (b - a)
//     in fp32, along x, then y, then z, gives J0 from X0 and mX from X's mask as 0 / 1 (1 without a mask).
//     v = maskR and inside and mX >= 0.5;  J0 = 0 off v.  stats = { n, n_ref = #maskR, sum I, sum J, sum I^2, sum J^2, sum I J,
//     max I } over v (I = I0, J = J0; max I = -inf without a valid voxel).
//   nesvor_volume_ssim.  params = {a, b, c1, c2} in device memory.  J' = a J0 + b on v (a multiply, then an add) and 0 elsewhere,
//     I = I0 on v and 0 elsewhere, e = I - J'.  S is the separable 11-tap Gaussian window of window.h with zero padding,
//     along x, then y, then z, taps added in ascending order from 0; Wt = S(v), the moments and the SSIM formula are
//     structural.hip's (window::ssim_value).  ssim = 0 off v.  stats = { n, sum ssim, sum e^2, sum |e| } over v.
//
//   nesvor_volume_pose_moments (nesvor_amd/align.py, `evaluate --align`).  Up to 16 maps at once: for each the resampler's v
//     and { n, sum I, sum J, sum I^2, sum J^2, sum I J } over it - its stats 0, 2, 3, 4, 5, 6 - without its two volume-sized
//     outputs, R read once.  sample_voxel is the one definition of the per-voxel arithmetic for both kernels.
//
// Composed from torch operators the two are the gathers of sixteen corners with a dozen volume-sized temporaries and 3 x 11
// shifted adds over six moment volumes: a few hundred launches.  Here each is one pass and a small reduce launch.
//
// The resampling pass: a thread per R voxel, 256 consecutive voxels per workgroup.  Memory safety does not depend on M: the
// corner indices come from coordinates clamped to the lattice, a NaN coordinate (impossible with a finite M) fails the inside
// test and its indices are clamped as integers again.
//
// The SSIM pass: a 256-thread workgroup owns a 16 x 16 in-plane tile and kZChunk consecutive planes.  It marches along z from
// 5 planes before its first output plane to 5 after its last (10 planes of warm-up per chunk: the price of filling the machine
// at small in-plane sizes); planes outside the volume are the window's zero padding.  Per plane the halo, the x and y passes and their
// LDS layout are window.h's (25 KB, two barriers per plane; the x pass is a copy, for the reason given at it).  A thread keeps the six in-plane moments of its pixel for the last
// 11 planes in registers: the z step of the plane loop is specialised by the plane's index mod 11 (ring_step), so that every
// ring index is a constant and plane p lives in slot (p - first plane) mod 11.  After plane p is in, output plane p - 5 is the
// 11 slots in tap order.  The centre values of an output plane are read again from global memory (they left the halo five
// planes ago; an L2 hit).  Left to itself the compiler takes 186 VGPRs (two waves per SIMD); asked for three waves it takes
// 168 without scratch, asked for four it spills 168 bytes per lane: three it is (LDS would allow six workgroups per CU).
//
// The per-voxel arithmetic is that of the torch expressions in fp32 (coordinates: double), operation for operation (the build
// has -ffp-contract=off; the divisions are correctly rounded).  Sums: counts are exact; the float sums are added in double
// from the first add - per thread over its planes in ascending order (SSIM pass), then wave_sum_f64 and the four waves as
// (0 + 1) + (2 + 3), slice_sums.h's steps 1 and 2 in double, as structural.hip has them and for its reason.  A volume is ONE
// entry with up to 2^23 workgroup rows, so step 3 is not slice_sums.h's one thread per sum but one workgroup: thread t adds rows
// t, t + 256, .. in ascending order, then the 256 threads are added by a fixed pairwise tree in LDS.  The order is fixed by the
// shape alone: bit-identical from run to run.  max I is reduced next to the sums with fmax (exact), as masking.hip reduces its
// extremes.  No atomics, no memset: every output and every workspace row is written by exactly one thread.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include "slice_sums.h"
#include "window.h"
#include "../../include/nesvor_hip.h"

namespace {

using window::kRadius;
using window::kTaps;
using window::kTile;
using window::Taps;

constexpr int kResampleStats = 8, kSsimStats = 4;
constexpr int kZChunk = 32;                    // output planes per workgroup (EVALUATE_Z_CHUNK of nesvor_amd/ops.py)
constexpr double kEps = 1.0 / 1048576.0;       // 2^-20 voxels

struct Map { double m[12]; };

constexpr int kPoseStats = 6, kMaxPoses = 16;
constexpr int kPoseVoxels = 4;                     // voxels a thread of the multi-pose pass keeps in registers
constexpr int kPoseChunk = 256 * kPoseVoxels;      // voxels per workgroup (EVALUATE_POSE_CHUNK of nesvor_amd/ops.py)
struct Maps { double m[kMaxPoses][12]; };

// One axis: the inside test on u, then the clamped taps.  i0, i1 in [0, n - 1] whatever u is.
__device__ __forceinline__ bool axis_taps(double u, int n, int& i0, int& i1, float& f) {
  const double top = (double)(n - 1);
  const bool inside = u >= -kEps && u <= top + kEps;  // false for a NaN
  const double c = fmin(fmax(u, 0.0), top);           // (fmax / fmin drop a NaN: 0)
  const double fl = floor(c);
  i0 = min(max((int)fl, 0), n - 1);
  i1 = min(i0 + 1, n - 1);
  f = (float)(c - fl);
  return inside;
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// One R voxel (x, y, z) under one map m (12 doubles): the inside test first, then the gathers - 8 of the mask (none without
// one) and, where mX >= 0.5, 8 of the volume.  -> v (false at once off the reference mask); jv = J0 where v, untouched elsewhere.
// The resampling pass and the multi-pose moments pass both call it: one definition of the per-voxel arithmetic.
__device__ __forceinline__ bool sample_voxel(const double* m, int x, int y, int z, bool in_ref, const float* __restrict__ vol,
                                             const uint8_t* __restrict__ mask_x, int xd, int xh, int xw, float& jv) {
  const double dx = (double)x, dy = (double)y, dz = (double)z;
  const double ux = ((m[0] * dx + m[1] * dy) + m[2] * dz) + m[3];
  const double uy = ((m[4] * dx + m[5] * dy) + m[6] * dz) + m[7];
  const double uz = ((m[8] * dx + m[9] * dy) + m[10] * dz) + m[11];
  int x0, x1, y0, y1, z0, z1;
  float fx, fy, fz;
  const bool inx = axis_taps(ux, xw, x0, x1, fx), iny = axis_taps(uy, xh, y0, y1, fy), inz = axis_taps(uz, xd, z0, z1, fz);
  bool on = in_ref && inx && iny && inz;
  if (on) {
    const size_t r00 = ((size_t)z0 * xh + y0) * xw, r01 = ((size_t)z0 * xh + y1) * xw;
    const size_t r10 = ((size_t)z1 * xh + y0) * xw, r11 = ((size_t)z1 * xh + y1) * xw;
    if (mask_x != nullptr) {
      const float a00 = lerp(mask_x[r00 + x0] ? 1.f : 0.f, mask_x[r00 + x1] ? 1.f : 0.f, fx);
      const float a01 = lerp(mask_x[r01 + x0] ? 1.f : 0.f, mask_x[r01 + x1] ? 1.f : 0.f, fx);
      const float a10 = lerp(mask_x[r10 + x0] ? 1.f : 0.f, mask_x[r10 + x1] ? 1.f : 0.f, fx);
      const float a11 = lerp(mask_x[r11 + x0] ? 1.f : 0.f, mask_x[r11 + x1] ? 1.f : 0.f, fx);
      on = lerp(lerp(a00, a01, fy), lerp(a10, a11, fy), fz) >= 0.5f;
    }
    if (on) {
      const float c00 = lerp(vol[r00 + x0], vol[r00 + x1], fx), c01 = lerp(vol[r01 + x0], vol[r01 + x1], fx);
      const float c10 = lerp(vol[r10 + x0], vol[r10 + x1], fx), c11 = lerp(vol[r11 + x0], vol[r11 + x1], fx);
      jv = lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fz);
    }
  }
  return on;
}

// grid: ceil(N / 256) workgroups, N = d h w.  partial: (wgs, 8) doubles.
__global__ __launch_bounds__(256) void volume_resample_kernel(const float* __restrict__ ref, const uint8_t* __restrict__ mask_r,
                                                              const float* __restrict__ vol, const uint8_t* __restrict__ mask_x,
                                                              int h, int w, int N, int xd, int xh, int xw, Map map,
                                                              float* __restrict__ out, uint8_t* __restrict__ valid,
                                                              double* __restrict__ partial) {
  __shared__ double red[4][kResampleStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int idx = blockIdx.x * 256 + tid;  // the host checked N <= INT_MAX - 256
  const bool here = idx < N;
  const int p = here ? idx : 0;
  const int z = p / (h * w), rem = p - z * (h * w), y = rem / w, x = rem - y * w;
  const bool in_ref = here && (mask_r == nullptr || mask_r[p]);
  float iv = 0.f, jv = 0.f;
  const bool on = sample_voxel(map.m, x, y, z, in_ref, vol, mask_x, xd, xh, xw, jv);
  if (on) iv = ref[p];
  if (here) {
    out[p] = jv;
    valid[p] = on ? 1 : 0;
  }
  const double s0 = (double)wave_sum_dpp(on ? 1.f : 0.f), s1 = (double)wave_sum_dpp(in_ref ? 1.f : 0.f);
  const double s2 = wave_sum_f64(iv), s3 = wave_sum_f64(jv), s4 = wave_sum_f64(iv * iv), s5 = wave_sum_f64(jv * jv),
               s6 = wave_sum_f64(iv * jv);
  const double s7 = (double)wave_max(on ? iv : -INFINITY);  // (fmaxf: a NaN intensity does not enter)
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3;
    red[wave][4] = s4; red[wave][5] = s5; red[wave][6] = s6; red[wave][7] = s7;
  }
  __syncthreads();
  if (tid < kResampleStats - 1)
    partial[(size_t)blockIdx.x * kResampleStats + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  if (tid == kResampleStats - 1)
    partial[(size_t)blockIdx.x * kResampleStats + tid] = fmax(fmax(red[0][tid], red[1][tid]), fmax(red[2][tid], red[3][tid]));
}

// The moments of K poses in one pass over R (nesvor_amd/align.py).  grid: wgs = ceil(N / kPoseChunk) workgroups; a workgroup owns
// kPoseChunk consecutive voxels and thread t the voxels base + t + 256 j, j = 0 .. kPoseVoxels - 1, whatever K is.  The
// reference value, its mask byte and (x, y, z) of the thread's voxels are read and worked out once and stay in registers; the
// pose loop runs OUTSIDE them, so only one pose's six double accumulators are live at a time (16 x 6 would be 192 VGPRs).  Per
// pose: the thread adds its voxels in ascending order in double from the first add, wave_sum_f64, the four waves as
// (0 + 1) + (2 + 3), one row of partial (K, wgs, 6).  The maps are kernel arguments: maps.m[k] with the uniform k is scalar loads.
// The LDS rows alternate with k, so one barrier per pose is enough (row k & 1 is written again only behind barrier k + 1).
__global__ __launch_bounds__(256) void volume_pose_moments_kernel(const float* __restrict__ ref, const uint8_t* __restrict__ mask_r,
                                                                  const float* __restrict__ vol, const uint8_t* __restrict__ mask_x,
                                                                  int h, int w, int N, int xd, int xh, int xw, Maps maps, int K,
                                                                  double* __restrict__ partial) {
  __shared__ double red[2][4][kPoseStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * kPoseChunk + tid;  // (N <= INT_MAX - 256, but the last chunk may reach past INT_MAX)
  int vx[kPoseVoxels], vy[kPoseVoxels], vz[kPoseVoxels];
  float iv[kPoseVoxels];
  bool in_ref[kPoseVoxels];
#pragma unroll
  for (int j = 0; j < kPoseVoxels; ++j) {
    const int64_t idx = base + 256 * j;
    const bool here = idx < N;
    const int p = here ? (int)idx : 0;
    const int z = p / (h * w), rem = p - z * (h * w), y = rem / w;
    vx[j] = rem - y * w; vy[j] = y; vz[j] = z;
    in_ref[j] = here && (mask_r == nullptr || mask_r[p]);
    iv[j] = in_ref[j] ? ref[p] : 0.f;
  }
  const size_t wgs = gridDim.x;
  for (int k = 0; k < K; ++k) {
    const double* m = maps.m[k];
    int count = 0;
    double si = 0.0, sj = 0.0, sii = 0.0, sjj = 0.0, sij = 0.0;
#pragma unroll
    for (int j = 0; j < kPoseVoxels; ++j) {
      float jv = 0.f;
      if (sample_voxel(m, vx[j], vy[j], vz[j], in_ref[j], vol, mask_x, xd, xh, xw, jv)) {
        const float i = iv[j];
        count += 1;
        si += (double)i;
        sj += (double)jv;
        sii += (double)(i * i);
        sjj += (double)(jv * jv);
        sij += (double)(i * jv);
      }
    }
    const double s[kPoseStats] = {wave_sum_f64((double)count), wave_sum_f64(si), wave_sum_f64(sj), wave_sum_f64(sii), wave_sum_f64(sjj),
                                  wave_sum_f64(sij)};
    double (&row)[4][kPoseStats] = red[k & 1];
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kPoseStats; ++c) row[wave][c] = s[c];
    }
    __syncthreads();
    if (tid < kPoseStats) partial[((size_t)k * wgs + blockIdx.x) * kPoseStats + tid] = (row[0][tid] + row[1][tid]) + (row[2][tid] + row[3][tid]);
  }
}

// One workgroup per entry (the two passes of a comparison have one entry, the multi-pose moments one per pose): partial is
// (entries, wgs, N), stats (entries, N).  stats[j] = the wgs rows of column j: thread t combines rows t, t + 256, .. in ascending
// order, then the 256 threads are combined pairwise (stride 128, 64, .. 1).  Columns >= first_max are maxima, the others sums.
template <int N>
__global__ __launch_bounds__(256) void volume_reduce_kernel(const double* __restrict__ partial, int wgs, int first_max,
                                                            double* __restrict__ stats) {
  __shared__ double buf[N][256];
  const int tid = threadIdx.x;
  partial += (size_t)blockIdx.x * wgs * N;
  stats += (size_t)blockIdx.x * N;
  double acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = j >= first_max ? -INFINITY : 0.0;
  for (int g = tid; g < wgs; g += 256) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double v = partial[(size_t)g * N + j];
      acc[j] = j >= first_max ? fmax(acc[j], v) : acc[j] + v;
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) buf[j][tid] = acc[j];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int j = 0; j < N; ++j) buf[j][tid] = j >= first_max ? fmax(buf[j][tid], buf[j][tid + s]) : buf[j][tid] + buf[j][tid + s];
    }
    __syncthreads();
  }
  if (tid < N) stats[tid] = buf[tid][0];
}

// The z pass of one plane, specialised by s = (p - p_begin) mod 11 so that every ring index is a constant and the ring stays in
// registers (the plane loop "unrolled by 11" without eleven copies of the in-plane passes: a scalar branch picks the step).
// Plane p goes to slot S; planes p - 10 .. p are then the slots (S + 1 + t) mod 11, t = 0 .. 10.
template <int S>
__device__ __forceinline__ void ring_step(float (&ring)[kTaps][6], const float (&m)[6], const Taps& taps, bool emit, float (&out)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) ring[S][k] = m[k];
  if (!emit) return;
#pragma unroll
  for (int t = 0; t < kTaps; ++t) {
    const float g = taps.g[t];
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = out[k] + g * ring[(S + 1 + t) % kTaps][k];
  }
}

// grid: chunks * tiles workgroups, tiles = tiles_y * tiles_x per plane, chunks = ceil(d / kZChunk).  partial: (grid, 4) doubles.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void volume_ssim_kernel(const float* __restrict__ ref, const float* __restrict__ res,
                                                          const uint8_t* __restrict__ valid, const float* __restrict__ params,
                                                          int d, int h, int w, int tiles_x, int tiles, Taps taps,
                                                          float* __restrict__ ssim, double* __restrict__ partial) {
  __shared__ window::Lds lds;
  __shared__ double red[4][kSsimStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
  const int tile_y = tile / tiles_x;
  const int y0 = tile_y * kTile, x0 = (tile - tile_y * tiles_x) * kTile;
  const int z_begin = chunk * kZChunk, z_end = min(z_begin + kZChunk, d);
  const int p_begin = z_begin - kRadius, p_end = z_end + kRadius;  // the planes that enter this chunk's windows
  const float a = params[0], b = params[1], c1 = params[2], c2 = params[3];  // workgroup-uniform: the scalar path
  const int ty = tid >> 4, tx = tid & 15;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < h && gx < w;
  const size_t plane = (size_t)h * w;  // the host checked d h w <= INT_MAX - 256

  float ring[kTaps][6];
#pragma unroll
  for (int s = 0; s < kTaps; ++s)
#pragma unroll
    for (int k = 0; k < 6; ++k) ring[s][k] = 0.f;
  double sum_n = 0.0, sum_ssim = 0.0, sum_e2 = 0.0, sum_abs = 0.0;

  int s = 0;  // p - p_begin mod 11: workgroup-uniform, as p and every branch on either
  for (int p = p_begin; p < p_end; ++p, s = s + 1 == kTaps ? 0 : s + 1) {
    float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p >= 0 && p < d) {
      // the halo: I = ref, J' = a res + b on v, of plane p
      window::stage_halo(lds, y0, x0, h, w, [&](int hy, int hx, float& iv, float& jv) {
        const size_t idx = (size_t)p * plane + (size_t)hy * w + hx;
        if (!valid[idx]) return false;
        iv = ref[idx];
        jv = a * res[idx] + b;
        return true;
      });
      __syncthreads();
      // window::row_pass written out: called here (the same values, the same floating-point instructions) the kernel measured
      // 2 to 7 % slower at 128^3 and 256^3 in five of five alternating runs; the other three calls cost nothing measurable.
      for (int i = tid; i < window::kRows; i += 256) {
        const int o = (i >> 4) * window::kHaloPitch + (i & 15);
        float av = 0.f, ai = 0.f, aj = 0.f, aii = 0.f, ajj = 0.f, aij = 0.f;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
          const float g = taps.g[t], iv = lds.halo[0][o + t], jv = lds.halo[1][o + t], vv = lds.halo[2][o + t];
          av = av + g * vv;
          ai = ai + g * iv;
          aj = aj + g * jv;
          aii = aii + g * (iv * iv);
          ajj = ajj + g * (jv * jv);
          aij = aij + g * (iv * jv);
        }
        lds.mom[0][i] = av; lds.mom[1][i] = ai; lds.mom[2][i] = aj; lds.mom[3][i] = aii; lds.mom[4][i] = ajj; lds.mom[5][i] = aij;
      }
      __syncthreads();  // (the next plane's halo is written behind this barrier, its row pass writes mom behind its own first)
      window::column_pass(lds, taps, ty, tx, m);
    }

    // along z: plane p goes to slot s; output plane q = p - 5 is planes p - 10 .. p in tap order
    const int q = p - kRadius;
    const bool emit = q >= z_begin;  // (q < z_end: p < p_end)
    float wsum[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    switch (s) {
      case 0: ring_step<0>(ring, m, taps, emit, wsum); break;
      case 1: ring_step<1>(ring, m, taps, emit, wsum); break;
      case 2: ring_step<2>(ring, m, taps, emit, wsum); break;
      case 3: ring_step<3>(ring, m, taps, emit, wsum); break;
      case 4: ring_step<4>(ring, m, taps, emit, wsum); break;
      case 5: ring_step<5>(ring, m, taps, emit, wsum); break;
      case 6: ring_step<6>(ring, m, taps, emit, wsum); break;
      case 7: ring_step<7>(ring, m, taps, emit, wsum); break;
      case 8: ring_step<8>(ring, m, taps, emit, wsum); break;
      case 9: ring_step<9>(ring, m, taps, emit, wsum); break;
      default: ring_step<10>(ring, m, taps, emit, wsum); break;
    }
    if (emit && inside) {
      const size_t idx = (size_t)q * plane + (size_t)gy * w + gx;
      float value = 0.f;
      if (valid[idx]) {
        const float iv = ref[idx], jv = a * res[idx] + b;
        value = window::ssim_value(wsum, c1, c2);
        const float e = iv - jv;
        sum_n += 1.0;
        sum_ssim += (double)value;
        sum_e2 += (double)(e * e);
        sum_abs += (double)fabsf(e);
      }
      ssim[idx] = value;
    }
  }

  // (the thread sums are doubles already)
  const double s4[kSsimStats] = {wave_sum_f64(sum_n), wave_sum_f64(sum_ssim), wave_sum_f64(sum_e2), wave_sum_f64(sum_abs)};
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kSsimStats; ++j) red[wave][j] = s4[j];
  }
  __syncthreads();
  if (tid < kSsimStats) partial[(size_t)blockIdx.x * kSsimStats + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

int64_t resample_wgs(int d, int h, int w) { return ((int64_t)d * h * w + 255) / 256; }

int64_t pose_wgs(int d, int h, int w) { return ((int64_t)d * h * w + kPoseChunk - 1) / kPoseChunk; }

int64_t ssim_wgs(int d, int h, int w) { return (((int64_t)d + kZChunk - 1) / kZChunk) * slice_sums::tile_workgroups(h, w); }

}  // namespace

extern "C" int64_t nesvor_volume_resample_workspace_bytes(int d, int h, int w) {
  if (bad_volume(d, h, w)) return 0;
  return (int64_t)sizeof(double) * kResampleStats * resample_wgs(d, h, w);
}

extern "C" int nesvor_volume_resample(const float* reference, const uint8_t* reference_mask, int d, int h, int w, const float* volume,
                                      const uint8_t* volume_mask, int vd, int vh, int vw, const double* index_map, float* resampled,
                                      uint8_t* valid, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (reference == nullptr || volume == nullptr || index_map == nullptr || resampled == nullptr || valid == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  if (bad_volume(d, h, w) || bad_volume(vd, vh, vw)) return (int)hipErrorInvalidValue;
  Map map;
  for (int i = 0; i < 12; ++i) {
    if (!isfinite(index_map[i])) return (int)hipErrorInvalidValue;
    map.m[i] = index_map[i];
  }
  const int64_t wgs = resample_wgs(d, h, w);  // <= INT_MAX / 256
  if (workspace == nullptr || (int64_t)workspace_bytes < nesvor_volume_resample_workspace_bytes(d, h, w)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(volume_resample_kernel, dim3((unsigned)wgs), dim3(256), 0, st, reference, reference_mask, volume, volume_mask, h,
                     w, d * h * w, vd, vh, vw, map, resampled, valid, (double*)workspace);
  hipLaunchKernelGGL(volume_reduce_kernel<kResampleStats>, dim3(1), dim3(256), 0, st, (const double*)workspace, (int)wgs,
                     kResampleStats - 1, stats);
  return (int)hipGetLastError();
}

extern "C" int64_t nesvor_volume_pose_moments_workspace_bytes(int d, int h, int w, int K) {
  if (bad_volume(d, h, w) || K < 1 || K > kMaxPoses) return 0;
  return (int64_t)sizeof(double) * kPoseStats * K * pose_wgs(d, h, w);
}

extern "C" int nesvor_volume_pose_moments(const float* reference, const uint8_t* reference_mask, int d, int h, int w, const float* volume,
                                          const uint8_t* volume_mask, int vd, int vh, int vw, const double* index_maps, int K,
                                          double* sums, void* workspace, size_t workspace_bytes, void* stream) {
  if (K < 0 || K > kMaxPoses) return (int)hipErrorInvalidValue;
  if (reference == nullptr || volume == nullptr || (K > 0 && (index_maps == nullptr || sums == nullptr))) return (int)hipErrorInvalidValue;
  if (bad_volume(d, h, w) || bad_volume(vd, vh, vw)) return (int)hipErrorInvalidValue;
  if (K == 0) return 0;  // nothing to write, nothing launched
  Maps maps = {};
  for (int i = 0; i < 12 * K; ++i) {
    if (!isfinite(index_maps[i])) return (int)hipErrorInvalidValue;
    maps.m[i / 12][i % 12] = index_maps[i];
  }
  const int64_t wgs = pose_wgs(d, h, w);  // <= INT_MAX / 1024
  if (workspace == nullptr || (int64_t)workspace_bytes < nesvor_volume_pose_moments_workspace_bytes(d, h, w, K)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(volume_pose_moments_kernel, dim3((unsigned)wgs), dim3(256), 0, st, reference, reference_mask, volume, volume_mask, h,
                     w, d * h * w, vd, vh, vw, maps, K, (double*)workspace);
  hipLaunchKernelGGL(volume_reduce_kernel<kPoseStats>, dim3((unsigned)K), dim3(256), 0, st, (const double*)workspace, (int)wgs, kPoseStats,
                     sums);
  return (int)hipGetLastError();
}

extern "C" int64_t nesvor_volume_ssim_workspace_bytes(int d, int h, int w) {
  if (bad_volume(d, h, w) || ssim_wgs(d, h, w) > INT_MAX) return 0;
  return (int64_t)sizeof(double) * kSsimStats * ssim_wgs(d, h, w);
}

extern "C" int nesvor_volume_ssim(const float* reference, const float* resampled, const uint8_t* valid, const float* params, int d,
                                  int h, int w, float* ssim, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (reference == nullptr || resampled == nullptr || valid == nullptr || params == nullptr || ssim == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  if (bad_volume(d, h, w)) return (int)hipErrorInvalidValue;
  const int64_t wgs = ssim_wgs(d, h, w);
  if (wgs > INT_MAX) return (int)hipErrorInvalidValue;
  if (workspace == nullptr || (int64_t)workspace_bytes < nesvor_volume_ssim_workspace_bytes(d, h, w)) return (int)hipErrorInvalidValue;
  Taps taps;
  window::gaussian_taps(1.5, kRadius, taps.g);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(volume_ssim_kernel, dim3((unsigned)wgs), dim3(256), 0, st, reference, resampled, valid, params, d, h, w,
                     (int)((w + kTile - 1) / kTile), (int)slice_sums::tile_workgroups(h, w), taps, ssim, (double*)workspace);
  hipLaunchKernelGGL(volume_reduce_kernel<kSsimStats>, dim3(1), dim3(256), 0, st, (const double*)workspace, (int)wgs, kSsimStats, stats);
  return (int)hipGetLastError();
}
