// The separable 11-tap Gaussian window of the SSIM kernels (structural.hip: one slice per tile; evaluate.hip: the x and y passes
// of every plane of a volume) on a 16 x 16 tile, and the host's Gaussian taps (slice_bias.hip takes those alone).
//
// S(a) with zero padding: along x first, acc = 0; acc = acc + g[t] * a[x + t - 5] for t = 0 .. 10, then the same along y over
// the rows of acc.  The six windowed moments of a pixel are S(v, I, J, I I, J J, I J), v the validity as 0 / 1.
//
// Layout.  A 256-thread workgroup owns a 16 x 16 tile of one slice: thread t is pixel (t / 16, t % 16), so a 32-lane half of a
// wave - the group whose ds_read_b32 / ds_write_b32 addresses share 32 banks - is two tile rows.
//   halo  3 x 26 x 48 floats  I, J, v on the tile and 5 pixels around it.  Staged as 8 rows x 32 columns per sweep (26 live):
//         a half-wave writes one row, consecutive banks.  The horizontal pass's half-wave reads columns c + t, c = 0 .. 15, of
//         rows r and r + 1: with the row pitch = 16 mod 32 the two runs of 16 never share a bank (the pitch 26 would put them
//         26 banks apart: 6 two-way conflicts on every read).  48 is the smallest such pitch >= 26.
//   mom   6 x 26 x 16 floats  S_h(v, I, J, I I, J J, I J).  Pitch 16: rows r and r + 1 are 32 consecutive floats, so the horizontal
//         pass's writes and the vertical pass's reads (rows ty + t, ty + 1 + t) are conflict-free.
// 14976 + 9984 bytes of LDS: six workgroups per CU before LDS limits occupancy.  Two barriers, which the kernels place: one
// between stage_halo and row_pass, one between row_pass and column_pass.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// (unnamed: every translation unit gets a copy of its own, as slice_sums.h's)
namespace {
namespace window {

constexpr int kTile = 16;                      // the tile's edge: 256 threads
constexpr int kRadius = 5, kTaps = 2 * kRadius + 1;
constexpr int kHalo = kTile + 2 * kRadius;     // 26
constexpr int kHaloPitch = 48;                 // = 16 mod 32, >= kHalo
constexpr int kRows = kHalo * kTile;           // 416 horizontally filtered values per moment

struct Taps { float g[kTaps]; };

// a kernel declares one __shared__
struct Lds {
  float halo[3][kHalo * kHaloPitch];
  float mom[6][kRows];
};

// The halo of the tile at (y0, x0) of an h x w image: I, J, v; 0 where `load` says no and outside the image (the window's zero
// padding).  load(gy, gx, iv, jv) -> bool is called inside the image only: false off the mask, else it sets I and J.
template <typename Load>
__device__ __forceinline__ void stage_halo(Lds& lds, int y0, int x0, int h, int w, Load load) {
  const int tid = threadIdx.x, c = tid & 31;
  if (c < kHalo) {
    const int gx = x0 + c - kRadius;
    for (int r = tid >> 5; r < kHalo; r += 8) {
      const int gy = y0 + r - kRadius;
      float iv = 0.f, jv = 0.f, vv = 0.f;
      if (gy >= 0 && gy < h && gx >= 0 && gx < w && load(gy, gx, iv, jv)) vv = 1.f;
      lds.halo[0][r * kHaloPitch + c] = iv;
      lds.halo[1][r * kHaloPitch + c] = jv;
      lds.halo[2][r * kHaloPitch + c] = vv;
    }
  }
}

// along x: the six moments of the 26 rows on the tile's 16 columns.  (evaluate.hip's volume_ssim_kernel carries a copy of this
// loop and says why: a change here is made there too.)
__device__ __forceinline__ void row_pass(Lds& lds, const Taps& taps) {
  for (int i = threadIdx.x; i < kRows; i += 256) {
    const int o = (i >> 4) * kHaloPitch + (i & 15);
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
}

// along y: the taps of pixel (ty, tx) of the tile are added to m, which the caller zeroed
__device__ __forceinline__ void column_pass(const Lds& lds, const Taps& taps, int ty, int tx, float (&m)[6]) {
#pragma unroll
  for (int t = 0; t < kTaps; ++t) {
    const float g = taps.g[t];
    const int o = (ty + t) * kTile + tx;
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = m[k] + g * lds.mom[k][o];
  }
}

// the SSIM of a valid pixel from its windowed moments S(v, I, J, I I, J J, I J): Wt = m[0] >= g[5]^2 > 0 (g[5]^3 in a volume)
__device__ __forceinline__ float ssim_value(const float (&m)[6], float c1, float c2) {
  const float mu_i = m[1] / m[0], mu_j = m[2] / m[0];
  const float var_i = m[3] / m[0] - mu_i * mu_i, var_j = m[4] / m[0] - mu_j * mu_j, cov = m[5] / m[0] - mu_i * mu_j;
  const float num = (2.f * mu_i * mu_j + c1) * (2.f * cov + c2);
  const float den = (mu_i * mu_i + mu_j * mu_j + c1) * (var_i + var_j + c2);
  return num / den;
}

// g[t] = exp(-(t - radius)^2 / (2 sigma^2)), t = 0 .. 2 radius, normalised to sum 1, in double, rounded to fp32 once; 0 beyond.
// The caller checked 2 radius < N.
template <int N>
inline void gaussian_taps(double sigma, int radius, float (&g)[N]) {
  double e[N], sum = 0.0;
  for (int t = 0; t <= 2 * radius; ++t) {
    e[t] = exp(-(double)((t - radius) * (t - radius)) / (2.0 * sigma * sigma));
    sum += e[t];
  }
  for (int t = 0; t < N; ++t) g[t] = t <= 2 * radius ? (float)(e[t] / sum) : 0.f;
}

}  // namespace window
}  // namespace
