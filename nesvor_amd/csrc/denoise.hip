// Stack denoising (gfx950): 2-D non-local means of every slice of a stack in one launch, plus the ordered reduction of the two
// per-slice sums.
//
// Definition (nesvor_amd/denoise.py::nlm_composed, include/nesvor_hip.h).  With m the validity as 0 / 1 (0 outside the image),
// y0 = y on valid pixels and 0 elsewhere, P the patch radius, S the search radius, for a valid pixel p of a slice with sigma > 0:
//   candidates   q = p + t, t in [-S,S]^2 \ {0}, m(q) = 1, in ascending (t_y, t_x)
//   c_o = m(p+o) m(q+o),  e_o = c_o (y0(p+o) - y0(q+o))^2,  o in [-P,P]^2;  num = sum e_o, den = sum c_o, along x first, then y
//   d2 = num / max(den, 1),  w = exp(-(max(d2 - 2 sigma^2, 0) / (beta sigma)^2))
//   w_c = max_q w or 1 without a candidate,  W = w_c + sum_q w,  V = w_c y(p) + sum_q w y(q),  out(p) = V / W (y(p) where W = 0)
// Invalid pixels and slices whose sigma is not positive and finite are copied.  stats = { #valid, sum_valid (out - y)^2 }.
//
// Composed from torch operators this is (2 S + 1)^2 - 1 shifts of some 4 P + 20 launches over slice-sized temporaries each (48
// shifts at the defaults, 440 at S = 10).  Here a 256-thread workgroup owns a 16 x 16 tile of one slice (thread t is pixel
// (t / 16, t % 16), as in structural.hip and slice_bias.hip): the tile and its S + P halo go to LDS once, as {y0, m} pairs, and
// every thread produces its pixel from LDS alone; no weight and no distance ever exists in memory.
//
// Schedule: shift by shift (the loop over t is workgroup-uniform), three steps with two barriers per shift.
//   1. {e, c} of the shift on the tile extended by P, E x E pixels with E = 16 + 2 P <= 22: at most two per thread, whose own
//      {y0, m} stay in registers over all shifts, so a pixel costs one LDS read (the shifted pair) and one write.
//   2. The row sums over 2 P + 1 columns for the E rows of the tile's 16 columns: E x 16 entries, at most two per thread.
//   3. Every thread whose pixel and candidate are valid adds 2 P + 1 row sums down its column: num and den; the weight follows.
// A pair {e, c} or {row sum of e, row sum of c} is one float2, so every access is a ds_read_b64 / ds_write_b64.  The other
// schedule - every thread walking its own (2 P + 1)^2 patch per candidate, (2 P + 1)^2 reads instead of some 2 (2 P + 1) + 4 -
// gives the same bits and was measured: equal at P = 1, 1.7 x slower at P = 2 and 2.3 x at P = 3 ("Stack denoising").
// Hazards: step 1 of the next shift writes what step 2 read (the barrier after step 2 lies between), step 2 of the next shift
// writes what step 3 read (the barrier after the next step 1 lies between).
//
// LDS banks.  ds_read_b64 is served in 32-lane halves over 64 banks.  The stage and the {e, c} tile have a pitch of 48 pairs
// = 96 dwords: in step 2 a half reads two rows of 16 pairs = 32 dwords each, and 96 = 32 (mod 64) puts the second row on the
// other 32 banks.  The row sums have the pitch 16: the two rows of a half are 64 consecutive dwords.  Step 1 walks the E x E
// tile in row-major order (runs of E consecutive pairs).  42 x 48 + 22 x 48 + 22 x 16 pairs = 27392 bytes at the limits.
//
// The per-pixel arithmetic is that of the torch expression in fp32, operation for operation and in its order (the build has
// -ffp-contract=off; the divisions are correctly rounded, expf is the library's, the one torch's fp32 exp calls): on MI355X the
// kernel and the expression in fp32 give equal bits on every case of tests/test_gpu_denoise.py.  The sums are added in the
// reproducible order of slice_sums.h, a workgroup being a tile; the count in fp32 inside a wave (at most 64 ones: exact), the
// squares in double from the first add (wave_sum_f64), as structural.hip and slice_bias.hip do and say why.
// Memory safety does not depend on a value: every index is a function of n, h, w, P and S, which the host checks.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kStats = 2;
constexpr int kTile = 16;
constexpr int kMaxPatch = 3, kMaxSearch = 10;
constexpr int kMaxSpan = kTile + 2 * (kMaxSearch + kMaxPatch);  // 42 rows and columns
constexpr int kPitch = 48;                                      // pairs per LDS row: >= kMaxSpan, 2 kPitch = 32 (mod 64)
static_assert(kPitch >= kMaxSpan && (2 * kPitch) % 64 == 32, "the pitch holds a row and alternates the bank halves");

// grid: n * tiles workgroups, tiles = tiles_y * tiles_x per slice.  partial: (n, tiles, 2) doubles.
template <int P>
__global__ __launch_bounds__(256) void nlm_denoise_kernel(const float* __restrict__ y, const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ sigma, int h, int w, int tiles_x, int tiles, int S,
                                                          float beta, float* __restrict__ out, double* __restrict__ partial) {
  constexpr int D = 2 * P + 1, E = kTile + 2 * P;
  static_assert(E * E <= 512 && E * kTile <= 512, "at most two entries per thread in steps 1 and 2");
  __shared__ float2 stage[kMaxSpan * kPitch];  // {y0, m} of the tile and its halo
  __shared__ float2 ebuf[E * kPitch];          // {e, c} of the current shift on the extended tile
  __shared__ float2 rbuf[E * kTile];           // their row sums on the tile's columns
  __shared__ double red[4][kStats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int in = blockIdx.x / tiles, tile = blockIdx.x - in * tiles;
  const int tile_y = tile / tiles_x;
  const int y0 = tile_y * kTile, x0 = (tile - tile_y * tiles_x) * kTile;
  const size_t base = (size_t)in * h * w;  // the host checked h w <= INT_MAX - 256
  const int R = S + P, span = kTile + 2 * R;
  const float sg = sigma[in];                 // workgroup-uniform: the scalar path
  const bool ok = sg > 0.f && sg <= FLT_MAX;  // positive and finite (a NaN fails the first test)

  const int ty = tid >> 4, tx = tid & 15;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < h && gx < w;
  const size_t idx = base + (size_t)gy * w + gx;  // (only used where `inside`)
  float yv = 0.f, o = 0.f;
  bool valid = false;
  if (inside) {
    yv = y[idx];
    valid = mask == nullptr || mask[idx];
    o = yv;
  }

  if (ok) {  // (workgroup-uniform, as are the loops over the shifts: every barrier is reached by all threads or by none)
    // the tile and its halo; {0, 0} outside the image and off the mask
    for (int i = tid; i < span * span; i += 256) {
      const int r = i / span, c = i - r * span;
      const int py = y0 - R + r, px = x0 - R + c;
      float2 v = make_float2(0.f, 0.f);
      if (py >= 0 && py < h && px >= 0 && px < w) {
        const size_t j = base + (size_t)py * w + px;
        if (mask == nullptr || mask[j]) v = make_float2(y[j], 1.f);
      }
      stage[r * kPitch + c] = v;
    }
    __syncthreads();

    const float two_s2 = 2.f * (sg * sg);
    const float hs = beta * sg;
    const float h2 = hs * hs;
    // step 1's pixels of this thread, (r, c) of the extended tile = (S + r, S + c) of the stage: rows up to S + E - 1 + S = span - 1
    int mine[2], park[2];
    float2 a[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = j * 256 + tid < E * E ? j * 256 + tid : 0;
      const int r = i / E, c = i - r * E;
      mine[j] = (S + r) * kPitch + S + c;
      park[j] = r * kPitch + c;
      a[j] = stage[mine[j]];
    }
    const int centre_at = (ty + R) * kPitch + tx + R;
    float acc_w = 0.f, acc_wy = 0.f, wmax = 0.f;
    bool any = false;
    for (int dy = -S; dy <= S; ++dy) {
      for (int dx = -S; dx <= S; ++dx) {
        if (dy == 0 && dx == 0) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (j * 256 + tid < E * E) {
            const float2 b = stage[mine[j] + dy * kPitch + dx];
            const float diff = a[j].x - b.x;
            const float cc = a[j].y * b.y;
            ebuf[park[j]] = make_float2(cc * (diff * diff), cc);
          }
        }
        __syncthreads();
        for (int i = tid; i < E * kTile; i += 256) {
          const int r = i >> 4, x = i & 15;
          float2 s = ebuf[r * kPitch + x];
#pragma unroll
          for (int ox = 1; ox < D; ++ox) {
            const float2 t = ebuf[r * kPitch + x + ox];  // x + ox <= 15 + 2 P = E - 1
            s.x = s.x + t.x;
            s.y = s.y + t.y;
          }
          rbuf[i] = s;
        }
        __syncthreads();
        if (valid) {
          const float2 centre = stage[centre_at + dy * kPitch + dx];
          if (centre.y != 0.f) {  // an invalid candidate: its weight is an exact 0 that adds nothing
            float2 s = rbuf[ty * kTile + tx];
#pragma unroll
            for (int oy = 1; oy < D; ++oy) {
              const float2 t = rbuf[(ty + oy) * kTile + tx];
              s.x = s.x + t.x;
              s.y = s.y + t.y;
            }
            const float d2 = s.x / fmaxf(s.y, 1.f);
            const float x = fmaxf(d2 - two_s2, 0.f);
            const float wgt = expf(-(x / h2));
            acc_w = acc_w + wgt;
            acc_wy = acc_wy + wgt * centre.x;
            wmax = fmaxf(wmax, wgt);
            any = true;
          }
        }
      }
    }
    if (valid) {
      const float wc = any ? wmax : 1.f;
      const float W = wc + acc_w;
      const float V = wc * yv + acc_wy;
      if (W > 0.f) o = V / W;
    }
  }
  if (inside) out[idx] = o;

  const float d = valid ? o - yv : 0.f;
  const double s0 = (double)wave_sum_dpp(valid ? 1.f : 0.f);
  const double s1 = wave_sum_f64(d * d);
  // (step 2 of slice_sums.h written out, as structural.hip has it and says why)
  if (lane == 0) {
    red[wave][0] = s0;
    red[wave][1] = s1;
  }
  __syncthreads();
  if (tid < kStats) partial[((size_t)in * tiles + tile) * kStats + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

}  // namespace

extern "C" int64_t nesvor_nlm_denoise_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1 || (int64_t)h * w > INT_MAX - 256) return 0;
  return slice_sums::Plan<kStats>{n, slice_sums::tile_workgroups(h, w)}.workspace_bytes();
}

extern "C" int nesvor_nlm_denoise(const float* y, const uint8_t* mask, const float* sigma, int n, int h, int w, int patch_radius,
                                  int search_radius, float strength, float* out, double* stats, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (y == nullptr || sigma == nullptr || out == nullptr || stats == nullptr || out == y) return (int)hipErrorInvalidValue;
  if (patch_radius < 1 || patch_radius > kMaxPatch || search_radius < 1 || search_radius > kMaxSearch) return (int)hipErrorInvalidValue;
  if (!(strength > 0.f && strength <= FLT_MAX)) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kStats> plan{n, slice_sums::tile_workgroups(h, w)};  // a workgroup per tile
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(plan.wgs * n)), block(256);
  const int tiles_x = (w + kTile - 1) / kTile;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  switch (patch_radius) {
    case 1:
      hipLaunchKernelGGL(nlm_denoise_kernel<1>, grid, block, 0, st, y, mask, sigma, h, w, tiles_x, (int)plan.wgs, search_radius, strength,
                         out, partial);
      break;
    case 2:
      hipLaunchKernelGGL(nlm_denoise_kernel<2>, grid, block, 0, st, y, mask, sigma, h, w, tiles_x, (int)plan.wgs, search_radius, strength,
                         out, partial);
      break;
    default:
      hipLaunchKernelGGL(nlm_denoise_kernel<3>, grid, block, 0, st, y, mask, sigma, h, w, tiles_x, (int)plan.wgs, search_radius, strength,
                         out, partial);
  }
  plan.reduce(workspace, stats, st);
  return (int)hipGetLastError();
}
