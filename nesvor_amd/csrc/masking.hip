// Stack masking (nesvor_amd/masking.py) on gfx950: which voxels of a stack count, decided in one pass per stack.
//
// A stack's mask is narrowed by up to three per-voxel rules (each only removes voxels): an intensity threshold, a world-space
// mask volume, and the intersection with the slabs of every other stack.  Composed from torch operators the last one is a loop
// over all slices of all other stacks with (N,3) fp64 temporaries each, the second a gather of eight corners per voxel; here
//   nesvor_stack_mask      one launch over the voxels of a stack does the three rules and the per-slice {count, min, max} of the
//                          kept intensities, a small second launch adds the per-workgroup partials,
//   nesvor_otsu_histogram  the integer histogram of the kept intensities between the reduced min and max (read from the device),
//   nesvor_otsu_threshold  one workgroup: histogram and range -> Otsu's threshold, a device float nesvor_stack_mask takes back as
//                          its threshold, so applying it needs no host read.
//
// Arithmetic.  Positions are double from the pixel index on (gfx950 runs fp64 at the fp32 rate, and the decisions are
// comparisons against faces and 0.5: the composed fp64 path's values).  A pixel (r, c) of slice s lies at
//   p = R_s (x + t_s),  x = ((c - (w - 1) / 2) rx, (r - (h - 1) / 2) ry, 0)          [R_s | t_s] = transforms[s], fp32
// The count is added in slice_sums.h's order (exact: at most 64 ones per wave in fp32, double beyond), min and max next to it
// in the same fixed order (fmin / fmax: a NaN intensity never enters them).  No global atomics, no memset, no spin-wait: every
// workgroup stores its partials, follow-up launches combine them in workgroup order.  The histogram's LDS atomics are integer
// adds, so the order they retire in does not matter: bit-identical results from run to run.
//
// Memory safety does not depend on the inputs' values: slab offsets are clamped to the table, lattice indices are tested
// against the volume's shape before a byte is read, bin indices are clamped to [0, n_bins - 1].
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "slice_sums.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kStats = 3;        // {count, min, max}
constexpr int kChunk = 64;       // world-to-slice matrices per LDS chunk (6 KB)

// One axis of the trilinear lookup: u the continuous voxel index; i0 = floor u and the weight of i0 + 1.  false: both
// neighbours are off the axis (also for a NaN), the value is 0.
__device__ __forceinline__ bool axis_taps(double u, int n, int& i0, double& f) {
  if (!(u > -1.0 && u < (double)n)) return false;
  const double fl = floor(u);
  i0 = (int)fl;  // in [-1, n - 1]
  f = u - fl;
  return true;
}

// The mask volume (bytes, any set byte = 1, 0 off the lattice) interpolated at lattice coordinates (ux, uy, uz).
__device__ __forceinline__ double sample_volume_mask(const uint8_t* __restrict__ vol, int vd, int vh, int vw, double ux, double uy,
                                                     double uz) {
  int x0, y0, z0;
  double fx, fy, fz;
  if (!axis_taps(ux, vw, x0, fx) || !axis_taps(uy, vh, y0, fy) || !axis_taps(uz, vd, z0, fz)) return 0.0;
  double acc = 0.0;  // corners in the order z, y, x ascending
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int z = z0 + dz, y = y0 + dy, x = x0 + dx;
        if (z < 0 || z >= vd || y < 0 || y >= vh || x < 0 || x >= vw) continue;
        if (vol[((size_t)z * vh + y) * vw + x] == 0) continue;
        acc += ((dz ? fz : 1.0 - fz) * (dy ? fy : 1.0 - fy)) * (dx ? fx : 1.0 - fx);
      }
  return acc;
}

// grid: n * wgs workgroups of 256 pixels, wgs = ceil(hw / 256) per slice.  partial: (n, wgs, 3) doubles.
// slabs: (n_slabs, 3, 4) doubles, q = M[:, :3] p + M[:, 3]; extents (n_others, 3) the half-extents {x, y, z} of every other
// stack's slices; offsets (n_others + 1) the first matrix of every other stack.
__global__ __launch_bounds__(256) void stack_mask_kernel(const float* __restrict__ slices, const uint8_t* __restrict__ mask,
                                                         const float* __restrict__ transforms, int h, int w, int wgs, double rx,
                                                         double ry, const float* __restrict__ threshold,
                                                         const uint8_t* __restrict__ volume, int vd, int vh, int vw,
                                                         const double* __restrict__ vgeom, const double* __restrict__ slabs,
                                                         const double* __restrict__ extents, const int32_t* __restrict__ offsets,
                                                         int n_others, int n_slabs, uint8_t* __restrict__ out,
                                                         double* __restrict__ partial) {
  __shared__ double tab[kChunk * 12];
  __shared__ double red[4][2];
  const int tid = threadIdx.x, hw = h * w;
  const int is = blockIdx.x / wgs, wg = blockIdx.x - is * wgs;
  const int pix = wg * 256 + tid;  // the host checked hw <= INT_MAX - 256
  const bool inside = pix < hw;
  const size_t idx = (size_t)is * hw + (inside ? pix : 0);
  const float v = slices[idx];
  bool keep = inside && (mask == nullptr || mask[idx]);
  if (threshold != nullptr) keep = keep && v > threshold[0];  // false for a NaN on either side

  double px = 0.0, py = 0.0, pz = 0.0;
  if (volume != nullptr || n_others > 0) {
    const float* T = transforms + 12 * (size_t)is;  // workgroup-uniform: the scalar path
    const int r = pix / w, c = pix - r * w;
    const double ax = ((double)c - 0.5 * (double)(w - 1)) * rx + (double)T[3];
    const double ay = ((double)r - 0.5 * (double)(h - 1)) * ry + (double)T[7];
    const double az = (double)T[11];
    px = ((double)T[0] * ax + (double)T[1] * ay) + (double)T[2] * az;
    py = ((double)T[4] * ax + (double)T[5] * ay) + (double)T[6] * az;
    pz = ((double)T[8] * ax + (double)T[9] * ay) + (double)T[10] * az;
  }

  if (volume != nullptr && keep) {
    // vgeom: world-to-lattice (3,4) then the voxel sizes {x, y, z}; u = (M p + t) / size + (shape - 1) / 2
    const double lx = ((vgeom[0] * px + vgeom[1] * py) + vgeom[2] * pz) + vgeom[3];
    const double ly = ((vgeom[4] * px + vgeom[5] * py) + vgeom[6] * pz) + vgeom[7];
    const double lz = ((vgeom[8] * px + vgeom[9] * py) + vgeom[10] * pz) + vgeom[11];
    const double ux = lx / vgeom[12] + 0.5 * (double)(vw - 1), uy = ly / vgeom[13] + 0.5 * (double)(vh - 1),
                 uz = lz / vgeom[14] + 0.5 * (double)(vd - 1);
    keep = sample_volume_mask(volume, vd, vh, vw, ux, uy, uz) >= 0.5;
  }

  // every other stack must have a slice whose slab contains p.  The two outer loops and the barriers are workgroup-uniform
  // (offsets are); only the scan of a chunk in LDS ends early, per thread, at the first containing slice.
  for (int k = 0; k < n_others; ++k) {
    const int begin = min(max(offsets[k], 0), n_slabs), end = min(max(offsets[k + 1], begin), n_slabs);
    const double ex = extents[3 * k], ey = extents[3 * k + 1], ez = extents[3 * k + 2];
    bool found = false;
    for (int c0 = begin; c0 < end; c0 += kChunk) {
      const int m = min(kChunk, end - c0);
      __syncthreads();  // the readers of the chunk before
      for (int i = tid; i < m * 12; i += 256) tab[i] = slabs[(size_t)c0 * 12 + i];
      __syncthreads();
      if (keep && !found) {
        for (int t = 0; t < m; ++t) {
          const double* M = tab + 12 * t;  // one address for the wave: a broadcast read
          const double qz = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11];
          if (!(fabs(qz) <= ez)) continue;
          const double qx = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3];
          const double qy = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7];
          if (fabs(qx) <= ex && fabs(qy) <= ey) {
            found = true;
            break;
          }
        }
      }
    }
    keep = keep && found;
  }

  if (inside) out[idx] = keep ? 1 : 0;

  double* row = partial + ((size_t)is * wgs + wg) * kStats;
  const float cnt[1] = {wave_sum_dpp(keep ? 1.f : 0.f)};
  const double lo = wave_min_f64(keep ? (double)v : INFINITY), hi = wave_max_f64(keep ? (double)v : -INFINITY);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = lo;
    red[tid >> 6][1] = hi;
  }
  slice_sums::store_workgroup_sums(cnt, row);  // row[0]; its barrier also publishes red
  if (tid == 1) row[1] = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
  if (tid == 2) row[2] = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
}

// stats[s] = the wgs partials of slice s combined in workgroup order
__global__ __launch_bounds__(256) void stack_mask_reduce_kernel(const double* __restrict__ partial, int n, int wgs,
                                                                double* __restrict__ stats) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  double cnt = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int g = 0; g < wgs; ++g) {
    const double* p = partial + ((size_t)s * wgs + g) * kStats;
    cnt += p[0];
    lo = fmin(lo, p[1]);
    hi = fmax(hi, p[2]);
  }
  stats[(size_t)s * kStats] = cnt;
  stats[(size_t)s * kStats + 1] = lo;
  stats[(size_t)s * kStats + 2] = hi;
}

// ---------------------------------------------------------------------------------------------------------------------
// Otsu.  histogram: G <= kHistWgs workgroups striding over the voxels; partial (G, n_bins) 32-bit counts (N < 2^31)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void otsu_histogram_kernel(const float* __restrict__ slices, const uint8_t* __restrict__ mask,
                                                             const double* __restrict__ range, int64_t N, int n_bins,
                                                             unsigned int* __restrict__ partial) {
  __shared__ unsigned int bins[kMaxBins];
  for (int i = threadIdx.x; i < n_bins; i += 256) bins[i] = 0u;
  __syncthreads();
  const double lo = range[0], width = (range[1] - lo) / (double)n_bins;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += stride) {
    if (mask != nullptr && !mask[p]) continue;
    const double c = ((double)slices[p] - lo) / width;
    if (!(c >= 0.0)) continue;  // a NaN intensity, an empty or flat range (0 / 0): not counted
    atomicAdd(&bins[(int)fmin(floor(c), (double)(n_bins - 1))], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_bins; i += 256) partial[(size_t)blockIdx.x * n_bins + i] = bins[i];
}

__global__ __launch_bounds__(256) void otsu_histogram_reduce_kernel(const unsigned int* __restrict__ partial, int G, int n_bins,
                                                                    int64_t* __restrict__ hist) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_bins) return;
  int64_t s = 0;
  for (int g = 0; g < G; ++g) s += (int64_t)partial[(size_t)g * n_bins + b];
  hist[b] = s;
}

// One workgroup.  Bin centres m_i = lo + (i + 0.5) width; for the split after bin i (i = 0 .. n_bins - 2) the classes are the
// bins <= i and > i: var_i = w0 w1 (mu0 - mu1)^2 with the class weights and the class means of the centres; the running sums
// are added in ascending bin order by one thread, the first maximum wins.  out = (float)m_i, or -inf for fewer than two
// counted voxels or a range that is not lo < hi.
__global__ __launch_bounds__(256) void otsu_threshold_kernel(const int64_t* __restrict__ hist, const double* __restrict__ range,
                                                             int n_bins, float* __restrict__ out) {
  __shared__ double cum_n[kMaxBins], cum_s[kMaxBins];
  __shared__ double best_v[256];
  __shared__ int best_i[256];
  const int tid = threadIdx.x;
  const double lo = range[0], hi = range[1], width = (hi - lo) / (double)n_bins;
  for (int i = tid; i < n_bins; i += 256) {
    const double c = (double)hist[i];  // below 2^31: exact
    cum_n[i] = c;
    cum_s[i] = c * (lo + ((double)i + 0.5) * width);
  }
  __syncthreads();
  if (tid == 0) {
    double n = 0.0, s = 0.0;
    for (int i = 0; i < n_bins; ++i) {
      n += cum_n[i];
      s += cum_s[i];
      cum_n[i] = n;
      cum_s[i] = s;
    }
  }
  __syncthreads();
  const double total_n = cum_n[n_bins - 1], total_s = cum_s[n_bins - 1];
  double bv = -1.0;
  int bi = INT_MAX;
  for (int i = tid; i < n_bins - 1; i += 256) {  // ascending: a later equal value does not replace an earlier one
    const double n0 = cum_n[i], n1 = total_n - n0;
    double var = 0.0;
    if (n0 > 0.0 && n1 > 0.0) {
      const double d = cum_s[i] / n0 - (total_s - cum_s[i]) / n1;
      var = ((n0 / total_n) * (n1 / total_n)) * (d * d);
    }
    if (var > bv) {
      bv = var;
      bi = i;
    }
  }
  best_v[tid] = bv;
  best_i[tid] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t)
      if (best_v[t] > bv || (best_v[t] == bv && best_i[t] < bi)) {
        bv = best_v[t];
        bi = best_i[t];
      }
    const bool usable = total_n >= 2.0 && hi > lo && bi < n_bins - 1;
    out[0] = usable ? (float)(lo + ((double)bi + 0.5) * width) : -INFINITY;
  }
}

bool bad_stack(int n, int h, int w) {
  return n < 1 || h < 1 || w < 1 || (int64_t)h * w > (int64_t)INT_MAX - 256 || (int64_t)n * h * w > (int64_t)INT_MAX - 256;
}

}  // namespace

extern "C" int64_t nesvor_stack_mask_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return slice_sums::Plan<kStats>{n, slice_sums::pixel_workgroups(h, w)}.workspace_bytes();
}

extern "C" int nesvor_stack_mask(const float* slices, const uint8_t* mask, const float* transforms, int n, int h, int w, double rx,
                                 double ry, const float* threshold, const uint8_t* volume, int vd, int vh, int vw,
                                 const double* volume_geometry, const double* slabs, const double* slab_extents,
                                 const int32_t* slab_offsets, int n_others, int n_slabs, uint8_t* out_mask, double* stats,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (n < 1 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if (slices == nullptr || transforms == nullptr || out_mask == nullptr || stats == nullptr) return (int)hipErrorInvalidValue;
  if (!(rx > 0.0) || !(ry > 0.0) || !isfinite(rx) || !isfinite(ry)) return (int)hipErrorInvalidValue;
  if (volume != nullptr) {
    if (volume_geometry == nullptr || vd < 1 || vh < 1 || vw < 1 || (int64_t)vd * vh * vw > (int64_t)INT_MAX)
      return (int)hipErrorInvalidValue;
  }
  if (n_others < 0 || n_slabs < 0) return (int)hipErrorInvalidValue;
  if (n_others > 0 && (slabs == nullptr || slab_extents == nullptr || slab_offsets == nullptr)) return (int)hipErrorInvalidValue;
  const slice_sums::Plan<kStats> plan{n, slice_sums::pixel_workgroups(h, w)};
  if (!plan.accepts(h, w, plan.wgs * n, workspace, workspace_bytes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stack_mask_kernel, dim3((unsigned)(plan.wgs * n)), dim3(256), 0, st, slices, mask, transforms, h, w, (int)plan.wgs,
                     rx, ry, threshold, volume, vd, vh, vw, volume_geometry, slabs, slab_extents, slab_offsets, n_others, n_slabs,
                     out_mask, (double*)workspace);
  hipLaunchKernelGGL(stack_mask_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)workspace, n,
                     (int)plan.wgs, stats);
  return (int)hipGetLastError();
}

extern "C" int64_t nesvor_otsu_histogram_workspace_bytes(int n, int h, int w, int n_bins) {
  if (bad_stack(n, h, w) || n_bins < 2 || n_bins > kMaxBins) return 0;
  return (int64_t)sizeof(unsigned int) * n_bins * hist_wgs((int64_t)n * h * w);
}

extern "C" int nesvor_otsu_histogram(const float* slices, const uint8_t* mask, int n, int h, int w, const double* range, int n_bins,
                                     int64_t* hist, void* workspace, size_t workspace_bytes, void* stream) {
  if (slices == nullptr || range == nullptr || hist == nullptr) return (int)hipErrorInvalidValue;
  if (bad_stack(n, h, w) || n_bins < 2 || n_bins > kMaxBins) return (int)hipErrorInvalidValue;
  const int64_t need = nesvor_otsu_histogram_workspace_bytes(n, h, w, n_bins);
  if (workspace == nullptr || (int64_t)workspace_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)n * h * w;
  const int G = hist_wgs(N);
  hipLaunchKernelGGL(otsu_histogram_kernel, dim3((unsigned)G), dim3(256), 0, st, slices, mask, range, N, n_bins,
                     (unsigned int*)workspace);
  hipLaunchKernelGGL(otsu_histogram_reduce_kernel, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, st,
                     (const unsigned int*)workspace, G, n_bins, hist);
  return (int)hipGetLastError();
}

extern "C" int64_t nesvor_otsu_threshold_workspace_bytes(int n_bins) {
  (void)n_bins;
  return 0;  // the one workgroup works in LDS
}

extern "C" int nesvor_otsu_threshold(const int64_t* hist, const double* range, int n_bins, float* threshold, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (hist == nullptr || range == nullptr || threshold == nullptr) return (int)hipErrorInvalidValue;
  if (n_bins < 2 || n_bins > kMaxBins) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(otsu_threshold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, range, n_bins, threshold);
  return (int)hipGetLastError();
}
