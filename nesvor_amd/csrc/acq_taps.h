// The PSF-tap core of the slice-acquisition operators: the kernels of slice_acq.hip (A, A^T and both backwards, linear and
// interp_psf modes) and the svr statistics (svr.hip, svr_nmi.hip), which simulate A<float> under several poses per pixel through
// simulate_pixel, the one statement of that pixel outside slice_acq_fwd.  Two kernels of
// slice_acq.hip keep their tap loops written out for speed: slice_acq_adjoint_gather (the parent's test: it indexes nothing by a
// tap's position; under a non-finite pose A^T hands the NaN on into vol and vol_weight) and slice_acq_adjoint_bwd (this
// header's order spelled out, its NaN rule in the hoisted form: pose_is_bounded).
//
// A slice pixel sits at q = (qx, qy, qz) in its slice's frame and at c = R q + (dims - 1) / 2 in the volume (pixel_geom); PSF tap
// (ox, oy, oz) samples the volume at p = c + R (ox, oy, oz) (tap_position).  What this header fixes, so that the kernels agree
// bit for bit (the build compiles with -ffp-contract=off):
//   * the affine map of q in double, rounded once (the reference: slice_acq_cuda_kernel.cu:46-47); c and p in T, added left to right;
//   * the taps in the order of the dense PSF array (ip = (iz d_h + iy) d_w + ix), zero taps skipped - walked densely from global
//     memory (for_psf_taps) or from a compacted LDS list (compact_taps, for_lds_taps);
//   * a tap counts iff 0 <= p < dims - 1 on every axis.  The test is written so that a NaN coordinate FAILS it: a non-finite
//     pose skips every tap (the pixel gets no weight) in every kernel that indexes the volume by p, instead of reaching
//     (int)floor(p) and a volume index.  Two forms: tap_position's ordered compares per tap, or pose_is_bounded once per
//     slice in front of a pixel loop whose tap loop keeps the plain `x < 0 || ... || z >= D - 1`;
//   * the forward operator's linear tap in the reference's corner order 000, 100, 010, 001, 110, 101, 011, 111, eight loads
//     before eight accumulations (linear_tap); the two pose-gradient kernels walk the same cell with corner c = 0 .. 7 by bits,
//     x lowest (cell_corner, add_corner_gradient), and add the 12 pose sums per tap (accumulate_pose_grad) and per slice
//     (reduce_pose_grad: wave_sum, then the four waves as (0 + 1) + (2 + 3)) in one order.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "common.h"

// (unnamed: every translation unit gets a copy of its own, as slice_sums.h's)
namespace {
namespace acq {

constexpr int kMaxTaps = 1024;  // the LDS list's capacity: 16 KB of float taps

template <typename T> struct Tap { T x, y, z, w; };

// The PSF's non-zero taps, in the order of the dense array, into `taps` (kMaxTaps entries: the host checked d_p h_p w_p <= kMaxTaps);
// returns their number.  One thread calls; the caller publishes the count and places the barrier.
template <typename T>
__device__ __forceinline__ int compact_taps(const T* __restrict__ psf, int d_p, int h_p, int w_p, Tap<T>* taps) {
  int cnt = 0, ip = 0;
  for (int iz = -d_p / 2; iz < (d_p + 1) / 2; ++iz)
    for (int iy = -h_p / 2; iy < (h_p + 1) / 2; ++iy)
      for (int ix = -w_p / 2; ix < (w_p + 1) / 2; ++ix, ++ip) {
        const T pv = psf[ip];
        if (pv != (T)0.0) taps[cnt++] = Tap<T>{(T)ix, (T)iy, (T)iz, pv};
      }
  return cnt;
}

// Which PSF a slice takes.  A kernel is written once over a source S with `S::at(k)`, the PSF of slice k as a view; k is uniform
// over a workgroup (the forward, svr) or over the launch (the k loop of the voxel gather), so the id and the table row stay in
// scalar registers: read once per slice, never per tap.
template <typename T> struct PsfView { const T* psf; int d, h, w; };

// One PSF for every slice (the kernels' first form; at() is loop-invariant and costs nothing).
template <typename T> struct OnePsf {
  const T* psf; int d, h, w;
  __device__ __forceinline__ PsfView<T> at(int) const { return PsfView<T>{psf, d, h, w}; }
};

// A PSF bank: P dense PSFs of their own sizes concatenated in `data`, row p of the table {offset in elements, d_p, h_p, w_p}, one
// id per slice in device memory.  The table travels by value as a kernel argument (the host checked it: P <= kMaxBankMembers,
// positive sizes); an id outside [0, P) gives the empty view - no taps (compact_taps and for_psf_taps walk nothing of a 0 x 0 x 0
// PSF, the gather's tap range iz = 0 .. -1 is empty), nothing indexed.
constexpr int kMaxBankMembers = 32;
template <typename T> struct BankPsf {
  const T* data;
  const int* ids;
  int P;
  int table[kMaxBankMembers][4];
  __device__ __forceinline__ PsfView<T> at(int k) const {
    const int id = ids[k];
    if (id < 0 || id >= P) return PsfView<T>{data, 0, 0, 0};
    return PsfView<T>{data + table[id][0], table[id][1], table[id][2], table[id][3]};
  }
};

// The host's side of a bank: the checks every bank entry point makes before a launch, and the kernel argument.  `table` is HOST
// memory, (P,4) ints.  false: P outside 1 .. kMaxBankMembers, no data or table, ids missing for n > 0 slices, a negative offset or a
// member with a size below 1.
// max_elements: the largest member's d_p h_p w_p.
template <typename T>
inline bool make_bank(const T* data, const int* table, int P, const int* ids, int n, BankPsf<T>& out, int64_t& max_elements) {
  if (P < 1 || P > kMaxBankMembers || data == nullptr || table == nullptr || (ids == nullptr && n > 0)) return false;
  out.data = data;
  out.ids = ids;
  out.P = P;
  max_elements = 0;
  for (int p = 0; p < kMaxBankMembers; ++p)
    for (int j = 0; j < 4; ++j) out.table[p][j] = p < P ? table[4 * p + j] : 0;
  for (int p = 0; p < P; ++p) {
    if (out.table[p][0] < 0 || out.table[p][1] < 1 || out.table[p][2] < 1 || out.table[p][3] < 1) return false;
    const int64_t e = (int64_t)out.table[p][1] * out.table[p][2] * out.table[p][3];
    if (e > max_elements) max_elements = e;
  }
  return true;
}

// The tap-list prologue of a workgroup that serves slice k: thread 0 compacts the slice's PSF into `taps` and publishes the count -
// 0, with nothing indexed by k, for a workgroup that is not `live`.  Every thread calls; the caller places the barrier.
template <typename T, typename PSF>
__device__ __forceinline__ void workgroup_taps(const PSF& psfs, bool live, int k, Tap<T>* taps, int& n_taps) {
  if (threadIdx.x == 0) {
    int cnt = 0;
    if (live) {
      const PsfView<T> pk = psfs.at(k);
      cnt = compact_taps(pk.psf, pk.d, pk.h, pk.w, taps);
    }
    n_taps = cnt;
  }
}

// The host's side of a kernel with an LDS tap list: its PSF source as the kernel argument, behind the checks every such entry point
// makes - every PSF fits the list (kMaxTaps elements, ANY bank member) and the volume's voxel indices fit an int.  false: refused.
// The two forms of an entry point differ in when they ask: the one-PSF form returns its no-op (nothing to do: 0) BEFORE it looks at
// the PSF, the bank form checks the bank and the volume first and a bad bank is refused even where nothing would be launched.
template <typename T> inline bool lds_one_psf(const T* psf, int d_p, int h_p, int w_p, int D, int H, int W, OnePsf<T>& out) {
  if (d_p < 1 || h_p < 1 || w_p < 1 || (int64_t)d_p * h_p * w_p > kMaxTaps || (int64_t)D * H * W > INT_MAX) return false;
  out = OnePsf<T>{psf, d_p, h_p, w_p};
  return true;
}
template <typename T>
inline bool lds_bank_psf(const T* data, const int* table, int P, const int* ids, int n, int D, int H, int W, BankPsf<T>& out) {
  int64_t max_elements;
  return make_bank(data, table, P, ids, n, out, max_elements) && max_elements <= kMaxTaps && (int64_t)D * H * W <= INT_MAX;
}

template <typename T> struct PixelGeom { T qx, qy, qz, xc, yc, zc; };

template <typename T>
__device__ __forceinline__ PixelGeom<T> pixel_geom(const T* t, int ix, int iy, int h, int w, T res_slice, int D, int H, int W) {
  PixelGeom<T> g;
  g.qx = (T)((ix - (w - 1) / 2.) * (double)res_slice + (double)t[3]);
  g.qy = (T)((iy - (h - 1) / 2.) * (double)res_slice + (double)t[7]);
  g.qz = t[11];
  g.xc = t[0] * g.qx + t[1] * g.qy + t[2] * g.qz + (W - 1) / (T)2.0;
  g.yc = t[4] * g.qx + t[5] * g.qy + t[6] * g.qz + (H - 1) / (T)2.0;
  g.zc = t[8] * g.qx + t[9] * g.qy + t[10] * g.qz + (D - 1) / (T)2.0;
  return g;
}

// Tap (ox, oy, oz) of the pixel: its position, and whether it lies inside the volume (false for a NaN coordinate).
template <typename T>
__device__ __forceinline__ bool tap_position(const T* t, const PixelGeom<T>& g, T ox, T oy, T oz, int D, int H, int W, T& x, T& y, T& z) {
  x = g.xc + t[0] * ox + t[1] * oy + t[2] * oz;
  y = g.yc + t[4] * ox + t[5] * oy + t[6] * oz;
  z = g.zc + t[8] * ox + t[9] * oy + t[10] * oz;
  return x >= 0 && y >= 0 && z >= 0 && x < W - 1 && y < H - 1 && z < D - 1;
}

// The NaN rule hoisted out of a tap loop, once per slice: true iff no tap of any pixel of the slice can have a NaN coordinate, so
// that the loop may test `x < 0 || ... || z >= D - 1` alone (which a NaN would pass).  With the twelve pose entries at most 1e18
// and the pixel size at most 1e8 in magnitude, q (|pixel index| < 2^31) stays below 2e18, c = R q + centre and every product
// R o (integer offsets, |o| < 2^31) below 1e37: p = c + R o is a sum of finite terms, finite or one infinity, never NaN, and an
// infinite coordinate fails the plain test.  False for a NaN entry (the comparisons are ordered).  Uniform over the slice.
template <typename T> __device__ __forceinline__ bool pose_is_bounded(const T* t, T res_slice) {
  bool ok = fabs(res_slice) <= (T)1e8;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && fabs(t[i]) <= (T)1e18;
  return ok;
}

// body(ox, oy, oz, pv, x, y, z) for every non-zero PSF tap inside the volume, in ip order: the tap's integer offsets (as T), its
// PSF value and its position.
template <typename T, typename Body>
__device__ __forceinline__ void for_psf_taps(const T* t, const PixelGeom<T>& g, const T* __restrict__ psf, int d_p, int h_p, int w_p,
                                             int D, int H, int W, Body body) {
  int ip = 0;
  for (int iz = -d_p / 2; iz < (d_p + 1) / 2; ++iz)
    for (int iy = -h_p / 2; iy < (h_p + 1) / 2; ++iy)
      for (int ix = -w_p / 2; ix < (w_p + 1) / 2; ++ix, ++ip) {
        const T pv = psf[ip], ox = (T)ix, oy = (T)iy, oz = (T)iz;
        if (pv == (T)0.0) continue;
        T x, y, z;
        if (tap_position(t, g, ox, oy, oz, D, H, W, x, y, z)) body(ox, oy, oz, pv, x, y, z);
      }
}

// The same walk over the list compact_taps made.
template <typename T, typename Body>
__device__ __forceinline__ void for_lds_taps(const T* t, const PixelGeom<T>& g, const Tap<T>* taps, int n_taps, int D, int H, int W,
                                             Body body) {
  for (int k = 0; k < n_taps; ++k) {
    const Tap<T> tp = taps[k];
    T x, y, z;
    if (tap_position(t, g, tp.x, tp.y, tp.z, D, H, W, x, y, z)) body(tp.x, tp.y, tp.z, tp.w, x, y, z);
  }
}

// The trilinear cell of a position inside the volume: its low corner's voxel index (an int: the host refuses larger volumes), the
// fractions and the strides.
template <typename T> struct Cell { int i0, Sy, Sz; T wx, wy, wz; };

template <typename T> __device__ __forceinline__ Cell<T> trilinear_cell(T x, T y, T z, int H, int W) {
  const int xf = (int)floor(x), yf = (int)floor(y), zf = (int)floor(z);
  const int Sy = W, Sz = H * W;
  return Cell<T>{zf * Sz + yf * Sy + xf, Sy, Sz, x - xf, y - yf, z - zf};
}

// One tap of the forward operator: val += pw v, wsum += pw over the cell's corners on the mask (vol_mask may be null), pw =
// corner weight * pv.
template <typename T>
__device__ __forceinline__ void linear_tap(const T* __restrict__ vol, const uint8_t* __restrict__ vol_mask, const Cell<T>& c, T pv,
                                           T& val, T& wsum) {
  const T wx = c.wx, wy = c.wy, wz = c.wz;
  // corner order as the reference accumulates: 000,100,010,001,110,101,011,111
  const int off[8] = {0, 1, c.Sy, c.Sz, 1 + c.Sy, 1 + c.Sz, c.Sy + c.Sz, 1 + c.Sy + c.Sz};
  const T cw[8] = {(1 - wx) * (1 - wy) * (1 - wz), wx * (1 - wy) * (1 - wz), (1 - wx) * wy * (1 - wz),
                   (1 - wx) * (1 - wy) * wz,       wx * wy * (1 - wz),       wx * (1 - wy) * wz,
                   (1 - wx) * wy * wz,             wx * wy * wz};
  T v8[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v8[k] = vol[c.i0 + off[k]];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (vol_mask == nullptr || vol_mask[c.i0 + off[k]]) {
      const T pw = cw[k] * pv;
      val += pw * v8[k];
      wsum += pw;
    }
  }
}

// The pixel (ix, iy) of A<T> under pose t from an LDS tap list, linear mode, no volume mask: the value I = val / wsum and true iff
// the PSF weight wsum > 0 (I untouched otherwise).  The functions, the order and the division are those of slice_acq_fwd<T, false,
// true> (slice_acq.hip, which keeps its own statement: it carries the volume mask and the dense walk), so value and valid set are
// that operator's bit for bit; every svr statistic takes its pixel from here.
template <typename T>
__device__ __forceinline__ bool simulate_pixel(const T* __restrict__ vol, int D, int H, int W, const T* t, int ix, int iy, int h, int w,
                                               T res_slice, const Tap<T>* taps, int nt, T& I) {
  const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
  T val = 0, wsum = 0;
  for_lds_taps(t, g, taps, nt, D, H, W, [&](T, T, T, T pv, T x, T y, T z) {
    linear_tap(vol, (const uint8_t*)nullptr, trilinear_cell(x, y, z, H, W), pv, val, wsum);
  });
  if (!(wsum > 0)) return false;
  I = val / wsum;
  return true;
}

// Corner k = 0 .. 7 of a cell by bits (x lowest): its voxel index and per-axis weights; add_corner_gradient adds the corner's share
// of d / d (x, y, z) of sum_corners s * trilinear weight.
template <typename T> struct Corner { int ic, cx, cy, cz; T ax, ay, az; };

template <typename T> __device__ __forceinline__ Corner<T> cell_corner(const Cell<T>& c, int k) {
  const int cx = k & 1, cy = (k >> 1) & 1, cz = k >> 2;
  return Corner<T>{c.i0 + cx + cy * c.Sy + cz * c.Sz, cx, cy, cz, cx ? c.wx : (T)1.0 - c.wx, cy ? c.wy : (T)1.0 - c.wy,
                   cz ? c.wz : (T)1.0 - c.wz};
}

template <typename T> __device__ __forceinline__ void add_corner_gradient(const Corner<T>& n, T s, T& dx, T& dy, T& dz) {
  dx += (n.cx ? s : -s) * n.ay * n.az;
  dy += (n.cy ? s : -s) * n.ax * n.az;
  dz += (n.cz ? s : -s) * n.ax * n.ay;
}

// The 12 entries of d / d [R | t] from d / d p of one tap: p = R (q + o) + centre.
template <typename T>
__device__ __forceinline__ void accumulate_pose_grad(T (&g)[12], const T* t, const PixelGeom<T>& pg, T tx, T ty, T tz, T dx,
                                                     T dy, T dz) {
  const T ox = pg.qx + tx, oy = pg.qy + ty, oz = pg.qz + tz;
  g[0] += dx * ox; g[1] += dx * oy; g[2] += dx * oz;
  g[4] += dy * ox; g[5] += dy * oy; g[6] += dy * oz;
  g[8] += dz * ox; g[9] += dz * oy; g[10] += dz * oz;
  g[3] += dx * t[0] + dy * t[4] + dz * t[8];
  g[7] += dx * t[1] + dy * t[5] + dz * t[9];
  g[11] += dx * t[2] + dy * t[6] + dz * t[10];
}

// The 12 pose sums of a slice over its 256-thread workgroup -> out[12].  Every thread must call (barrier).
template <typename T> __device__ __forceinline__ void reduce_pose_grad(const T (&g)[12], T* __restrict__ out) {
  __shared__ T red[4][12];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const T s = wave_sum(g[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 12) out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

}  // namespace acq
}  // namespace
