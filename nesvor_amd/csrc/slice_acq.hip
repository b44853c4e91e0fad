// Slice acquisition forward operator A for gfx950: volume -> PSF-blurred slices.
//
// Behavioural spec: `slice_acquisition_forward_cuda_kernel`
// (nesvor/slice_acquisition/slice_acq_cuda_kernel.cu:17-171).  Gather-only.
// One thread per slice pixel.  The PSF is compacted once per workgroup into an
// LDS list of its non-zero taps (offset + weight, original order preserved so
// the fp32 accumulation order matches the reference), which removes the
// zero-tap branches from the inner loop; the per-slice rotation is read through
// the scalar path.  Volume reads are 8 scattered dwords per tap and stay in
// L2/Infinity Cache for phantom-sized volumes (128^3 fp32 = 8 MB).
// The pixel geometry, the tap walks, the inside test and the per-tap arithmetic of the kernels here are acq_taps.h's
// (slice_acq_adjoint_gather and slice_acq_adjoint_bwd keep theirs written out and say why).
#include <hip/hip_runtime.h>
#include "acq_taps.h"

namespace {
using namespace acq;

template <typename T> struct InterpTap { int iv, xr, yr, zr; T pw, gx, gy, gz; };

// One PSF tap at (x, y, z) already known to lie inside the volume.  false: the rounded voxel's offset falls outside the
// PSF support.  GRAD: also d pw / d (x_psf, y_psf, z_psf), the corner sums of the reference (.cu:311-352).
template <typename T, bool GRAD>
__device__ __forceinline__ bool interp_tap(const T* __restrict__ t, const PixelGeom<T>& g, const T* __restrict__ psf, int d_p,
                                           int h_p, int w_p, T x, T y, T z, int Sy, int Sz, InterpTap<T>& o) {
  o.xr = (int)floor(x + (T)0.5); o.yr = (int)floor(y + (T)0.5); o.zr = (int)floor(z + (T)0.5);
  o.iv = o.zr * Sz + o.yr * Sy + o.xr;
  const T dx = o.xr - g.xc, dy = o.yr - g.yc, dz = o.zr - g.zc;
  const T xp = t[0] * dx + t[4] * dy + t[8] * dz + (w_p - 1) / (T)2.0;
  const T yp = t[1] * dx + t[5] * dy + t[9] * dz + (h_p - 1) / (T)2.0;
  const T zp = t[2] * dx + t[6] * dy + t[10] * dz + (d_p - 1) / (T)2.0;
  if (xp < 0 || yp < 0 || zp < 0 || xp >= w_p - 1 || yp >= h_p - 1 || zp >= d_p - 1) return false;
  const int xf = (int)floor(xp), yf = (int)floor(yp), zf = (int)floor(zp);
  const T wx = xp - xf, wy = yp - yf, wz = zp - zf;
  const T* p0 = psf + (zf * h_p + yf) * w_p + xf;
  const int py = w_p, pz = w_p * h_p;
  const T c000 = p0[0], c100 = p0[1], c010 = p0[py], c001 = p0[pz], c110 = p0[1 + py], c101 = p0[1 + pz], c011 = p0[py + pz],
          c111 = p0[1 + py + pz];
  T pw = (T)0.0;  // corner order of the reference: 000, 100, 010, 001, 110, 101, 011, 111
  pw += (1 - wx) * (1 - wy) * (1 - wz) * c000;
  pw += wx * (1 - wy) * (1 - wz) * c100;
  pw += (1 - wx) * wy * (1 - wz) * c010;
  pw += (1 - wx) * (1 - wy) * wz * c001;
  pw += wx * wy * (1 - wz) * c110;
  pw += wx * (1 - wy) * wz * c101;
  pw += (1 - wx) * wy * wz * c011;
  pw += wx * wy * wz * c111;
  o.pw = pw;
  if constexpr (GRAD) {
    T gx = (T)0.0, gy = (T)0.0, gz = (T)0.0;
    gx -= (1 - wy) * (1 - wz) * c000; gy -= (1 - wx) * (1 - wz) * c000; gz -= (1 - wx) * (1 - wy) * c000;
    gx += (1 - wy) * (1 - wz) * c100; gy -= wx * (1 - wz) * c100;       gz -= wx * (1 - wy) * c100;
    gx -= wy * (1 - wz) * c010;       gy += (1 - wx) * (1 - wz) * c010; gz -= (1 - wx) * wy * c010;
    gx -= (1 - wy) * wz * c001;       gy -= (1 - wx) * wz * c001;       gz += (1 - wx) * (1 - wy) * c001;
    gx += wy * (1 - wz) * c110;       gy += wx * (1 - wz) * c110;       gz -= wx * wy * c110;
    gx += (1 - wy) * wz * c101;       gy -= wx * wz * c101;             gz += wx * (1 - wy) * c101;
    gx -= wy * wz * c011;             gy += (1 - wx) * wz * c011;       gz += (1 - wx) * wy * c011;
    gx += wy * wz * c111;             gy += wx * wz * c111;             gz += wx * wy * c111;
    o.gx = gx; o.gy = gy; o.gz = gz;
  }
  return true;
}

// LDS_TAPS: the PSF's non-zero taps fit the LDS list (every PSF get_PSF builds for clinical geometries: (9,5,5) = 153
// taps for 1.5 x 1.5 x 3 mm slices on a 1 mm grid); larger PSFs (thick slices on a fine grid, e.g. 6 mm on 0.5 mm = 1813
// taps) walk the dense PSF array in global memory instead - same arithmetic, same order.
template <typename T, bool INTERP_PSF, bool LDS_TAPS>
__global__ __launch_bounds__(256) void slice_acq_fwd(
    const T* __restrict__ transforms, const T* __restrict__ vol, const uint8_t* __restrict__ vol_mask,
    const uint8_t* __restrict__ slices_mask, const T* __restrict__ psf, T* __restrict__ slices,
    T* __restrict__ slices_weight, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
    T res_slice) {
  __shared__ Tap<T> taps[LDS_TAPS ? kMaxTaps : 1];
  __shared__ int n_taps;
  if constexpr (LDS_TAPS) {
    if (threadIdx.x == 0) n_taps = compact_taps(psf, d_p, h_p, w_p, taps);
    __syncthreads();
  }
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * h * w) return;
  if (slices_mask != nullptr && !slices_mask[idx]) return;
  const int ix = idx % w, iy = (idx / w) % h, in = idx / ((int64_t)h * w);
  const T* t = transforms + (size_t)in * 12;
  const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
  T val = (T)0.0, wsum = (T)0.0;
  auto tap = [&](T, T, T, T pv, T x, T y, T z) {
    if constexpr (INTERP_PSF) {
      // nearest voxel, PSF re-interpolated at the voxel's offset from the centre
      InterpTap<T> o;
      if (!interp_tap<T, false>(t, g, psf, d_p, h_p, w_p, x, y, z, W, H * W, o)) return;
      if (vol_mask != nullptr && !vol_mask[o.iv]) return;
      val += o.pw * vol[o.iv];
      wsum += o.pw;
    } else {
      linear_tap(vol, vol_mask, trilinear_cell(x, y, z, H, W), pv, val, wsum);
    }
  };
  if constexpr (LDS_TAPS) for_lds_taps(t, g, taps, n_taps, D, H, W, tap);
  else for_psf_taps(t, g, psf, d_p, h_p, w_p, D, H, W, tap);
  if (wsum > 0) {
    slices[idx] = val / wsum;
    if (slices_weight != nullptr) slices_weight[idx] = wsum;
  }
}

// A with a PSF bank (fp32, linear mode): slice k is blurred by PSF ids[k].  One workgroup serves pixels of ONE slice (grid:
// n * wgs, wgs = ceil(h w / 256), as svr_similarity_kernel), so the PSF, its sizes and the choice between the LDS list and the
// dense walk (a member of more than kMaxTaps elements) are uniform over the workgroup.  Per pixel the arithmetic is slice_acq_fwd's.
__global__ __launch_bounds__(256) void slice_acq_fwd_bank(const float* __restrict__ transforms, const float* __restrict__ vol,
                                                          const uint8_t* __restrict__ vol_mask, const uint8_t* __restrict__ slices_mask,
                                                          const BankPsf<float> psfs, float* __restrict__ slices,
                                                          float* __restrict__ slices_weight, int D, int H, int W, int h, int w, int wgs,
                                                          float res_slice) {
  __shared__ Tap<float> taps[kMaxTaps];
  __shared__ int n_taps;
  const int in = blockIdx.x / wgs, wg = blockIdx.x - in * wgs;
  const PsfView<float> pk = psfs.at(in);
  const bool lds = (int64_t)pk.d * pk.h * pk.w <= kMaxTaps;
  if (lds) {
    if (threadIdx.x == 0) n_taps = compact_taps(pk.psf, pk.d, pk.h, pk.w, taps);
    __syncthreads();
  }
  const int pix = wg * 256 + (int)threadIdx.x;
  if (pix >= h * w) return;
  const size_t idx = (size_t)in * h * w + pix;
  if (slices_mask != nullptr && !slices_mask[idx]) return;
  const int ix = pix % w, iy = pix / w;
  const float* t = transforms + (size_t)in * 12;
  const PixelGeom<float> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
  float val = 0.f, wsum = 0.f;
  auto tap = [&](float, float, float, float pv, float x, float y, float z) {
    linear_tap(vol, vol_mask, trilinear_cell(x, y, z, H, W), pv, val, wsum);
  };
  if (lds) for_lds_taps(t, g, taps, n_taps, D, H, W, tap);
  else for_psf_taps(t, g, pk.psf, pk.d, pk.h, pk.w, D, H, W, tap);
  if (wsum > 0) {
    slices[idx] = val / wsum;
    if (slices_weight != nullptr) slices_weight[idx] = wsum;
  }
}

// ------------------------------------------------------------------ adjoint A^T and backward of A
// The reference scatters every (pixel, PSF tap) into 8 voxels with atomicAdd
// (slice_acq_cuda_kernel.cu:173-470 backward, :472-670 adjoint).  On MI355X global atomics execute
// memory-side (~16 G/s): one adjoint of 3 stacks of 77 x 151^2 pixels would be 13 G atomics.  Both
// operators are therefore evaluated as a GATHER OVER VOXELS: a voxel collects, slice by slice, the
// samples p = R (q_pixel + tap) + c0 that have it as one of their 8 trilinear corners
// (-1 <= p - v < 1 per axis).  In the slice frame that is the small box |q + tap - R^T (v - c0)| < sqrt 3,
// so per slice only ~6 x 6 pixels x <= 4^3 taps are visited.  No atomics, each voxel written once.
//   pass 1 (per pixel): PSF weight = sum of the taps inside the volume; coef = value / weight under the
//                       operator's activity rule (adjoint: weight >= 0.5; backward: grad != 0, weight != 0)
//   pass 2 (per voxel): vol[v] = sum coef * psf[tap] * trilinear(p - v)   [+ the same sum with 1/weight]
//   backward only     : grad_transforms by one workgroup per slice (block reduction, no atomics)
template <typename T> __device__ __forceinline__ constexpr T sqrt3() { return (T)1.7320508075688772; }

// mode 0: adjoint (value = slices, active iff weight >= 0.5); mode 1: backward (value = grad_slices,
// active iff value != 0 and weight != 0).  coef[idx] = value / weight, cw[idx] = 1 / weight (0 if inactive).
template <typename T>
__global__ __launch_bounds__(256) void slice_acq_pixel_coef(const T* __restrict__ transforms, const T* __restrict__ psf,
                                                            const T* __restrict__ value, const uint8_t* __restrict__ slices_mask,
                                                            T* __restrict__ coef, T* __restrict__ cw, int D, int H, int W,
                                                            int d_p, int h_p, int w_p, int n, int h, int w, T res_slice, int mode) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * h * w) return;
  T c = (T)0.0, iw = (T)0.0;
  const T val = value[idx];
  const bool on = (slices_mask == nullptr || slices_mask[idx]) && (mode == 0 || val != (T)0.0);
  if (on) {
    const int ix = idx % w, iy = (idx / w) % h, in = idx / ((int64_t)h * w);
    const T* t = transforms + (size_t)in * 12;
    const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
    T weight = (T)0.0;
    for_psf_taps(t, g, psf, d_p, h_p, w_p, D, H, W, [&](T, T, T, T pv, T, T, T) { weight += pv; });
    const bool active = mode == 0 ? weight >= (T)0.5 : weight != (T)0.0;
    if (active) { c = val / weight; iw = (T)1.0 / weight; }
  }
  coef[idx] = c;
  if (cw != nullptr) cw[idx] = iw;
}

// Pass 1 of A^T with a PSF bank (mode 0 of slice_acq_pixel_coef): the weight sum of a pixel runs over its slice's PSF.  Grid as
// slice_acq_fwd_bank: the workgroup's slice, hence its PSF, is uniform.
__global__ __launch_bounds__(256) void slice_acq_pixel_coef_bank(const float* __restrict__ transforms, const BankPsf<float> psfs,
                                                                 const float* __restrict__ value, const uint8_t* __restrict__ slices_mask,
                                                                 float* __restrict__ coef, float* __restrict__ cw, int D, int H, int W,
                                                                 int h, int w, int wgs, float res_slice) {
  const int in = blockIdx.x / wgs, wg = blockIdx.x - in * wgs;
  const int pix = wg * 256 + (int)threadIdx.x;
  if (pix >= h * w) return;
  const PsfView<float> pk = psfs.at(in);
  const size_t idx = (size_t)in * h * w + pix;
  float c = 0.f, iw = 0.f;
  if (slices_mask == nullptr || slices_mask[idx]) {
    const float* t = transforms + (size_t)in * 12;
    const PixelGeom<float> g = pixel_geom(t, pix % w, pix / w, h, w, res_slice, D, H, W);
    float weight = 0.f;
    for_psf_taps(t, g, pk.psf, pk.d, pk.h, pk.w, D, H, W, [&](float, float, float, float pv, float, float, float) { weight += pv; });
    if (weight >= 0.5f) { c = value[idx] / weight; iw = 1.f / weight; }
  }
  coef[idx] = c;
  cw[idx] = iw;
}

// PSF: OnePsf<T>, or BankPsf<T> - slice k then takes its own PSF and, with it, its own tap ranges tz0 .. tx1 in the box bounds.
template <typename T, typename PSF>
__global__ __launch_bounds__(256) void slice_acq_adjoint_gather(const T* __restrict__ transforms, const PSF psfs,
                                                                const T* __restrict__ coef, const T* __restrict__ cw,
                                                                const uint8_t* __restrict__ vol_mask, T* __restrict__ vol,
                                                                T* __restrict__ vol_weight, int D, int H, int W, int n, int h, int w,
                                                                T res_slice, int equalize, int accumulate) {
  const int64_t iv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (iv >= (int64_t)D * H * W) return;
  const int vx = iv % W, vy = (iv / W) % H, vz = iv / ((int64_t)H * W);
  T acc = (T)0.0, accw = (T)0.0;
  if (vol_mask == nullptr || vol_mask[iv]) {
    const T d0 = vx - (W - 1) / (T)2.0, d1 = vy - (H - 1) / (T)2.0, d2 = vz - (D - 1) / (T)2.0;
    for (int k = 0; k < n; ++k) {
      const PsfView<T> pk = psfs.at(k);  // (uniform over the launch; loop-invariant for OnePsf)
      const T* __restrict__ psf = pk.psf;
      const int d_p = pk.d, h_p = pk.h, w_p = pk.w;
      const int tz0 = -d_p / 2, tz1 = (d_p + 1) / 2 - 1, ty0 = -h_p / 2, ty1 = (h_p + 1) / 2 - 1, tx0 = -w_p / 2, tx1 = (w_p + 1) / 2 - 1;
      const T* t = transforms + (size_t)k * 12;
      // voxel in the slice frame: r = R^T (v - c0)
      const T rz = t[2] * d0 + t[6] * d1 + t[10] * d2;
      const T ez = rz - t[11];
      const int izlo = max(tz0, (int)ceil(ez - sqrt3<T>())), izhi = min(tz1, (int)floor(ez + sqrt3<T>()));
      if (izlo > izhi) continue;
      const T rx = t[0] * d0 + t[4] * d1 + t[8] * d2, ry = t[1] * d0 + t[5] * d1 + t[9] * d2;
      const int ixlo = max(0, (int)ceil((rx - t[3] - sqrt3<T>() - tx1) / res_slice + (w - 1) / (T)2.0));
      const int ixhi = min(w - 1, (int)floor((rx - t[3] + sqrt3<T>() - tx0) / res_slice + (w - 1) / (T)2.0));
      const int iylo = max(0, (int)ceil((ry - t[7] - sqrt3<T>() - ty1) / res_slice + (h - 1) / (T)2.0));
      const int iyhi = min(h - 1, (int)floor((ry - t[7] + sqrt3<T>() - ty0) / res_slice + (h - 1) / (T)2.0));
      for (int iy = iylo; iy <= iyhi; ++iy)
        for (int ix = ixlo; ix <= ixhi; ++ix) {
          const size_t pidx = ((size_t)k * h + iy) * w + ix;
          const T cf = coef[pidx];
          const T cwv = cw != nullptr ? cw[pidx] : (T)0.0;
          if (cf == (T)0.0 && cwv == (T)0.0) continue;
          const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
          const int jxlo = max(tx0, (int)ceil(rx - g.qx - sqrt3<T>())), jxhi = min(tx1, (int)floor(rx - g.qx + sqrt3<T>()));
          const int jylo = max(ty0, (int)ceil(ry - g.qy - sqrt3<T>())), jyhi = min(ty1, (int)floor(ry - g.qy + sqrt3<T>()));
          for (int iz = izlo; iz <= izhi; ++iz)
            for (int jy = jylo; jy <= jyhi; ++jy)
              for (int jx = jxlo; jx <= jxhi; ++jx) {
                const T pv = psf[((iz - tz0) * h_p + (jy - ty0)) * w_p + (jx - tx0)];
                if (pv == (T)0.0) continue;
                // (position and test written out, not tap_position: a position only weighs a sum here, it indexes nothing, and
                //  the NaN-safe form of the test costs this innermost loop 6 % of the adjoint's time)
                const T x = g.xc + t[0] * jx + t[1] * jy + t[2] * iz;
                const T y = g.yc + t[4] * jx + t[5] * jy + t[6] * iz;
                const T z = g.zc + t[8] * jx + t[9] * jy + t[10] * iz;
                if (x < 0 || y < 0 || z < 0 || x >= W - 1 || y >= H - 1 || z >= D - 1) continue;
                const T ex = x - vx, ey = y - vy, ezz = z - vz;
                if (ex < -(T)1.0 || ex >= (T)1.0 || ey < -(T)1.0 || ey >= (T)1.0 || ezz < -(T)1.0 || ezz >= (T)1.0) continue;
                // the voxel must be floor(p) or floor(p) + 1 on every axis, with the scatter's weights
                const T wx = ex >= (T)0.0 ? (T)1.0 - ex : (T)1.0 + ex, wy = ey >= (T)0.0 ? (T)1.0 - ey : (T)1.0 + ey, wz = ezz >= (T)0.0 ? (T)1.0 - ezz : (T)1.0 + ezz;
                const T wgt = wx * wy * wz * pv;
                acc += wgt * cf;
                accw += wgt * cwv;
              }
        }
    }
  }
  if (equalize && accw > (T)0.0) acc /= accw;
  if (accumulate) vol[iv] += acc; else vol[iv] = acc;
  if (vol_weight != nullptr) vol_weight[iv] = accw;
}

// d L / d transforms of the forward operator: one workgroup per slice, block reduction of 12 sums.
template <typename T>
__global__ __launch_bounds__(256) void slice_acq_bwd_transforms(const T* __restrict__ transforms, const T* __restrict__ vol,
                                                                const uint8_t* __restrict__ vol_mask, const T* __restrict__ psf,
                                                                const T* __restrict__ coef, T* __restrict__ grad_transforms,
                                                                int D, int H, int W, int d_p, int h_p, int w_p, int h, int w,
                                                                T res_slice) {
  const int k = blockIdx.x;
  const T* t = transforms + (size_t)k * 12;
  T g[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) g[i] = (T)0.0;
  for (int pix = threadIdx.x; pix < h * w; pix += blockDim.x) {
    const T gs = coef[(size_t)k * h * w + pix];
    if (gs == (T)0.0) continue;
    const int ix = pix % w, iy = pix / w;
    const PixelGeom<T> pg = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
    for_psf_taps(t, pg, psf, d_p, h_p, w_p, D, H, W, [&](T tx, T ty, T tz, T pv, T x, T y, T z) {
      const T pgs = pv * gs;
      const Cell<T> cell = trilinear_cell(x, y, z, H, W);
      T dx = (T)0.0, dy = (T)0.0, dz = (T)0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const Corner<T> cn = cell_corner(cell, c);
        if (vol_mask != nullptr && !vol_mask[cn.ic]) continue;
        add_corner_gradient(cn, pgs * vol[cn.ic], dx, dy, dz);
      }
      accumulate_pose_grad(g, t, pg, tx, ty, tz, dx, dy, dz);
    });
  }
  reduce_pose_grad(g, grad_transforms + (size_t)k * 12);
}

// in-place "equalise a gradient" step of adjoint_backward (slice_acq_cuda_kernel.cu:672-693 with is_grad = true)
template <typename T>
__global__ void slice_acq_equalize_grad(T* __restrict__ grad_vol, const T* __restrict__ vol_weight, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T wgt = vol_weight[i];
  if (wgt > (T)0.0) grad_vol[i] /= (wgt < (T)1e-3 ? (T)1e-3 : wgt);
}

// Backward of A^T (slice_acq_cuda_kernel.cu:695-950, linear mode): a gather per slice pixel,
//   grad_slices[p] = sum_taps psf * trilinear(grad_vol) / sum_taps psf            (taps inside the volume)
//   grad_transforms[k] += d/dT of the same expression with the corner values weighted by
//                         (slices[p] - vol[corner]) (equalised adjoint) or slices[p].
// One workgroup per slice; the 12 pose sums are block-reduced (the reference adds them with atomics).
// The tap walk, the corner loop and the pose accumulation stay written out here (the twins of for_psf_taps, cell_corner /
// add_corner_gradient and accumulate_pose_grad in acq_taps.h, with that header's NaN rule in its hoisted form): routed through the helpers this
// kernel's fp32 allocation came out at 82 registers, one occupancy step down, and held at 78 by launch bounds it ran 5 % slower.
template <typename T>
__global__ __launch_bounds__(256) void slice_acq_adjoint_bwd(const T* __restrict__ transforms, const T* __restrict__ grad_vol,
                                                             const T* __restrict__ psf, const T* __restrict__ slices,
                                                             const uint8_t* __restrict__ slices_mask, const T* __restrict__ vol,
                                                             const uint8_t* __restrict__ vol_mask, T* __restrict__ grad_slices,
                                                             T* __restrict__ grad_transforms, int D, int H, int W, int d_p,
                                                             int h_p, int w_p, int h, int w, T res_slice) {
  const int k = blockIdx.x;
  const T* t = transforms + (size_t)k * 12;
  const int Sy = W, Sz = H * W;
  const int n_pix = pose_is_bounded(t, res_slice) ? h * w : 0;  // a non-finite pose: no pixel walks its taps, so that the plain test below suffices
  T g[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) g[i] = (T)0.0;
  for (int pix = threadIdx.x; pix < n_pix; pix += blockDim.x) {
    const size_t idx = (size_t)k * h * w + pix;
    if (slices_mask != nullptr && !slices_mask[idx]) continue;
    const int ix = pix % w, iy = pix / w;
    const PixelGeom<T> pg = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
    const T sv = slices[idx];
    T val = (T)0.0, weight = (T)0.0;
    T gp[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) gp[i] = (T)0.0;
    int ip = 0;
    for (int iz = -d_p / 2; iz < (d_p + 1) / 2; ++iz)
      for (int iyp = -h_p / 2; iyp < (h_p + 1) / 2; ++iyp)
        for (int ixp = -w_p / 2; ixp < (w_p + 1) / 2; ++ixp, ++ip) {
          const T pv = psf[ip];
          if (pv == (T)0.0) continue;
          const T x = pg.xc + t[0] * ixp + t[1] * iyp + t[2] * iz;
          const T y = pg.yc + t[4] * ixp + t[5] * iyp + t[6] * iz;
          const T z = pg.zc + t[8] * ixp + t[9] * iyp + t[10] * iz;
          if (x < 0 || y < 0 || z < 0 || x >= W - 1 || y >= H - 1 || z >= D - 1) continue;
          const int xf = (int)floor(x), yf = (int)floor(y), zf = (int)floor(z);
          const T wx = x - xf, wy = y - yf, wz = z - zf;
          const int i0 = zf * Sz + yf * Sy + xf;
          T v_ = (T)0.0, dx = (T)0.0, dy = (T)0.0, dz = (T)0.0;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
            const int ic = i0 + cx + cy * Sy + cz * Sz;
            if (vol_mask != nullptr && !vol_mask[ic]) continue;
            const T gv = grad_vol[ic];
            const T ax = cx ? wx : (T)1.0 - wx, ay = cy ? wy : (T)1.0 - wy, az = cz ? wz : (T)1.0 - wz;
            v_ += ax * ay * az * gv;
            const T s = (vol == nullptr ? sv : sv - vol[ic]) * gv;
            dx += (cx ? s : -s) * ay * az;
            dy += (cy ? s : -s) * ax * az;
            dz += (cz ? s : -s) * ax * ay;
          }
          val += pv * v_;
          weight += pv;
          dx *= pv; dy *= pv; dz *= pv;
          const T ox = pg.qx + ixp, oy = pg.qy + iyp, oz = pg.qz + iz;
          gp[0] += dx * ox; gp[1] += dx * oy; gp[2] += dx * oz;
          gp[4] += dy * ox; gp[5] += dy * oy; gp[6] += dy * oz;
          gp[8] += dz * ox; gp[9] += dz * oy; gp[10] += dz * oz;
          gp[3] += dx * t[0] + dy * t[4] + dz * t[8];
          gp[7] += dx * t[1] + dy * t[5] + dz * t[9];
          gp[11] += dx * t[2] + dy * t[6] + dz * t[10];
        }
    if (weight > (T)0.0) {
      if (grad_slices != nullptr) grad_slices[idx] = val / weight;
#pragma unroll
      for (int i = 0; i < 12; ++i) g[i] += gp[i] / weight;
    }
  }
  if (grad_transforms != nullptr) reduce_pose_grad(g, grad_transforms + (size_t)k * 12);
}

// The kernels above index voxels with int (zf * Sz + yf * Sy + xf): every entry point refuses a larger volume before a launch.
inline bool volume_too_large(int D, int H, int W) { return (int64_t)D * H * W > (int64_t)INT_MAX; }

// A gradient of an empty stack (no launch writes it) is zero, not whatever its buffer held.
template <typename T> int zero_fill(T* p, int64_t count, hipStream_t st) {
  if (p == nullptr || count <= 0) return 0;
  return (int)hipMemsetAsync(p, 0, sizeof(T) * (size_t)count, st);
}

template <typename T>
int slice_acq_adjoint_backward_impl(const T* transforms, T* grad_vol, const T* vol_weight,
                                                 const uint8_t* vol_mask, const T* psf, const T* slices,
                                                 const uint8_t* slices_mask, const T* vol, T* grad_slices,
                                                 T* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p,
                                                 int n, int h, int w, T res_slice, int equalize, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if ((int64_t)n * h * w <= 0) return zero_fill(grad_transforms, (int64_t)n * 12, st);  // (grad_slices has no element)
  if (equalize) {
    if (vol_weight == nullptr || vol == nullptr) return (int)hipErrorInvalidValue;
    const int64_t nv = (int64_t)D * H * W;
    hipLaunchKernelGGL(slice_acq_equalize_grad<T>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, grad_vol, vol_weight, nv);
  }
  hipLaunchKernelGGL(slice_acq_adjoint_bwd<T>, dim3((unsigned)n), dim3(256), 0, st, transforms, (const T*)grad_vol, psf, slices,
                     slices_mask, equalize ? vol : (const T*)nullptr, vol_mask, grad_slices, grad_transforms, D, H, W, d_p, h_p,
                     w_p, h, w, res_slice);
  return (int)hipGetLastError();
}

template <typename T>
int slice_acq_forward_impl(const T* transforms, const T* vol, const uint8_t* vol_mask,
                                        const uint8_t* slices_mask, const T* psf, T* slices,
                                        T* slices_weight, int D, int H, int W, int d_p, int h_p, int w_p, int n,
                                        int h, int w, T res_slice, int interp_psf, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)n * h * w;
  if (total <= 0) return 0;
  const bool lds = (int64_t)d_p * h_p * w_p <= kMaxTaps;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define NESVOR_LAUNCH_FWD(I, L)                                                                                           \
  hipLaunchKernelGGL((slice_acq_fwd<T, I, L>), grid, block, 0, (hipStream_t)stream, transforms, vol, vol_mask, slices_mask, psf, \
                     slices, slices_weight, D, H, W, d_p, h_p, w_p, n, h, w, res_slice)
  if (interp_psf) { if (lds) NESVOR_LAUNCH_FWD(true, true); else NESVOR_LAUNCH_FWD(true, false); }
  else { if (lds) NESVOR_LAUNCH_FWD(false, true); else NESVOR_LAUNCH_FWD(false, false); }
#undef NESVOR_LAUNCH_FWD
  return (int)hipGetLastError();
}

template <typename T>
int slice_acq_adjoint_forward_impl(const T* transforms, const T* psf, const T* slices,
                                                const uint8_t* slices_mask, const uint8_t* vol_mask, T* vol,
                                                T* vol_weight, T* scratch, int D, int H, int W, int d_p, int h_p,
                                                int w_p, int n, int h, int w, T res_slice, int equalize, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  const int64_t np = (int64_t)n * h * w, nv = (int64_t)D * H * W;
  if (nv <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  T* coef = scratch;
  T* cw = scratch + np;
  if (np > 0)
    hipLaunchKernelGGL(slice_acq_pixel_coef<T>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, transforms, psf, slices,
                       slices_mask, coef, cw, D, H, W, d_p, h_p, w_p, n, h, w, res_slice, 0);
  hipLaunchKernelGGL((slice_acq_adjoint_gather<T, OnePsf<T>>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, transforms,
                     OnePsf<T>{psf, d_p, h_p, w_p}, coef, (equalize || vol_weight != nullptr) ? cw : (const T*)nullptr, vol_mask, vol,
                     vol_weight, D, H, W, n, h, w, res_slice, equalize, 0);
  return (int)hipGetLastError();
}

// The bank entry points' common checks -> the kernel argument and the per-slice grid (n * wgs workgroups of 256 pixels).
bool bank_request(const float* psf_bank, const int* psf_table, int P, const int* psf_id, int D, int H, int W, int n, int h, int w,
                  BankPsf<float>& bank, int64_t& wgs) {
  int64_t max_elements;
  if (!make_bank(psf_bank, psf_table, P, psf_id, n, bank, max_elements) || volume_too_large(D, H, W)) return false;
  if (n < 0 || h < 0 || w < 0 || (int64_t)h * w > (int64_t)INT_MAX) return false;
  wgs = ((int64_t)h * w + 255) / 256;
  return wgs * n <= (int64_t)INT_MAX;
}

int slice_acq_forward_bank_impl(const float* transforms, const float* vol, const uint8_t* vol_mask, const uint8_t* slices_mask,
                                const float* psf_bank, const int* psf_table, int P, const int* psf_id, float* slices,
                                float* slices_weight, int D, int H, int W, int n, int h, int w, float res_slice, void* stream) {
  BankPsf<float> bank;
  int64_t wgs;
  if (!bank_request(psf_bank, psf_table, P, psf_id, D, H, W, n, h, w, bank, wgs)) return (int)hipErrorInvalidValue;
  if (wgs * n <= 0) return 0;
  hipLaunchKernelGGL(slice_acq_fwd_bank, dim3((unsigned)(wgs * n)), dim3(256), 0, (hipStream_t)stream, transforms, vol, vol_mask,
                     slices_mask, bank, slices, slices_weight, D, H, W, h, w, (int)wgs, res_slice);
  return (int)hipGetLastError();
}

int slice_acq_adjoint_forward_bank_impl(const float* transforms, const float* psf_bank, const int* psf_table, int P, const int* psf_id,
                                        const float* slices, const uint8_t* slices_mask, const uint8_t* vol_mask, float* vol,
                                        float* vol_weight, float* scratch, int D, int H, int W, int n, int h, int w, float res_slice,
                                        int equalize, void* stream) {
  BankPsf<float> bank;
  int64_t wgs;
  if (!bank_request(psf_bank, psf_table, P, psf_id, D, H, W, n, h, w, bank, wgs)) return (int)hipErrorInvalidValue;
  const int64_t np = (int64_t)n * h * w, nv = (int64_t)D * H * W;
  if (nv <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (np <= 0) {  // an empty stack launches nothing: A^T of it is the zero volume, by two clears
    const int e = zero_fill(vol, nv, st);
    return e != 0 ? e : zero_fill(vol_weight, nv, st);
  }
  float* coef = scratch;
  float* cw = scratch + np;
  hipLaunchKernelGGL(slice_acq_pixel_coef_bank, dim3((unsigned)(wgs * n)), dim3(256), 0, st, transforms, bank, slices, slices_mask,
                     coef, cw, D, H, W, h, w, (int)wgs, res_slice);
  hipLaunchKernelGGL((slice_acq_adjoint_gather<float, BankPsf<float>>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, transforms,
                     bank, (const float*)coef, (equalize || vol_weight != nullptr) ? (const float*)cw : (const float*)nullptr, vol_mask,
                     vol, vol_weight, D, H, W, n, h, w, res_slice, equalize, 0);
  return (int)hipGetLastError();
}

template <typename T>
int slice_acq_backward_impl(const T* transforms, const T* vol, const uint8_t* vol_mask,
                                         const T* psf, const T* grad_slices, const uint8_t* slices_mask,
                                         T* grad_vol, T* grad_transforms, T* scratch, int D, int H, int W,
                                         int d_p, int h_p, int w_p, int n, int h, int w, T res_slice, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  const int64_t np = (int64_t)n * h * w, nv = (int64_t)D * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (np <= 0 || nv <= 0) {
    const int e = zero_fill(grad_vol, nv, st);
    return e != 0 ? e : zero_fill(grad_transforms, (int64_t)n * 12, st);
  }
  T* coef = scratch;
  hipLaunchKernelGGL(slice_acq_pixel_coef<T>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, transforms, psf, grad_slices,
                     slices_mask, coef, (T*)nullptr, D, H, W, d_p, h_p, w_p, n, h, w, res_slice, 1);
  if (grad_vol != nullptr)
    hipLaunchKernelGGL((slice_acq_adjoint_gather<T, OnePsf<T>>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, transforms,
                       OnePsf<T>{psf, d_p, h_p, w_p}, coef, (const T*)nullptr, vol_mask, grad_vol, (T*)nullptr, D, H, W, n, h, w,
                       res_slice, 0, 0);
  if (grad_transforms != nullptr)
    hipLaunchKernelGGL(slice_acq_bwd_transforms<T>, dim3((unsigned)n), dim3(256), 0, st, transforms, vol, vol_mask, psf, coef,
                       grad_transforms, D, H, W, d_p, h_p, w_p, h, w, res_slice);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ interp_psf mode of A^T and of both backwards
// `interp_psf = true` (nearest voxel + the PSF re-interpolated at the voxel's offset from the pixel centre) exists in all
// four reference kernels (slice_acq_cuda_kernel.cu:71-109 forward, :229-257 / :279-370 backward, :526-572 / :582-606
// adjoint, :754-836 adjoint backward), and no caller of the reference ever switches it on.  It is built here for
// completeness of the module, one thread per slice pixel exactly as the reference formulates it; the scatters are
// global atomics (memory-side on MI355X, ~16 G/s: fine for a mode nothing iterates on - the linear mode above is the
// one that was re-formulated as a gather).  interp_tap stands above the forward kernel, which takes it too.

// the taps of a pixel: body(tap) for every non-zero PSF tap whose position lies inside the volume and whose rounded voxel
// lies inside the PSF support
template <typename T, bool GRAD, typename Body>
__device__ __forceinline__ void for_interp_taps(const T* __restrict__ t, const PixelGeom<T>& g, const T* __restrict__ psf, int d_p,
                                                int h_p, int w_p, int D, int H, int W, Body body) {
  for_psf_taps(t, g, psf, d_p, h_p, w_p, D, H, W, [&](T, T, T, T, T x, T y, T z) {
    InterpTap<T> tap;
    if (interp_tap<T, GRAD>(t, g, psf, d_p, h_p, w_p, x, y, z, W, H * W, tap)) body(tap);
  });
}

// the 12 pose sums of a pixel -> grad_transforms of its slice (wave reduction, one atomic per wave and entry)
template <typename T>
__device__ __forceinline__ void add_pose_grad(T* __restrict__ grad_transforms, int in, const T (&gt)[12], bool uniform_slice) {
  if (uniform_slice) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const T s = wave_sum(gt[k]);
      if ((threadIdx.x & 63) == 0 && s != (T)0.0) atomicAdd(grad_transforms + (size_t)in * 12 + k, s);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (gt[k] != (T)0.0) atomicAdd(grad_transforms + (size_t)in * 12 + k, gt[k]);
  }
}

// backward of A (.cu:173-470, interp branch): grad_vol[voxel] += pw gs,  grad_transforms from d pw / d pose
template <typename T>
__global__ __launch_bounds__(256) void slice_acq_bwd_interp(const T* __restrict__ transforms, const T* __restrict__ vol,
                                                            const uint8_t* __restrict__ vol_mask, const T* __restrict__ psf,
                                                            const T* __restrict__ grad_slices, const uint8_t* __restrict__ slices_mask,
                                                            T* __restrict__ grad_vol, T* __restrict__ grad_transforms, int D, int H,
                                                            int W, int d_p, int h_p, int w_p, int n, int h, int w, T res_slice) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n * h * w;
  const int64_t cidx = idx < total ? idx : total - 1;
  const int ix = cidx % w, iy = (cidx / w) % h, in = cidx / ((int64_t)h * w);
  const T* t = transforms + (size_t)in * 12;
  T gt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) gt[k] = (T)0.0;
  T gs = idx < total && (slices_mask == nullptr || slices_mask[idx]) ? grad_slices[idx] : (T)0.0;
  if (gs != (T)0.0) {
    const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
    T weight = (T)0.0;  // pass 1: no vol_mask here (.cu:229-257)
    for_interp_taps<T, false>(t, g, psf, d_p, h_p, w_p, D, H, W, [&](const InterpTap<T>& tap) { weight += tap.pw; });
    if (weight != (T)0.0) {
      gs /= weight;
      const T cx = (W - 1) / (T)2.0, cy = (H - 1) / (T)2.0, cz = (D - 1) / (T)2.0;
      for_interp_taps<T, true>(t, g, psf, d_p, h_p, w_p, D, H, W, [&](const InterpTap<T>& tap) {
        if (vol_mask != nullptr && !vol_mask[tap.iv]) return;
        if (grad_vol != nullptr) atomicAdd(grad_vol + tap.iv, tap.pw * gs);
        if (grad_transforms != nullptr) {
          const T tmp = gs * vol[tap.iv];
          const T dx = tap.gx * tmp, dy = tap.gy * tmp, dz = tap.gz * tmp;
          gt[0] += dx * (tap.xr - cx); gt[1] += dy * (tap.xr - cx); gt[2] += dz * (tap.xr - cx); gt[3] -= dx;
          gt[4] += dx * (tap.yr - cy); gt[5] += dy * (tap.yr - cy); gt[6] += dz * (tap.yr - cy); gt[7] -= dy;
          gt[8] += dx * (tap.zr - cz); gt[9] += dy * (tap.zr - cz); gt[10] += dz * (tap.zr - cz); gt[11] -= dz;
        }
      });
    }
  }
  if (grad_transforms != nullptr) {
    // a wave lies in one slice iff its first and last pixel do (then one atomic per wave instead of 64)
    const int64_t first = idx - (threadIdx.x & 63), last = first + 63;
    const bool uniform = last < total && first / ((int64_t)h * w) == last / ((int64_t)h * w);
    add_pose_grad(grad_transforms, in, gt, uniform);
  }
}

// A^T (.cu:472-670, interp branch): vol[voxel] += pw / weight s, vol_weight[voxel] += pw / weight for weight >= 0.5
template <typename T>
__global__ __launch_bounds__(256) void slice_acq_adjoint_interp(const T* __restrict__ transforms, const T* __restrict__ psf,
                                                                const T* __restrict__ slices, const uint8_t* __restrict__ slices_mask,
                                                                const uint8_t* __restrict__ vol_mask, T* __restrict__ vol,
                                                                T* __restrict__ vol_weight, int D, int H, int W, int d_p, int h_p,
                                                                int w_p, int n, int h, int w, T res_slice) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * h * w) return;
  if (slices_mask != nullptr && !slices_mask[idx]) return;
  const T s = slices[idx];
  const int ix = idx % w, iy = (idx / w) % h, in = idx / ((int64_t)h * w);
  const T* t = transforms + (size_t)in * 12;
  const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
  T weight = (T)0.0;
  for_interp_taps<T, false>(t, g, psf, d_p, h_p, w_p, D, H, W, [&](const InterpTap<T>& tap) { weight += tap.pw; });
  if (weight < (T)0.5) return;  // border
  for_interp_taps<T, false>(t, g, psf, d_p, h_p, w_p, D, H, W, [&](const InterpTap<T>& tap) {
    if (vol_mask != nullptr && !vol_mask[tap.iv]) return;
    const T pn = tap.pw / weight;
    atomicAdd(vol + tap.iv, pn * s);
    if (vol_weight != nullptr) atomicAdd(vol_weight + tap.iv, pn);
  });
}

template <typename T>
__global__ void slice_acq_equalize_vol(T* __restrict__ vol, const T* __restrict__ vol_weight, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && vol_weight[i] > (T)0.0) vol[i] /= vol_weight[i];
}

// backward of A^T (.cu:695-950, interp branch): grad_slices = sum pw g[voxel] / sum pw,  pose gradient from d pw / d pose
template <typename T>
__global__ __launch_bounds__(256) void slice_acq_adjoint_bwd_interp(const T* __restrict__ transforms, const T* __restrict__ grad_vol,
                                                                    const T* __restrict__ psf, const T* __restrict__ slices,
                                                                    const uint8_t* __restrict__ slices_mask, const T* __restrict__ vol,
                                                                    const uint8_t* __restrict__ vol_mask, T* __restrict__ grad_slices,
                                                                    T* __restrict__ grad_transforms, int D, int H, int W, int d_p,
                                                                    int h_p, int w_p, int n, int h, int w, T res_slice) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n * h * w;
  const int64_t cidx = idx < total ? idx : total - 1;
  const int ix = cidx % w, iy = (cidx / w) % h, in = cidx / ((int64_t)h * w);
  const T* t = transforms + (size_t)in * 12;
  T gt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) gt[k] = (T)0.0;
  if (idx < total && (slices_mask == nullptr || slices_mask[idx])) {
    const PixelGeom<T> g = pixel_geom(t, ix, iy, h, w, res_slice, D, H, W);
    const T sv = slices[idx];
    const T cx = (W - 1) / (T)2.0, cy = (H - 1) / (T)2.0, cz = (D - 1) / (T)2.0;
    T val = (T)0.0, weight = (T)0.0;
    T acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = (T)0.0;
    // the reference tests the voxel mask before the PSF support; both only skip the tap, the order does not matter
    for_interp_taps<T, true>(t, g, psf, d_p, h_p, w_p, D, H, W, [&](const InterpTap<T>& tap) {
      if (vol_mask != nullptr && !vol_mask[tap.iv]) return;
      const T gv = grad_vol[tap.iv];
      if (grad_transforms != nullptr) {
        const T s = (vol == nullptr ? sv : sv - vol[tap.iv]) * gv;
        const T dx = tap.gx * s, dy = tap.gy * s, dz = tap.gz * s;
        acc[0] += dx * (tap.xr - cx); acc[1] += dy * (tap.xr - cx); acc[2] += dz * (tap.xr - cx); acc[3] -= dx;
        acc[4] += dx * (tap.yr - cy); acc[5] += dy * (tap.yr - cy); acc[6] += dz * (tap.yr - cy); acc[7] -= dy;
        acc[8] += dx * (tap.zr - cz); acc[9] += dy * (tap.zr - cz); acc[10] += dz * (tap.zr - cz); acc[11] -= dz;
      }
      val += tap.pw * gv;
      weight += tap.pw;
    });
    if (weight > (T)0.0) {
      if (grad_slices != nullptr) grad_slices[idx] = val / weight;
#pragma unroll
      for (int k = 0; k < 12; ++k) gt[k] = acc[k] / weight;
    }
  }
  if (grad_transforms != nullptr) {
    const int64_t first = idx - (threadIdx.x & 63), last = first + 63;
    const bool uniform = last < total && first / ((int64_t)h * w) == last / ((int64_t)h * w);
    add_pose_grad(grad_transforms, in, gt, uniform);
  }
}

// host side of the interp_psf mode.  Outputs are accumulated into: the callers pass zero-filled vol / vol_weight /
// grad_vol / grad_transforms / grad_slices (as the reference's host functions allocate them, .cu:1000-1120)
template <typename T>
int slice_acq_backward_interp_impl(const T* transforms, const T* vol, const uint8_t* vol_mask, const T* psf, const T* grad_slices,
                                   const uint8_t* slices_mask, T* grad_vol, T* grad_transforms, int D, int H, int W, int d_p,
                                   int h_p, int w_p, int n, int h, int w, T res_slice, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  const int64_t np = (int64_t)n * h * w;
  if (np <= 0 || (int64_t)D * H * W <= 0) return 0;
  if (d_p < 2 || h_p < 2 || w_p < 2) return 0;  // no interior cell in the PSF: every tap is skipped
  hipLaunchKernelGGL(slice_acq_bwd_interp<T>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, transforms, vol,
                     vol_mask, psf, grad_slices, slices_mask, grad_vol, grad_transforms, D, H, W, d_p, h_p, w_p, n, h, w, res_slice);
  return (int)hipGetLastError();
}
template <typename T>
int slice_acq_adjoint_forward_interp_impl(const T* transforms, const T* psf, const T* slices, const uint8_t* slices_mask,
                                          const uint8_t* vol_mask, T* vol, T* vol_weight, int D, int H, int W, int d_p, int h_p,
                                          int w_p, int n, int h, int w, T res_slice, int equalize, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  const int64_t np = (int64_t)n * h * w, nv = (int64_t)D * H * W;
  if (np <= 0 || nv <= 0) return 0;
  if (equalize && vol_weight == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (d_p >= 2 && h_p >= 2 && w_p >= 2)
    hipLaunchKernelGGL(slice_acq_adjoint_interp<T>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, transforms, psf, slices,
                       slices_mask, vol_mask, vol, vol_weight, D, H, W, d_p, h_p, w_p, n, h, w, res_slice);
  if (equalize)
    hipLaunchKernelGGL(slice_acq_equalize_vol<T>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, vol, (const T*)vol_weight, nv);
  return (int)hipGetLastError();
}
template <typename T>
int slice_acq_adjoint_backward_interp_impl(const T* transforms, T* grad_vol, const T* vol_weight, const uint8_t* vol_mask,
                                           const T* psf, const T* slices, const uint8_t* slices_mask, const T* vol, T* grad_slices,
                                           T* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                                           T res_slice, int equalize, void* stream) {
  if (volume_too_large(D, H, W)) return (int)hipErrorInvalidValue;
  const int64_t np = (int64_t)n * h * w;
  if (np <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (equalize) {
    if (vol_weight == nullptr || vol == nullptr) return (int)hipErrorInvalidValue;
    const int64_t nv = (int64_t)D * H * W;
    hipLaunchKernelGGL(slice_acq_equalize_grad<T>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, grad_vol, vol_weight, nv);
  }
  if (d_p < 2 || h_p < 2 || w_p < 2) return (int)hipGetLastError();
  hipLaunchKernelGGL(slice_acq_adjoint_bwd_interp<T>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, transforms,
                     (const T*)grad_vol, psf, slices, slices_mask, equalize ? vol : (const T*)nullptr, vol_mask, grad_slices,
                     grad_transforms, D, H, W, d_p, h_p, w_p, n, h, w, res_slice);
  return (int)hipGetLastError();
}

}  // namespace

// ---- C entry points: float (the path every caller of the reference uses) and double (AT_DISPATCH_FLOATING_TYPES,
//      slice_acq_cuda_kernel.cu:970-1114)
#define NESVOR_SLICE_ACQ_ENTRY(SUFFIX, T)                                                                                      \
  extern "C" int nesvor_slice_acq_forward##SUFFIX(const T* transforms, const T* vol, const uint8_t* vol_mask,                  \
                                                  const uint8_t* slices_mask, const T* psf, T* slices, T* slices_weight, int D, \
                                                  int H, int W, int d_p, int h_p, int w_p, int n, int h, int w, T res_slice,    \
                                                  int interp_psf, void* stream) {                                               \
    return slice_acq_forward_impl<T>(transforms, vol, vol_mask, slices_mask, psf, slices, slices_weight, D, H, W, d_p, h_p,    \
                                     w_p, n, h, w, res_slice, interp_psf, stream);                                              \
  }                                                                                                                            \
  extern "C" int nesvor_slice_acq_adjoint_forward##SUFFIX(const T* transforms, const T* psf, const T* slices,                  \
                                                          const uint8_t* slices_mask, const uint8_t* vol_mask, T* vol,          \
                                                          T* vol_weight, T* scratch, int D, int H, int W, int d_p, int h_p,     \
                                                          int w_p, int n, int h, int w, T res_slice, int equalize,              \
                                                          void* stream) {                                                       \
    return slice_acq_adjoint_forward_impl<T>(transforms, psf, slices, slices_mask, vol_mask, vol, vol_weight, scratch, D, H, W, \
                                             d_p, h_p, w_p, n, h, w, res_slice, equalize, stream);                              \
  }                                                                                                                            \
  extern "C" int nesvor_slice_acq_backward##SUFFIX(const T* transforms, const T* vol, const uint8_t* vol_mask, const T* psf,   \
                                                   const T* grad_slices, const uint8_t* slices_mask, T* grad_vol,               \
                                                   T* grad_transforms, T* scratch, int D, int H, int W, int d_p, int h_p,       \
                                                   int w_p, int n, int h, int w, T res_slice, void* stream) {                   \
    return slice_acq_backward_impl<T>(transforms, vol, vol_mask, psf, grad_slices, slices_mask, grad_vol, grad_transforms,      \
                                      scratch, D, H, W, d_p, h_p, w_p, n, h, w, res_slice, stream);                             \
  }                                                                                                                            \
  extern "C" int nesvor_slice_acq_adjoint_backward##SUFFIX(const T* transforms, T* grad_vol, const T* vol_weight,              \
                                                           const uint8_t* vol_mask, const T* psf, const T* slices,              \
                                                           const uint8_t* slices_mask, const T* vol, T* grad_slices,            \
                                                           T* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p,  \
                                                           int n, int h, int w, T res_slice, int equalize, void* stream) {      \
    return slice_acq_adjoint_backward_impl<T>(transforms, grad_vol, vol_weight, vol_mask, psf, slices, slices_mask, vol,        \
                                              grad_slices, grad_transforms, D, H, W, d_p, h_p, w_p, n, h, w, res_slice,         \
                                              equalize, stream);                                                                \
  }                                                                                                                            \
  /* interp_psf = true: same arguments (no scratch), outputs zero-filled by the caller and accumulated into */                 \
  extern "C" int nesvor_slice_acq_adjoint_forward_interp##SUFFIX(const T* transforms, const T* psf, const T* slices,           \
                                                                 const uint8_t* slices_mask, const uint8_t* vol_mask, T* vol,   \
                                                                 T* vol_weight, int D, int H, int W, int d_p, int h_p, int w_p, \
                                                                 int n, int h, int w, T res_slice, int equalize, void* stream) {\
    return slice_acq_adjoint_forward_interp_impl<T>(transforms, psf, slices, slices_mask, vol_mask, vol, vol_weight, D, H, W,   \
                                                    d_p, h_p, w_p, n, h, w, res_slice, equalize, stream);                       \
  }                                                                                                                            \
  extern "C" int nesvor_slice_acq_backward_interp##SUFFIX(const T* transforms, const T* vol, const uint8_t* vol_mask,          \
                                                          const T* psf, const T* grad_slices, const uint8_t* slices_mask,       \
                                                          T* grad_vol, T* grad_transforms, int D, int H, int W, int d_p,        \
                                                          int h_p, int w_p, int n, int h, int w, T res_slice, void* stream) {   \
    return slice_acq_backward_interp_impl<T>(transforms, vol, vol_mask, psf, grad_slices, slices_mask, grad_vol,                \
                                             grad_transforms, D, H, W, d_p, h_p, w_p, n, h, w, res_slice, stream);              \
  }                                                                                                                            \
  extern "C" int nesvor_slice_acq_adjoint_backward_interp##SUFFIX(const T* transforms, T* grad_vol, const T* vol_weight,       \
                                                                  const uint8_t* vol_mask, const T* psf, const T* slices,       \
                                                                  const uint8_t* slices_mask, const T* vol, T* grad_slices,     \
                                                                  T* grad_transforms, int D, int H, int W, int d_p, int h_p,    \
                                                                  int w_p, int n, int h, int w, T res_slice, int equalize,      \
                                                                  void* stream) {                                               \
    return slice_acq_adjoint_backward_interp_impl<T>(transforms, grad_vol, vol_weight, vol_mask, psf, slices, slices_mask, vol, \
                                                     grad_slices, grad_transforms, D, H, W, d_p, h_p, w_p, n, h, w, res_slice,  \
                                                     equalize, stream);                                                         \
  }
NESVOR_SLICE_ACQ_ENTRY(, float)
NESVOR_SLICE_ACQ_ENTRY(_f64, double)
#undef NESVOR_SLICE_ACQ_ENTRY

// ---- A and A^T with a PSF bank (fp32, linear mode): slice k takes PSF psf_id[k]
extern "C" int nesvor_slice_acq_forward_bank(const float* transforms, const float* vol, const uint8_t* vol_mask,
                                             const uint8_t* slices_mask, const float* psf_bank, const int32_t* psf_table, int P,
                                             const int32_t* psf_id, float* slices, float* slices_weight, int D, int H, int W, int n,
                                             int h, int w, float res_slice, void* stream) {
  return slice_acq_forward_bank_impl(transforms, vol, vol_mask, slices_mask, psf_bank, psf_table, P, psf_id, slices, slices_weight, D, H,
                                     W, n, h, w, res_slice, stream);
}
extern "C" int nesvor_slice_acq_adjoint_forward_bank(const float* transforms, const float* psf_bank, const int32_t* psf_table, int P,
                                                     const int32_t* psf_id, const float* slices, const uint8_t* slices_mask,
                                                     const uint8_t* vol_mask, float* vol, float* vol_weight, float* scratch, int D,
                                                     int H, int W, int n, int h, int w, float res_slice, int equalize, void* stream) {
  return slice_acq_adjoint_forward_bank_impl(transforms, psf_bank, psf_table, P, psf_id, slices, slices_mask, vol_mask, vol, vol_weight,
                                             scratch, D, H, W, n, h, w, res_slice, equalize, stream);
}
