// The sample of the stack registration's kernels: the source volume at one point of the target's list under one pose.  vvr_nmi.hip's
// kernels (the joint histograms, the samples themselves) call sample_point; vvr.hip's moment sums share fetch and keep the same
// operations written out (see there).
//
// Sampling = F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True): normalised coordinate g in
// [-1, 1] -> index (g + 1) / 2 * (size - 1); corners outside the volume contribute 0, so a point that leaves the source samples 0.
#pragma once
#include <hip/hip_runtime.h>

namespace {
namespace vvr {

__device__ __forceinline__ float fetch(const float* __restrict__ v, int x, int y, int z, int W, int H, int D) {
  return (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) ? v[((size_t)z * H + y) * W + x] : 0.f;
}

// src (D,H,W) at the point (px, py, pz) [mm] moved by m = rows of [R | t], translation applied first: R (p + t); (ux, uy, uz) maps
// the moved point to normalised coordinates, (hx, hy, hz) = (size - 1) / 2 per axis.
__device__ __forceinline__ float sample_point(const float* __restrict__ src, int D, int H, int W, const float* m, float px, float py,
                                              float pz, float ux, float uy, float uz, float hx, float hy, float hz) {
  const float qx = px + m[3], qy = py + m[7], qz = pz + m[11];
  const float gx = (m[0] * qx + m[1] * qy + m[2] * qz) * ux, gy = (m[4] * qx + m[5] * qy + m[6] * qz) * uy,
              gz = (m[8] * qx + m[9] * qy + m[10] * qz) * uz;
  const float fx = (gx + 1.f) * hx, fy = (gy + 1.f) * hy, fz = (gz + 1.f) * hz;
  const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
  const float wx = fx - x0f, wy = fy - y0f, wz = fz - z0f;
  // (int) of a huge or NaN coordinate is clamped by the range test in fetch()
  const int x0 = (int)fmaxf(fminf(x0f, 1e9f), -1e9f), y0 = (int)fmaxf(fminf(y0f, 1e9f), -1e9f), z0 = (int)fmaxf(fminf(z0f, 1e9f), -1e9f);
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float w = ((c & 1) ? wx : 1.f - wx) * ((c & 2) ? wy : 1.f - wy) * ((c & 4) ? wz : 1.f - wz);
    v = fmaf(w, fetch(src, x0 + (c & 1), y0 + ((c >> 1) & 1), z0 + (c >> 2), W, H, D), v);
  }
  return v;
}

}  // namespace vvr
}  // namespace
