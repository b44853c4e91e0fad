// One gradient-descent step of the classical super-resolution reconstruction with the edge-preserving prior (gfx950):
//
//   out[a] = x[a] - alpha * (grad[a] + beta * dR(x)[a]),      optionally clamped at 0,
//
// dR as nesvor_amd/srr.py::edge_prior_gradient defines it (the reference's svort/srr.py:139-160): for an interior voxel the sum
// over its 26 neighbours o of  t / sqrt(1 + d t),  d = x[a] - x[a+o],  t = d / (|o|^2 delta^2);  0 on every border voxel.
// Composed from torch operators that is 26 shifted copies of the volume, four more temporaries of that size and about 40
// launches; here it is one launch that moves 12 bytes per voxel (x and grad in, out back).
//
// A workgroup owns a 32 x 8 (x, y) tile and marches along z over up to 16 planes.  Four planes of the tile with a one-voxel
// halo live in LDS as a ring: while the wave computes plane z from slots z-1, z, z+1, the slot of plane z+2 is free, so one
// barrier per plane is enough, and the global load of plane z+2 is in flight during the arithmetic of plane z.  Every value
// of x is fetched once per tile that touches it (halo: 340 / 256 per plane, 18 / 16 per march - the repeats hit in L2).
//
// The arithmetic is that of the torch expression, operation for operation (the build has -ffp-contract=off): the three
// factors 1 / (|o|^2 delta^2) are rounded to float once on the host, a term is  (d c) * rsq(1 + d (d c)),  the 26 terms are
// added in the fixed neighbour order of srr.py::_OFFSETS, plane by plane (three partial sums).  No atomics: the result is
// bit-reproducible.  A border voxel computes  x - alpha * (grad + beta * 0)  =  x - alpha * grad  exactly.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kTX = 32, kTY = 8, kTZ = 16;  // voxels per workgroup: tile in x, y; planes per march
constexpr int kPW = kTX + 2, kPH = kTY + 2, kPlane = kPW * kPH;  // the tile with its halo: 34 x 10 = 340 floats
constexpr int kThreads = kTX * kTY;
static_assert(kThreads == 256 && kPlane > kThreads && kPlane <= 2 * kThreads, "every thread stages at most two halo elements");

// grid: tiles_x * tiles_y * tiles_z workgroups, x fastest.  out may be grad (each thread reads grad[a] before it stores out[a]);
// out must not overlap x (the host refuses it).
__global__ __launch_bounds__(kThreads) void srr_step_kernel(const float* __restrict__ x, const float* grad, float* out, int D, int H,
                                                            int W, int tiles_x, int tiles_y, float alpha, float beta, float c1,
                                                            float c2, float c3, int clamp) {
  __shared__ float tile[4][kPlane];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int bx = b % tiles_x;
  b /= tiles_x;
  const int by = b % tiles_y, bz = b / tiles_y;
  const int x0 = bx * kTX, y0 = by * kTY, z0 = bz * kTZ;
  const int z1 = min(z0 + kTZ, D);
  const int HW = H * W;  // the host checked D H W <= INT_MAX

  // the (up to) two elements of a halo plane this thread stages: offset inside a plane of x, or -1 outside the volume
  const int e0 = tid, e1 = tid + kThreads;
  int off0, off1 = -1;
  {
    const int ly = e0 / kPW, lx = e0 - ly * kPW;
    const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
    off0 = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? gy * W + gx : -1;
  }
  if (e1 < kPlane) {
    const int ly = e1 / kPW, lx = e1 - ly * kPW;
    const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
    off1 = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? gy * W + gx : -1;
  }
  auto fetch = [&](int z, float& a0, float& a1) {  // a position outside the volume reads as 0: no interior voxel uses it
    const bool zin = z >= 0 && z < D;
    const size_t base = (size_t)(zin ? z : 0) * HW;
    a0 = (zin && off0 >= 0) ? x[base + off0] : 0.f;
    a1 = (zin && off1 >= 0) ? x[base + off1] : 0.f;
  };
  auto stash = [&](int z, float a0, float a1) {
    float* t = tile[z & 3];
    t[e0] = a0;
    if (e1 < kPlane) t[e1] = a1;
  };

  float a0, a1;
  fetch(z0 - 1, a0, a1);
  stash(z0 - 1, a0, a1);
  fetch(z0, a0, a1);
  stash(z0, a0, a1);
  fetch(z0 + 1, a0, a1);

  const int lx = tid & (kTX - 1), ly = tid / kTX;
  const int gx = x0 + lx, gy = y0 + ly;
  const bool inside = gx < W && gy < H;
  const bool inner_xy = gx >= 1 && gx < W - 1 && gy >= 1 && gy < H - 1;
  const int c = (ly + 1) * kPW + lx + 1;
  for (int z = z0; z < z1; ++z) {
    // slot (z + 1) & 3 was last read while plane z - 2 was computed, and every thread has passed the barrier of plane z - 1 since
    stash(z + 1, a0, a1);
    __syncthreads();
    if (z + 1 < z1) fetch(z + 2, a0, a1);  // in flight during the arithmetic below
    if (inside) {
      const float* pm = tile[(z - 1) & 3];
      const float* p0 = tile[z & 3];
      const float* pp = tile[(z + 1) & 3];
      const float v = p0[c];
      float dr = 0.f;
      if (inner_xy && z >= 1 && z < D - 1) {
        float sm = 0.f, s0 = 0.f, sp = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int n2 = dy * dy + dx * dx;  // |o|^2 - 1 in the planes above and below
            const float cf = n2 == 0 ? c1 : n2 == 1 ? c2 : c3;
            const float d = v - pm[c + dy * kPW + dx];
            const float s = d * cf;
            sm += s * __builtin_amdgcn_rsqf(1.f + d * s);  // the argument is >= 1 (or NaN): the bare instruction is rsqrtf here
          }
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int n2 = dy * dy + dx * dx;
            if (n2 == 0) continue;
            const float cf = n2 == 1 ? c1 : c2;
            const float d = v - p0[c + dy * kPW + dx];
            const float s = d * cf;
            s0 += s * __builtin_amdgcn_rsqf(1.f + d * s);
          }
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int n2 = dy * dy + dx * dx;
            const float cf = n2 == 0 ? c1 : n2 == 1 ? c2 : c3;
            const float d = v - pp[c + dy * kPW + dx];
            const float s = d * cf;
            sp += s * __builtin_amdgcn_rsqf(1.f + d * s);
          }
        dr = (sm + s0) + sp;
      }
      const size_t i = (size_t)z * HW + (size_t)(gy * W + gx);
      float r = v - alpha * (grad[i] + beta * dr);
      if (clamp) r = r < 0.f ? 0.f : r;  // (not fmaxf: NaN stays NaN, as clamp_ keeps it)
      out[i] = r;
    }
  }
}

inline bool overlaps(const void* a, const void* b, size_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" int nesvor_srr_step(const float* x, const float* grad, float* out, int D, int H, int W, float alpha, float beta,
                               float delta, int clamp, void* stream) {
  if (x == nullptr || grad == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  if (D < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)D * H * W;
  if (n > INT_MAX) return (int)hipErrorInvalidValue;  // voxel indices inside a plane and LDS offsets are ints
  const size_t bytes = (size_t)n * sizeof(float);
  if (overlaps(out, x, bytes)) return (int)hipErrorInvalidValue;  // the stencil reads neighbours of x
  if (out != grad && overlaps(out, grad, bytes)) return (int)hipErrorInvalidValue;
  const int tiles_x = (W + kTX - 1) / kTX, tiles_y = (H + kTY - 1) / kTY, tiles_z = (D + kTZ - 1) / kTZ;
  const int64_t blocks = (int64_t)tiles_x * tiles_y * tiles_z;
  if (blocks > INT_MAX) return (int)hipErrorInvalidValue;  // (cannot happen: every workgroup owns at least one voxel)
  const double dd = (double)delta;  // 1 / (|o|^2 delta delta) in double, rounded once: as srr.py builds its factors
  hipLaunchKernelGGL(srr_step_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, grad, out, D, H, W, tiles_x,
                     tiles_y, alpha, beta, (float)(1.0 / (1.0 * dd * dd)), (float)(1.0 / (2.0 * dd * dd)),
                     (float)(1.0 / (3.0 * dd * dd)), clamp);
  return (int)hipGetLastError();
}
