// What the joint-histogram kernels of the mutual-information similarity share (svr_nmi.hip: one histogram per (slice, pose);
// vvr_nmi.hip: one per pose of a stack pair): the place of a value on a binned axis, the four integer adds of a sample, the rule
// that cuts a list of samples into segments and the launch that adds the segments' 32-bit cells in 64 bits.  The definition itself
// is nesvor_amd/nmi.py's.
//
// A unit of work is a (entry, segment): one workgroup keeps the B x B histogram of its segment in LDS (32-bit cells, at most
// 16 KB), adds with integer LDS atomics and stores the cells to its own rows of the workspace, (entries, S, B, B) uint32, with plain
// stores; joint_histogram_reduce_kernel then writes every cell of the (entries, B, B) int64 result.  A segment holds at most
// kMaxSegmentPixels <= 65535 samples of at most 65536 units each, so no cell overflows; integer adds, so nothing depends on their
// order.  The segment length is the launch's (segment_pixels): a call with many entries takes long segments, which pay a
// workgroup's fixed cost - the histogram's clear and store - once per many samples; a call with few entries cuts its list until about
// kTargetWorkgroups workgroups fill the chip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
namespace nmi_hist {

constexpr int kMaxNmiBins = 64;
constexpr int kMinSegmentPixels = 1024, kMaxSegmentPixels = 16384;  // multiples of the workgroup's 256 samples
constexpr int kTargetWorkgroups = 1024;                             // four per CU: what a launch is cut for
static_assert(kMinSegmentPixels % 256 == 0 && kMaxSegmentPixels % 256 == 0 && kMaxSegmentPixels <= 65535,
              "a 32-bit cell holds at most 65535 pixels of 65536 units");

// A value's place on an axis: the lower bin and the weight (of 256) of the upper one.
struct AxisPlace { int b0, q; };

__device__ __forceinline__ AxisPlace axis_place(float v, float lo, float scale, int B) {
  const float u = fminf(fmaxf((v - lo) * scale, 0.f), (float)(B - 1));  // (a NaN becomes 0: nothing is indexed by it)
  const int b0 = min((int)u, B - 2);
  const float f = u - (float)b0;
  return AxisPlace{b0, (int)(f * 256.f + 0.5f)};
}

// One sample's 65536 units: the four products of its I weights (a) and its J weights (b), each handed with its cell (bI, bJ) of a
// B x B histogram, row = I bin, to add(cell, product) - the kernel's LDS atomic; zero products skipped.
template <typename Add>
__device__ __forceinline__ void add_sample(const AxisPlace a, const AxisPlace b, int B, const Add add) {
  const int c00 = a.b0 * B + b.b0;  // at most (B - 2) B + B - 2: the four cells stay below B B
  const uint32_t ai[2] = {(uint32_t)(256 - a.q), (uint32_t)a.q}, bj[2] = {(uint32_t)(256 - b.q), (uint32_t)b.q};
#pragma unroll
  for (int di = 0; di < 2; ++di)
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      const uint32_t p = ai[di] * bj[dj];
      if (p != 0u) add(c00 + di * B + dj, p);
    }
}

// out[e][c] = the S segments of entry e added in 64 bits; one thread per (entry, cell), total = entries * cells.
__global__ __launch_bounds__(256) void joint_histogram_reduce_kernel(const uint32_t* __restrict__ partial, int64_t total, int cells, int S,
                                                                     int64_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t e = t / cells;
  const int c = (int)(t - e * cells);
  int64_t sum = 0;
  for (int s = 0; s < S; ++s) sum += (int64_t)partial[((size_t)e * S + s) * cells + c];
  out[t] = sum;
}

// The segment length of a launch of `entries` lists of hw samples each: the list cut into as many segments as it takes to reach
// kTargetWorkgroups workgroups, in whole trips of 256 samples, between kMinSegmentPixels and kMaxSegmentPixels.
inline int segment_pixels(int64_t entries, int64_t hw) {
  const int64_t want = (kTargetWorkgroups + entries - 1) / entries;
  const int64_t seg = ((hw + want - 1) / want + 255) / 256 * 256;
  return (int)(seg < kMinSegmentPixels ? kMinSegmentPixels : seg > kMaxSegmentPixels ? kMaxSegmentPixels : seg);
}
inline int64_t segments(int64_t entries, int64_t hw) {
  const int64_t seg = segment_pixels(entries, hw);
  return (hw + seg - 1) / seg;
}

}  // namespace nmi_hist
}  // namespace
