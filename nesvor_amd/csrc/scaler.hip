// Loss scaler of the fp16 mode on the device (gfx950): torch.cuda.amp.GradScaler as the reference's training loop uses it
// (nesvor/nesvor/train.py:161-164, 190-196: scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()).
//
// The host form (nesvor_amd.fused.LossScaler without a device) reads one flag per iteration to decide whether the optimizer
// may step.  Here the decision never leaves the GPU:
//   nesvor_grad_found_inf      the finiteness check of the (all-reduced) flat gradient -> s->found_inf;
//   nesvor_adamw_step_scaled   AdamW predicated on s->found_inf, bias corrections and 1/scale formed from s;
//   nesvor_loss_scaler_update  GradScaler.update on s (one lane);
//   nesvor_loss_scale_weights  the loss kernel's upstream weights times s->scale, at the head of the step.
// After a sum all-reduce every rank holds the same gradient bits and reaches the same verdict: no extra collective.
// The state is written in plain C++ (vector memory instructions only).
#include <hip/hip_runtime.h>
#include "common.h"
#include "adam.h"
#include "../../include/nesvor_hip.h"

namespace {

constexpr int kInfBlock = 256;
constexpr int64_t kInfMaxBlocks = 256 * 8;

// exponent field all ones: +-Inf and every NaN
__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ bool non_finite4(const float4& q) {
  const uint32_t e = 0x7f800000u;
  // (a & e) == e for any of the four <=> min over the four of ((a & e) ^ e) == 0
  const uint32_t a = (__float_as_uint(q.x) & e) ^ e, b = (__float_as_uint(q.y) & e) ^ e;
  const uint32_t c = (__float_as_uint(q.z) & e) ^ e, d = (__float_as_uint(q.w) & e) ^ e;
  return min(min(a, b), min(c, d)) == 0u;
}

// grad = [head (0-3 floats up to the first 16-byte boundary) | n4 float4 | tail (0-3 floats)]
__global__ __launch_bounds__(kInfBlock) void grad_found_inf_kernel(const float* __restrict__ grad, int64_t n, int head,
                                                                 uint32_t* __restrict__ found_inf) {
  __shared__ int wg_bad;
  if (threadIdx.x == 0) wg_bad = 0;
  const int64_t n4 = (n - head) >> 2;
  const float4* __restrict__ body = reinterpret_cast<const float4*>(grad + head);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  int64_t i = gid;
  for (; i + stride < n4; i += 2 * stride) {  // two 16-byte loads in flight per lane
    const float4 a = body[i], b = body[i + stride];
    bad = bad || non_finite4(a) || non_finite4(b);
  }
  if (i < n4) bad |= non_finite4(body[i]);
  // scalar head and tail: at most 6 floats, threads 0-2 / 3-5 of the grid
  if (gid < head) bad |= non_finite(grad[gid]);
  const int64_t tail = head + (n4 << 2);
  if (gid >= 3 && tail + (gid - 3) < n && gid < 6) bad |= non_finite(grad[tail + gid - 3]);
  __syncthreads();
  // within the wave first (one ballot), then one LDS word per workgroup, then ONE global atomic per workgroup that saw any
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) wg_bad = 1;
  __syncthreads();
  if (threadIdx.x == 0 && wg_bad) atomicOr(found_inf, 1u);
}

template <bool ZERO>
__global__ __launch_bounds__(256) void adamw_scaled_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int64_t n, float lr, double beta1, double beta2,
                                                           float eps, float weight_decay, int world_size,
                                                           const nesvor_loss_scaler_t* __restrict__ s) {
  if (s->found_inf != 0u) {
    // the step is skipped: parameters and moments stay, the gradient is dropped (GradScaler.step + zero_grad)
    if (ZERO) {
      const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
        reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
      if (t < n) g[t] = 0.f;
    }
    return;
  }
  // what the host forms for nesvor_adamw_step (ops._adamw_step: 1 - beta**t and 1 / (world * scale) in double, then float;
  // make_adam_args in float): the same operations here, so a finite step is bit-identical to it
  const double t1 = (double)(s->t + 1);
  const float bc1 = (float)(1.0 - pow(beta1, t1)), bc2 = (float)(1.0 - pow(beta2, t1));
  const float grad_scale = (float)(1.0 / ((double)world_size * (double)s->scale));
  const AdamArgs a = make_adam_args(lr, (float)beta1, (float)beta2, eps, weight_decay, bc1, bc2, grad_scale);
  adamw_sweep<ZERO>(p, g, m, v, n, a);
}

__global__ __launch_bounds__(64) void loss_scaler_update_kernel(nesvor_loss_scaler_t* __restrict__ s) {
  if (threadIdx.x != 0) return;
  if (s->found_inf != 0u) {
    s->scale *= s->backoff_factor;
    s->growth_tracker = 0;
    s->skipped += 1;
  } else {
    s->t += 1;
    const int32_t tracker = s->growth_tracker + 1;
    if (tracker == s->growth_interval) {
      s->scale *= s->growth_factor;
      s->growth_tracker = 0;
    } else {
      s->growth_tracker = tracker;
    }
  }
  s->found_inf = 0u;
}

__global__ __launch_bounds__(64) void loss_scale_weights_kernel(const float* __restrict__ base, float* __restrict__ out, int n,
                                                                const nesvor_loss_scaler_t* __restrict__ s) {
  const int i = threadIdx.x;
  if (i < n) out[i] = base[i] * s->scale;
}

}  // namespace

extern "C" int nesvor_grad_found_inf(const float* grad, int64_t n, nesvor_loss_scaler_t* s, void* stream) {
  if (n <= 0) return 0;
  if (grad == nullptr || s == nullptr || ((uintptr_t)grad & 3)) return (int)hipErrorInvalidValue;
  int64_t head = (int64_t)(((16 - ((uintptr_t)grad & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int64_t n4 = (n - head) >> 2;
  int64_t blocks = (n4 + 2 * kInfBlock - 1) / (2 * kInfBlock);
  if (blocks < 1) blocks = 1;
  if (blocks > kInfMaxBlocks) blocks = kInfMaxBlocks;
  hipLaunchKernelGGL(grad_found_inf_kernel, dim3((unsigned)blocks), dim3(kInfBlock), 0, (hipStream_t)stream, grad, n, (int)head,
                     &s->found_inf);
  return (int)hipGetLastError();
}

extern "C" int nesvor_adamw_step_scaled(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                        double beta1, double beta2, float eps, float weight_decay, int world_size, int zero_grad,
                                        const nesvor_loss_scaler_t* s, void* stream) {
  if (n <= 0) return 0;
  if (s == nullptr || world_size < 1 || (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15))
    return (int)hipErrorInvalidValue;
  // nesvor_adamw_step's grid
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (zero_grad)
    hipLaunchKernelGGL((adamw_scaled_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, world_size, s);
  else
    hipLaunchKernelGGL((adamw_scaled_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, world_size, s);
  return (int)hipGetLastError();
}

extern "C" int nesvor_loss_scaler_update(nesvor_loss_scaler_t* s, void* stream) {
  if (s == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(loss_scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s);
  return (int)hipGetLastError();
}

extern "C" int nesvor_loss_scale_weights(const float* base, float* out, int n, const nesvor_loss_scaler_t* s, void* stream) {
  if (n <= 0) return 0;
  if (n > 64 || base == nullptr || out == nullptr || s == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(loss_scale_weights_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, base, out, n, s);
  return (int)hipGetLastError();
}
