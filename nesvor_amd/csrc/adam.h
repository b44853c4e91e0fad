// AdamW update of one parameter, shared by the flat-buffer optimiser kernel (adamw.hip) and the hash-grid backward's owner
// pass (hashgrid.hip), which can apply it to a table chunk while the chunk's gradient is still in LDS.
// Follows torch.optim.AdamW as the reference's training loop configures it (nesvor/nesvor/train.py:144-152).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

struct AdamArgs {
  float lr, beta1, beta2, eps, decay_mul, step_size, inv_sqrt_bc2, grad_scale;
};

// (__host__ __device__: the device loss scaler's AdamW forms the same numbers on the GPU, csrc/scaler.hip - the build's
// -ffp-contract=off and IEEE division / square root make both sides round alike)
__host__ __device__ inline AdamArgs make_adam_args(float lr, float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                               float bias_correction2, float grad_scale) {
  AdamArgs a;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.decay_mul = 1.f - lr * weight_decay;
  a.step_size = lr / bias_correction1;
  a.inv_sqrt_bc2 = 1.f / sqrtf(bias_correction2);
  a.grad_scale = grad_scale;
  return a;
}

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a) {
  const float gs = g * a.grad_scale;
  p *= a.decay_mul;
  m = fmaf(1.f - a.beta1, gs - m, m);
  v = fmaf(1.f - a.beta2, gs * gs, a.beta2 * v);
  const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
  p -= a.step_size * (m / denom);
}

// AdamW over a flat range, float4 per lane, grid-stride (+ zero-fill of the gradient): the body of nesvor_adamw_step's kernel
// (csrc/adamw.hip) and of the device loss scaler's predicated step (csrc/scaler.hip).  p, g, m, v 16-byte aligned.
template <bool ZERO>
__device__ __forceinline__ void adamw_sweep(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t n, const AdamArgs& a) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 P = reinterpret_cast<float4*>(p)[i], G = reinterpret_cast<float4*>(g)[i];
    float4 M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
    adam1(P.x, G.x, M.x, V.x, a); adam1(P.y, G.y, M.y, V.y, a);
    adam1(P.z, G.z, M.z, V.z, a); adam1(P.w, G.w, M.w, V.w, a);
    reinterpret_cast<float4*>(p)[i] = P;
    reinterpret_cast<float4*>(m)[i] = M;
    reinterpret_cast<float4*>(v)[i] = V;
    if (ZERO) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // tail (n not a multiple of 4)
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    adam1(p[t], g[t], m[t], v[t], a);
    if (ZERO) g[t] = 0.f;
  }
}
