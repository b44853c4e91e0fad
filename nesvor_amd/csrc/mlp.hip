// Fused small-MLP forward / backward for gfx950 on the fp32 matrix cores.
//
// Replaces the nn.Linear/ReLU stacks that the reference's build_network creates in
// single-precision mode (nesvor/nesvor/models.py:42-67; used for density_net :113-121,
// sigma_net :238-246, b_net :249-258) and the concat/expand glue in NeSVoR.net_forward
// (models.py:339-353).  rocBLAS runs these (N = 2^20) x 64 x 64 fp32 GEMMs at ~1-7 ms each
// (measured: 41 ms of a 46 ms iteration); here one launch runs a whole network.
//
// Formulation (all fp32, exact: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain):
//   H^T = W . X^T : MFMA rows i = output features, columns j = 16 samples, k = input features.
//   Lane l = (j = l & 15, q = l >> 4).  The accumulator fragment of a 16-feature block holds, in
//   lane (j,q), registers r = 0..3 -> feature 4q + r of sample j — which is exactly the B-operand
//   shape of the next layer if K is walked as k = 16 kb + 4 q + r.  Activations therefore never
//   leave registers between layers; only the weights are re-laid-out, once per workgroup, into LDS
//   images img[ob][kb][lane][r] = W[16 ob + (lane & 15)][16 kb + 4 (lane >> 4) + r] that every lane
//   reads with one conflict-free ds_read_b128 per four MFMAs.
//   Backward dX uses the same scheme with transposed images; dW/db contract over samples
//   (k = sample) and read their operands straight from the saved fragments.
//
// A network input is the concatenation [pixel features (P, k_a) broadcast over the S samples of a
// pixel | rows b_row0 .. b_row0 + k_b of a feature-major matrix (rows, N)], which covers
// density_net (pe), sigma_net (slice embedding | z[1:]) and b_net (slice embedding | pe[:n]) without
// materialising any expand/cat tensor (130 MB each in the reference).
//
// Saved for backward: post-ReLU hidden activations, stored as raw accumulator fragments
// ([group of 16 samples][feature block][lane][4]) so both the store and the reload are fully
// coalesced 1 KiB wave transactions.
#include <hip/hip_runtime.h>
#include <map>
#include <type_traits>
#include <utility>
#include <tuple>
#include <mutex>
#include "common.h"
#include "../../include/nesvor_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWidth = 64;      // hidden width (the reference's default and BASELINE's config)
constexpr int kHB = kWidth / 16;  // feature blocks per hidden layer
constexpr int kG = 2;  // 16-sample groups per wave per tile; 2 keeps the kernels under 128 VGPRs (>= 4 waves/SIMD); the % (4 * kG) gates assume it
constexpr int kMaxLayers = NESVOR_MAX_MLP_LAYERS;  // linear layers incl. the output layer

struct MlpArgs {
  const float* W[kMaxLayers];   // nn.Linear weights, (out, in) row-major
  const float* b[kMaxLayers];   // biases (out)
  float* H[kMaxLayers];         // saved hidden fragments per hidden layer (fwd: out, bwd: in); may be null in fwd
  float* dpre[kMaxLayers];      // bwd: grad w.r.t. pre-activation of each hidden layer, fragment layout
  const float* xa;              // pixel features (P, k_a) or null
  const float* xb;              // feature-major matrix (rows, N)
  float* y;                     // fwd: output (out_dim, N) feature-major;  bwd: dY (out_dim, N) (read)
  float* dxa;                   // bwd: (N, k_a) per-sample grad of the pixel features, or null
  float* dxb;                   // bwd: (k_b, N) feature-major grad of the matrix rows, or null
  float* dW_partial;            // dW kernel: (n_wg, total_params) partial sums
  int64_t N;
  int n_linear;                 // n_hidden + 1
  int k_a, k_b, b_row0;         // input composition
  int out_dim;                  // <= 16
  int S;                        // samples per pixel (pixel = n / S)
  int total_params;             // sum of W and b sizes (dW partial row length)
  int fast;                     // N % 16 == 0, S % 16 == 0, k_a % 16 == 0: group = one pixel, input blocks homogeneous
  int spg_shift;                // log2(S / 16) when that is a power of two, else -1
  int dxa_group;                // dxa holds one row per 16-sample GROUP (sum over its samples) instead of one per sample
  int half16;                   // with bf16 == 1: the 16-bit operand type is fp16, not bf16 (nesvor_mlp_t.bf16_operands == 3)
  int bf16;                     // 1: matrix operands rounded to bf16 (fp32 accumulation); 2: every operand split into two fp16 of a power-of-two-scaled copy (split mode, see below)
  int hi1;                      // with bf16 == 2: only the first term of the split (nesvor_mlp_t.bf16_operands == 4: power-of-two-scaled operands rounded to fp16, ONE MFMA per product)
  int off32;                    // every row of xb / y starts below 2^32 bytes: lane offsets fit the 32-bit VGPR offset of scalar-base loads
  uint32_t* Hm;                 // compact save (nesvor_mlp_t.compact_save): one word per (group, lane), bit 16 l + 4 b + r = [h_l > 0]
  float* dx_absmax;             // bwd, optional: device scalar raised (atomic max) to max |dxb| - the consumer of dxb (the hash-grid
                                // backward) scales its fixed-point sums by it instead of reading dxb an extra time
  const float* prep;            // split mode: operand bounds and weight norms of this launch (nesvor_mlp_t.prep; see MlpScales)
  float* y_absmax;              // fwd, optional: slotted bound raised to max |y| (the next network's input bound)
  const _Float16* wimg;         // split mode, optional: the operand images of all layers, prebuilt for the current weights (nesvor_mlp_t.weight_images)
};

// max |dx| over the xb blocks of a lane's dX fragments, folded into `mx`
template <int KB1>
__device__ __forceinline__ void track_absmax(const MlpArgs& a, const f32x4 (&dx)[KB1], float& mx) {
  const int ka_blocks = a.k_a >> 4;
#pragma unroll
  for (int kb = 0; kb < KB1; ++kb)
    if (kb >= ka_blocks) {
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, fabsf(dx[kb][r]));
    }
}
__device__ __forceinline__ void publish_absmax(const MlpArgs& a, float mx) {
  mx = wave_max(mx);  // rows beyond k_b hold exact zeros (zero weight columns): they cannot raise the maximum
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(reinterpret_cast<unsigned int*>(a.dx_absmax), __float_as_uint(mx));
}

// ReLU as an integer max: negative floats (and -0) are negative integers.  fmaxf() compiles to TWO instructions
// (v_max_f32 x, x to quiet a signalling NaN, then the max), this is one.
__device__ __forceinline__ float relu_f(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Optional mixed-precision mode (nesvor_mlp_t.bf16_operands): the matrix operands - weights, activations, upstream
// gradients - are rounded to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) and multiplied by
// v_mfma_f32_16x16x16_bf16 with fp32 accumulation; master weights, biases, ReLU and outputs stay fp32.  The saved
// hidden activations are stored as bf16 (same fragment layout, 8 bytes per lane): they are only ever used as bf16
// operands or as ReLU masks, so nothing is lost and the largest HBM stream of the MLPs halves.  One bf16 MFMA contracts the same 16 k-values as four fp32 16x16x4 MFMAs with the same lane
// maps (k = 4 (lane >> 4) + r), at 1/16 of their matrix-pipe time.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x4 pack_bf16(const f32x4& v) {
  // two v_cvt_pk_bf16_f32 (converting the four-vector at once is scalarised where a half of the result is used on its own:
  // four conversions with an undefined second source plus two v_perm_b32)
  const bf16x2_t a = __builtin_convertvector(f32x2{v[0], v[1]}, bf16x2_t), b = __builtin_convertvector(f32x2{v[2], v[3]}, bf16x2_t);
  return __builtin_bit_cast(s16x4, __builtin_shufflevector(a, b, 0, 1, 2, 3));
}
__device__ __forceinline__ f32x4 mfma16_bf16(s16x4 a, s16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
// The 16-bit operand modes share every kernel: HT = 1 rounds the matrix operands to bf16 (nesvor_mlp_t.bf16_operands == 1),
// HT = 2 to fp16 (mode 3, round 6: the reference's default arithmetic - fp16 CutlassMLP, nesvor/nesvor/models.py:28-41 - whose
// narrow exponent range is what its GradScaler exists for, train.py:161-164).  Same lane maps, same instruction shapes, fp32
// accumulation; an operand beyond 65504 becomes inf in fp16 and poisons the step - which the loss scaler then skips.
typedef _Float16 h16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2_t __attribute__((ext_vector_type(2)));
template <int HT>
__device__ __forceinline__ s16x4 pack16(const f32x4& v) {
  if constexpr (HT == 2) {
    const h16x2_t a = __builtin_convertvector(f32x2{v[0], v[1]}, h16x2_t), b = __builtin_convertvector(f32x2{v[2], v[3]}, h16x2_t);
    return __builtin_bit_cast(s16x4, __builtin_shufflevector(a, b, 0, 1, 2, 3));
  } else {
    return pack_bf16(v);
  }
}
template <int HT>
__device__ __forceinline__ f32x4 mfma16h(s16x4 a, s16x4 b, f32x4 c) {
  if constexpr (HT == 2) return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h16x4_t, a), __builtin_bit_cast(h16x4_t, b), c, 0, 0, 0);
  else return mfma16_bf16(a, b, c);
}
template <int HT>
__device__ __forceinline__ void store16(float* img, int e, float w) {
  if constexpr (HT == 2) reinterpret_cast<_Float16*>(img)[e] = (_Float16)w;
  else reinterpret_cast<__bf16*>(img)[e] = (__bf16)w;
}
template <int HT>
__device__ __forceinline__ float widen16(uint32_t low16) {  // a 16-bit operand (zero-extended in a register) as fp32
  if constexpr (HT == 2) return (float)__builtin_bit_cast(_Float16, (unsigned short)low16);
  else return __uint_as_float(low16 << 16);
}

// Split mode (nesvor_mlp_t.bf16_operands == 2), round 5: every fp32 operand x is written as TWO fp16 numbers of a scaled copy,
//     x s = hi + lo,   hi = rn_f16(x s),   lo = rn_f16(x s - hi)       (both round-to-nearest: |x s - hi - lo| <= 2^-24 |x s|)
// with s a power of two chosen PER LAUNCH and per operand tensor such that a bound on the tensor maps into [2^13, 2^14) - fp16
// then resolves every value above 2^-17 of the bound to 22-24 bits and the rest to an absolute 2^-38 of the bound - and a product
// a b is evaluated as the three fp16 MFMAs  a_lo b_hi + a_hi b_lo + a_hi b_hi  with fp32 accumulation (the dropped a_lo b_lo is
// below 2^-23 |a||b|).  Measured on the device (tools/f16_split_probe.hip, profiles/r05_f16_split_probe.log): the error of a
// 64-term product against fp64 is BELOW that of the fp32 MFMA chain on all three operand families tried (2.1e-7 against 3.6e-7
// of the largest result for N(0,1) operands; 3.4e-7 against 4.2e-7 with a dynamic range of e^3 per row), the f16 shape issues at
// the bf16 shape's rate, fp16 subnormals are honoured by the matrix pipe, and a block of 24 MFMAs + 12 splits takes 1.33 us
// where rounds 2-4's three-way bf16 split (six terms) took 2.15 us for the same products.
// The bounds come from the caller (nesvor_mlp_t.prep: max |input|, max |dY| and per layer max |W|, the largest row / column L1
// norms of W and max |b|, all device scalars - nesvor_mlp_prepare computes them, the training step lets the producing kernels
// publish them) and propagate through the layers as |W x + b| <= ||W||_inf max|x| + max|b|: every scale is a wave-uniform
// constant of the launch, the bias enters pre-scaled as the accumulators' initial value, ReLU and the gate bits do not care
// about a positive scale, and the scale of a layer's output folds into the multiplier of the next split - no per-value work
// besides the split itself (8 VALU per four values, v_fma_mixlo/hi_f16: the scale rides in the conversion) and one multiply
// per OUTPUT value.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
struct Split2 { s16x4 hi, lo; };
// (plain asm, not volatile: a pure function of its inputs - the scheduler may move and merge it; `m` is wave-uniform)
__device__ __forceinline__ Split2 split2(const f32x4& v, float m) {
  uint32_t h0, h1, l0, l1;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h0) : "v"(v[0]), "s"(m));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h0) : "v"(v[1]), "s"(m));
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h1) : "v"(v[2]), "s"(m));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h1) : "v"(v[3]), "s"(m));
  // x m - hi is exact in fp32 (hi is within 2^-11 of x m): ONE rounding, to fp16
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(l0) : "v"(v[0]), "s"(m), "v"(h0));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l0) : "v"(v[1]), "s"(m), "v"(h0));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(l1) : "v"(v[2]), "s"(m), "v"(h1));
  // (s_nop 1 below: a VALU result must be two wait states old before a matrix instruction reads it, and the hazard recogniser does
  //  not see writes made by inline asm - see split2m().  The statements of a split are scheduled one by one, so the wait states sit in
  //  a statement of their own that "redefines" all four results: every consumer is ordered behind it, it behind every write.  17 sites
  //  of the round-5 build had a v_fma_mix*, one s_waitcnt and the consuming MFMA in a row - the headline density forward among them;
  //  tools/check_inflight_loads.py::check_asm_valu_mfma now holds every site to the rule.)
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l1) : "v"(v[3]), "s"(m), "v"(h1));
  asm("s_nop 1" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));  // (every consumer of the four results sits behind this statement)
  Split2 r;
  r.hi = __builtin_bit_cast(s16x4, uint2{h0, h1});
  r.lo = __builtin_bit_cast(s16x4, uint2{l0, l1});
  return r;
}
// Mode 4 (HI1): the leading term alone.  A VALU write of a VGPR must be TWO wait states old before a matrix instruction reads that
// register; the compiler's hazard recogniser inserts them for instructions it emits, but it cannot see a write made by inline asm.
// The full split is safe by construction - its last writes are the low halves, which no product reads first - but with the low half
// dead the last v_fma_mixhi_f16 sits right in front of the MFMA that consumes it: found as run-to-run differences of ONE weight-gradient
// block in one instantiation (tools/diag_fp16s_repro.py: 6 of 19 runs; a single s_nop in between: 0 of 200).  The wait states therefore
// sit in an asm statement behind the writes that every consumer depends on, and the build's assembly check knows the rule
// (tools/check_inflight_loads.py: v_fma_mix* / v_bfe_i32 results read by v_mfma* fewer than two wait states later).
template <bool HI1>
__device__ __forceinline__ Split2 split2m(const f32x4& v, float m) {
  if constexpr (!HI1) {
    return split2(v, m);
  } else {
    uint32_t h0, h1;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h0) : "v"(v[0]), "s"(m));
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h1) : "v"(v[2]), "s"(m));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h0) : "v"(v[1]), "s"(m));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h1) : "v"(v[3]), "s"(m));
    asm("s_nop 1" : "+v"(h0), "+v"(h1));
    Split2 r;
    r.hi = __builtin_bit_cast(s16x4, uint2{h0, h1});
    r.lo = r.hi;  // (never read: the HI1 paths take the leading term only)
    return r;
  }
}
// gfx950's full-rate 16-bit shapes contract 32 k-values per instruction: lane (j, q) supplies k-slots (q, 0..7).  The
// k index may be numbered freely as long as A and B agree, so slots 0..3 take the lane's four values of one 16-feature
// block and slots 4..7 those of the next block: two of the kernels' fragments side by side, no data movement.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 join8(const s16x4& a, const s16x4& b) {
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ f32x4 mfma32_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
typedef _Float16 h16x8_t __attribute__((ext_vector_type(8)));
template <int HT>
__device__ __forceinline__ f32x4 mfma32h(bf16x8 a, bf16x8 b, f32x4 c) {  // (operands carried as 8 x 16 raw bits; HT names their type)
  if constexpr (HT == 2) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8_t, a), __builtin_bit_cast(h16x8_t, b), c, 0, 0, 0);
  else return mfma32_bf16(a, b, c);
}
__device__ __forceinline__ f16x8 join8h(const s16x4& a, const s16x4& b) {
  return __builtin_bit_cast(f16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ f32x4 mfma32_f16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16_f16(s16x4 a, s16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
}
// one 16-k block (an odd last block): the three terms, smallest first (HI1: the leading term alone - see kernels' SPL == 2)
template <bool HI1 = false>
__device__ __forceinline__ f32x4 mfma_split(const Split2& a, const Split2& b, f32x4 c) {
  if constexpr (!HI1) {
    c = mfma16_f16(a.lo, b.hi, c);
    c = mfma16_f16(a.hi, b.lo, c);
  }
  return mfma16_f16(a.hi, b.hi, c);
}

// Scales of one launch in the split mode (all powers of two, wave-uniform; `prep` as nesvor_mlp_t.prep):
//   sx[l]  input of linear layer l (l = 0: the network input, l >= 1: the post-ReLU activations of hidden layer l - 1)
//   sw[l]  W_l (both the forward and the transposed images)
//   sd[l]  backward: d pre-activation of hidden layer l (l < n_hidden); sd[n_hidden] = the upstream gradient dY
// Accumulator units: forward layer l: sw[l] sx[l];  backward product W_{l+1}^T d_{l+1}: sw[l+1] sd[l+1];  dW_l: sd[l] sx[l].
struct MlpScales {
  float sx[kMaxLayers + 1], sw[kMaxLayers], sd[kMaxLayers + 1];
};
__device__ __forceinline__ float uniform_f(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
// the power of two s with bound * s in [2^14, 2^15) (fp16 overflows at 65504), clamped to [2^-40, 2^40] (products and ratios of two scales stay finite)
__device__ __forceinline__ float pow2_scale(float bound) {
  const int e = (int)((__float_as_uint(bound) >> 23) & 0xFFu) - 126;  // bound = m 2^e, m in [0.5, 1); zero / subnormal: e = -126
  const int se = min(max(15 - e, -40), 40);
  return uniform_f(__uint_as_float((uint32_t)(se + 127) << 23));
}
__device__ __forceinline__ float pow2_inv(float p) {  // 1 / p for a power of two p in the clamped range: exact
  return uniform_f(__uint_as_float((254u << 23) - __float_as_uint(p)));
}
__device__ __forceinline__ MlpScales mlp_scales(const float* __restrict__ prep, int n_hidden, bool has_a, bool backward) {
  MlpScales s;
  float bound = absmax_slots(prep + NESVOR_MLP_PREP_XB);
  if (has_a) bound = fmaxf(bound, absmax_slots(prep + NESVOR_MLP_PREP_XA));
#pragma unroll
  for (int l = 0; l < kMaxLayers; ++l) {
    s.sx[l] = 1.f; s.sw[l] = 1.f; s.sd[l] = 1.f;
    if (l <= n_hidden) {
      const float* nl = prep + NESVOR_MLP_PREP_LAYER0 + 4 * l;
      s.sx[l] = pow2_scale(bound);
      s.sw[l] = pow2_scale(nl[0]);
      bound = fmaf(nl[1], bound, nl[3]) * 1.0001f;  // |W x + b| <= ||W||_inf max |x| + max |b|
    }
  }
  s.sx[kMaxLayers] = 1.f; s.sd[kMaxLayers] = 1.f;
  if (backward) {
    float g = absmax_slots(prep + NESVOR_MLP_PREP_DY);
#pragma unroll
    for (int l = kMaxLayers - 1; l >= 0; --l) {
      if (l == n_hidden) s.sd[l] = pow2_scale(g);
      if (l < n_hidden) {
        g = prep[NESVOR_MLP_PREP_LAYER0 + 4 * (l + 1) + 2] * g * 1.0001f;  // |W^T d| <= max column L1 norm of W times max |d|
        s.sd[l] = pow2_scale(g);
      }
    }
  }
  return s;
}

// ---------------------------------------------------------------- LDS images
// forward image of a layer with `ob_n` output blocks and `kb_n` input blocks
// (BF16: the image holds bf16 elements at the same element indices, i.e. it uses the first half of the fp32 carve)
template <int BF16 = 0>
__device__ void build_image(float* img, const float* __restrict__ W, int out_dim, int in_dim, int ob_n, int kb_n) {
  const int total = ob_n * kb_n * 256;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int r = e & 3, lane = (e >> 2) & 63, blk = e >> 8;
    const int kb = blk % kb_n, ob = blk / kb_n;
    const int o = 16 * ob + (lane & 15), k = 16 * kb + 4 * (lane >> 4) + r;
    const float w = (o < out_dim && k < in_dim) ? W[(size_t)o * in_dim + k] : 0.f;
    if constexpr (BF16) store16<BF16>(img, e, w);
    else img[e] = w;
  }
}
// transposed image: rows i = input features (ib blocks), k = output features (kb blocks)
template <int BF16 = 0>
__device__ void build_image_T(float* img, const float* __restrict__ W, int out_dim, int in_dim, int ib_n, int kb_n) {
  const int total = ib_n * kb_n * 256;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int r = e & 3, lane = (e >> 2) & 63, blk = e >> 8;
    const int kb = blk % kb_n, ib = blk / kb_n;
    const int in = 16 * ib + (lane & 15), o = 16 * kb + 4 * (lane >> 4) + r;
    const float w = (o < out_dim && in < in_dim) ? W[(size_t)o * in_dim + in] : 0.f;
    if constexpr (BF16) store16<BF16>(img, e, w);
    else img[e] = w;
  }
}

// The same two images with compile-time shapes (no run-time division per element) and the global loads of eight elements
// per thread in flight at once: the generic builders above walk one dependent load per iteration - 27 to 42 L2 round trips per
// thread before the first tile, 6-11 us of every launch of the pipelined forward (measured with the builds compiled out).
// T: transposed image (build_image_T); A_N / B_N = (ob_n, kb_n) or (ib_n, kb_n) of the generic versions.
// SPL: two fp16 planes hi | lo of `total` elements each of W * scale (split2's arithmetic) - the size of the fp32 carve.
template <int BF16, bool SPL, bool T, int A_N, int B_N, int THREADS>
__device__ __forceinline__ void build_image_ct(float* img, const float* __restrict__ W, int out_dim, int in_dim, float scale = 1.f) {
  constexpr int total = A_N * B_N * 256;
  constexpr int U = 8;
  for (int e0 = threadIdx.x; e0 < total; e0 += THREADS * U) {
    float w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * THREADS;
      const int r = e & 3, lane = (e >> 2) & 63, blk = e >> 8;
      const int kb = blk % B_N, ab = blk / B_N;
      const int row = 16 * ab + (lane & 15), col = 16 * kb + 4 * (lane >> 4) + r;  // T: row = input feature, col = output feature
      const int o = T ? col : row, k = T ? row : col;
      const bool ok = e < total && o < out_dim && k < in_dim;
      w[u] = W[ok ? (size_t)o * in_dim + k : 0];  // (every load issued, no branch: zero-filled below)
      w[u] = ok ? w[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * THREADS;
      if (e < total) {
        if constexpr (SPL) {
          _Float16* p = reinterpret_cast<_Float16*>(img);
          const float ws = w[u] * scale;
          const _Float16 hi = (_Float16)ws;
          p[e] = hi; p[total + e] = (_Float16)(ws - (float)hi);
        } else if constexpr (BF16) store16<BF16>(img, e, w[u]);
        else img[e] = w[u];
      }
    }
  }
}

// Prebuilt operand images (nesvor_mlp_t.weight_images, round 6).  Every launch of the split mode used to build its LDS images from
// the fp32 weights - a few dependent L2 round trips plus the splitting of every element, per workgroup.  The training step now
// builds them ONCE per iteration - in the launch that takes the weight norms, which has each layer's matrix in LDS and knows its
// scale - and a workgroup copies them: 16-byte loads, all of a thread's in flight at once, no arithmetic.  Measured in the step
// (in-job A/B, profiles/r06_mlp_image_build.log): the four MLP launches -3.4 us of 129 us at 2^17
// points per iteration, within noise at 2^20 (the builds had been brought down to ~1 us per launch in round 4; an ablation
// with the builds compiled out had suggested 30 us - it trains on garbage images, the poses turn NaN and
// every kernel of that step gets faster for reasons that have nothing to do with the builds).  Layout of a network's buffer, in fp16 elements, layer
// after layer (l = 0 .. n_hidden):   [F hi | F lo | T hi | T lo],  each plane E_l = (output blocks) x (input blocks) x 256 elements,
// F = the forward image (build_image_ct<.., T = false, output blocks, input blocks>), T = the transposed one (T = true, input
// blocks, output blocks); blocks: KB1 for the network input, kHB for a hidden layer, 1 for the output.  An LDS image of the split
// mode is [hi plane | lo plane] = one contiguous range of this buffer.
__host__ __device__ constexpr int wimg_plane(int n_hidden, int kb1, int l) {
  return (l == n_hidden ? 1 : kHB) * (l == 0 ? kb1 : kHB) * 256;
}
__host__ __device__ constexpr int wimg_offset(int n_hidden, int kb1, int l) {  // first element of layer l's F image
  int off = 0;
  for (int t = 0; t < l; ++t) off += 4 * wimg_plane(n_hidden, kb1, t);
  return off;
}
// LDS image <- FLOATS fp32-sized words of a prebuilt image: all loads of a thread issued before the first LDS store
template <int FLOATS, int THREADS>
__device__ __forceinline__ void copy_image_ct(float* __restrict__ dst, const _Float16* __restrict__ src) {
  static_assert(FLOATS % 4 == 0, "images are whole 16-byte vectors");
  constexpr int V = FLOATS / 4, PER = (V + THREADS - 1) / THREADS;
  const float4* s4 = reinterpret_cast<const float4*>(src);
  float4 v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int i = (int)threadIdx.x + u * THREADS; v[u] = s4[i < V ? i : 0]; }
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int i = (int)threadIdx.x + u * THREADS; if (i < V) reinterpret_cast<float4*>(dst)[i] = v[u]; }
}

// y[g][ob] (+)= img . x   for G groups at once; KB input blocks, OB output blocks
// SPL: `mult` = (scale of this layer's B operand) / (units x arrives in); y accumulates in units sw sx (MlpScales)
// SPL: 0 off, 1 the two-way split (three terms), 2 its leading term alone (scaled fp16 operands, one MFMA per product: mode 4)
template <int KB, int OB, int BF16 = 0, int SPL = 0>
__device__ __forceinline__ void apply_layer(const float* __restrict__ img, const f32x4 (&x)[kG][KB], f32x4 (&y)[kG][OB],
                                            int lane, float mult = 1.f) {
  if constexpr (SPL != 0) {
    constexpr bool HI1 = SPL == 2;
    const _Float16* img16 = reinterpret_cast<const _Float16*>(img);
    constexpr int plane = OB * KB * 256;
    auto load_a = [&](int ob, int kb) __attribute__((always_inline)) {
      const _Float16* pa = img16 + ((ob * KB + kb) * 64 + lane) * 4;
      Split2 a;
      a.hi = *reinterpret_cast<const s16x4*>(pa);
      a.lo = *reinterpret_cast<const s16x4*>(pa + plane);
      return a;
    };
    // Three MFMAs accumulate into one fragment; issued back to back they wait for one another (a dependent MFMA
    // issues ~1.5-2x later than an independent one).  The terms are therefore walked in the outer loop and the
    // independent accumulators (two output blocks x kG groups) in the inner one; every accumulator still receives
    // its terms in the same order, smallest first.
#pragma unroll
    for (int kb = 0; kb + 1 < KB; kb += 2) {
      f16x8 bh[kG], bl[kG];
#pragma unroll
      for (int g = 0; g < kG; ++g) {
        const Split2 p0 = split2m<HI1>(x[g][kb], mult), p1 = split2m<HI1>(x[g][kb + 1], mult);
        bh[g] = join8h(p0.hi, p1.hi); bl[g] = join8h(p0.lo, p1.lo);
      }
#pragma unroll
      for (int ob = 0; ob < OB; ob += 2) {
        constexpr int kPair = OB >= 2 ? 2 : 1;
        f16x8 ah[kPair], al[kPair];
#pragma unroll
        for (int o = 0; o < kPair; ++o) {
          const Split2 a0 = load_a(ob + o, kb), a1 = load_a(ob + o, kb + 1);
          ah[o] = join8h(a0.hi, a1.hi); al[o] = join8h(a0.lo, a1.lo);
        }
#define NESVOR_TERM(A, B)                                                                       \
  _Pragma("unroll") for (int o = 0; o < kPair; ++o)                                             \
    _Pragma("unroll") for (int g = 0; g < kG; ++g) y[g][ob + o] = mfma32_f16(A[o], B[g], y[g][ob + o]);
        if constexpr (!HI1) { NESVOR_TERM(al, bh) NESVOR_TERM(ah, bl) }
        NESVOR_TERM(ah, bh)
#undef NESVOR_TERM
      }
    }
    if constexpr (KB % 2 == 1) {
      constexpr int kb = KB - 1;
      Split2 pb[kG];
#pragma unroll
      for (int g = 0; g < kG; ++g) pb[g] = split2m<HI1>(x[g][kb], mult);
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) {
        const Split2 a = load_a(ob, kb);
#pragma unroll
        for (int g = 0; g < kG; ++g) y[g][ob] = mfma_split<HI1>(a, pb[g], y[g][ob]);
      }
    }
    return;
  }
  if constexpr (BF16) {
    const __bf16* img16 = reinterpret_cast<const __bf16*>(img);
    // two 16-feature blocks per full-rate 16x16x32 MFMA (see join8), a 16x16x16 one for an odd last block
#pragma unroll
    for (int kb = 0; kb + 1 < KB; kb += 2) {
      bf16x8 pb[kG];
#pragma unroll
      for (int g = 0; g < kG; ++g) pb[g] = join8(pack16<BF16>(x[g][kb]), pack16<BF16>(x[g][kb + 1]));
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) {
        const bf16x8 a = join8(*reinterpret_cast<const s16x4*>(img16 + ((ob * KB + kb) * 64 + lane) * 4),
                               *reinterpret_cast<const s16x4*>(img16 + ((ob * KB + kb + 1) * 64 + lane) * 4));
#pragma unroll
        for (int g = 0; g < kG; ++g) y[g][ob] = mfma32h<BF16>(a, pb[g], y[g][ob]);
      }
    }
    if constexpr (KB % 2 == 1) {
      constexpr int kb = KB - 1;
      s16x4 pb[kG];
#pragma unroll
      for (int g = 0; g < kG; ++g) pb[g] = pack16<BF16>(x[g][kb]);
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) {
        const s16x4 a = *reinterpret_cast<const s16x4*>(img16 + ((ob * KB + kb) * 64 + lane) * 4);
#pragma unroll
        for (int g = 0; g < kG; ++g) y[g][ob] = mfma16h<BF16>(a, pb[g], y[g][ob]);
      }
    }
    return;
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(img + ((ob * KB + kb) * 64 + lane) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int g = 0; g < kG; ++g) y[g][ob] = mfma4(a[r], x[g][kb][r], y[g][ob]);
    }
  }
}

// single 16-sample group variant (used by the fused backward, where registers hold the dW accumulators)
// Split-mode layer product on operands that are already split (the chain waves of the wave-specialised backward split a
// fragment once, for this product AND for the planes they hand to the dW waves).
template <int KB, int OB, bool ZERO = false, bool HI1 = false>
__device__ __forceinline__ void apply_layer_g1_s(const float* __restrict__ img, const Split2 (&xs)[KB], f32x4 (&y)[OB], int lane) {
  const _Float16* img16 = reinterpret_cast<const _Float16*>(img);
  constexpr int plane = OB * KB * 256;
  auto load_a = [&](int ob, int kb) __attribute__((always_inline)) {
    const _Float16* pa = img16 + ((ob * KB + kb) * 64 + lane) * 4;
    Split2 a;
    a.hi = *reinterpret_cast<const s16x4*>(pa);
    a.lo = *reinterpret_cast<const s16x4*>(pa + plane);
    return a;
  };
  // term-major over the OB independent accumulators (see apply_layer).  The weight planes of a k-block pair are read from
  // LDS while the activations of that pair are being split, not right in front of the first product that needs them.
  auto load_pair = [&](int kb, f16x8 (&ah)[OB], f16x8 (&al)[OB]) __attribute__((always_inline)) {
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      const Split2 a0 = load_a(ob, kb), a1 = load_a(ob, kb + 1);
      ah[ob] = join8h(a0.hi, a1.hi); al[ob] = join8h(a0.lo, a1.lo);
    }
  };
  f16x8 ah[OB], al[OB];
  if constexpr (KB >= 2) {
    load_pair(0, ah, al);
    __builtin_amdgcn_sched_barrier(0x047F);  // LDS reads stay above, everything else may cross
  }
#pragma unroll
  for (int kb = 0; kb + 1 < KB; kb += 2) {
    const Split2 &p0 = xs[kb], &p1 = xs[kb + 1];
    const f16x8 bh = join8h(p0.hi, p1.hi), bl = join8h(p0.lo, p1.lo);
    f16x8 nh[OB], nl[OB];
    const bool more = kb + 3 < KB;
#define NESVOR_TERM(A, B) _Pragma("unroll") for (int ob = 0; ob < OB; ++ob) y[ob] = mfma32_f16(A[ob], B, y[ob]);
    if constexpr (HI1) {  // the leading term alone
      if (ZERO && kb == 0) {
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) y[ob] = mfma32_f16(ah[ob], bh, f32x4{0.f, 0.f, 0.f, 0.f});
      } else {
        NESVOR_TERM(ah, bh)
      }
    } else {
      if (ZERO && kb == 0) {
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) y[ob] = mfma32_f16(al[ob], bh, f32x4{0.f, 0.f, 0.f, 0.f});
      } else {
        NESVOR_TERM(al, bh)
      }
      NESVOR_TERM(ah, bl) NESVOR_TERM(ah, bh)
    }
#undef NESVOR_TERM
    if (more) {
      load_pair(kb + 2, nh, nl);
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) { ah[ob] = nh[ob]; al[ob] = nl[ob]; }
    }
  }
  if constexpr (KB % 2 == 1) {
    const Split2& pb = xs[KB - 1];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) y[ob] = mfma_split<HI1>(load_a(ob, KB - 1), pb, (ZERO && KB == 1) ? f32x4{0.f, 0.f, 0.f, 0.f} : y[ob]);
  }
}

// ZERO (split mode): y is an output, not an accumulator - the first term of every block product takes a literal zero as its C
// operand instead of OB x 4 registers the caller would have to clear.
template <int KB, int OB, int BF16 = 0, int SPL = 0, bool ZERO = false>
__device__ __forceinline__ void apply_layer_g1(const float* __restrict__ img, const f32x4 (&x)[KB], f32x4 (&y)[OB], int lane, float mult = 1.f) {
  static_assert(!ZERO || SPL != 0, "ZERO: split mode only");
  if constexpr (SPL != 0) {
    Split2 xs[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) xs[kb] = split2m<SPL == 2>(x[kb], mult);
    apply_layer_g1_s<KB, OB, ZERO, SPL == 2>(img, xs, y, lane);
    return;
  }
  if constexpr (BF16) {
    const __bf16* img16 = reinterpret_cast<const __bf16*>(img);
#pragma unroll
    for (int kb = 0; kb + 1 < KB; kb += 2) {
      const bf16x8 pb = join8(pack16<BF16>(x[kb]), pack16<BF16>(x[kb + 1]));
#pragma unroll
      for (int ob = 0; ob < OB; ++ob)
        y[ob] = mfma32h<BF16>(join8(*reinterpret_cast<const s16x4*>(img16 + ((ob * KB + kb) * 64 + lane) * 4),
                                  *reinterpret_cast<const s16x4*>(img16 + ((ob * KB + kb + 1) * 64 + lane) * 4)), pb, y[ob]);
    }
    if constexpr (KB % 2 == 1) {
      const s16x4 pb = pack16<BF16>(x[KB - 1]);
#pragma unroll
      for (int ob = 0; ob < OB; ++ob)
        y[ob] = mfma16h<BF16>(*reinterpret_cast<const s16x4*>(img16 + ((ob * KB + KB - 1) * 64 + lane) * 4), pb, y[ob]);
    }
    return;
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    f32x4 a[OB];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) a[ob] = *reinterpret_cast<const f32x4*>(img + ((ob * KB + kb) * 64 + lane) * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) y[ob] = mfma4(a[ob][r], x[kb][r], y[ob]);
  }
}

// The same layer product with the operand roles exchanged: D = X . W^T, rows = the 16 samples of the group, columns = the
// output features of a block - lane (feature j, sample quad q) ends up with feature 16 ob + j of samples 4q .. 4q+3, which is
// the B-operand layout of the weight-gradient products.  x: the group's input in the chain layout (lane (sample j, q):
// features 16 kb + 4q + r), img: the FORWARD image of the layer (its fragments serve as B operands unchanged: both operand
// layouts index the lane by the non-contracted dimension).  Same terms in the same order as apply_layer; `mult` as there.
template <int KB, int OB>
__device__ __forceinline__ void apply_layer_g1_T(const float* __restrict__ img, const f32x4 (&x)[KB], f32x4 (&y)[OB], int lane, float mult) {
  const _Float16* img16 = reinterpret_cast<const _Float16*>(img);
  constexpr int plane = OB * KB * 256;
  auto load_w = [&](int ob, int kb) __attribute__((always_inline)) {
    const _Float16* pa = img16 + ((ob * KB + kb) * 64 + lane) * 4;
    Split2 w;
    w.hi = *reinterpret_cast<const s16x4*>(pa);
    w.lo = *reinterpret_cast<const s16x4*>(pa + plane);
    return w;
  };
#pragma unroll
  for (int kb = 0; kb + 1 < KB; kb += 2) {
    const Split2 p0 = split2(x[kb], mult), p1 = split2(x[kb + 1], mult);
    const f16x8 xh = join8h(p0.hi, p1.hi), xl = join8h(p0.lo, p1.lo);
#pragma unroll
    for (int ob = 0; ob < OB; ob += 2) {  // two independent accumulators at a time (a dependent MFMA issues later)
      constexpr int kPair = OB >= 2 ? 2 : 1;
      f16x8 wh[kPair], wl[kPair];
#pragma unroll
      for (int o = 0; o < kPair; ++o) {
        const Split2 w0 = load_w(ob + o, kb), w1 = load_w(ob + o, kb + 1);
        wh[o] = join8h(w0.hi, w1.hi); wl[o] = join8h(w0.lo, w1.lo);
      }
#define NESVOR_TERM(XP, WP) _Pragma("unroll") for (int o = 0; o < kPair; ++o) y[ob + o] = mfma32_f16(XP, WP[o], y[ob + o]);
      NESVOR_TERM(xh, wl) NESVOR_TERM(xl, wh) NESVOR_TERM(xh, wh)
#undef NESVOR_TERM
    }
  }
  if constexpr (KB % 2 == 1) {
    const Split2 px = split2(x[KB - 1], mult);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      const Split2 w = load_w(ob, KB - 1);
      f32x4 c = y[ob];
      c = mfma16_f16(px.hi, w.lo, c);
      c = mfma16_f16(px.lo, w.hi, c);
      y[ob] = mfma16_f16(px.hi, w.hi, c);
    }
  }
}

__device__ __forceinline__ float fetch_input(const MlpArgs& a, int kk, int64_t n) {
  if (kk < a.k_a) return a.xa[(size_t)(n / a.S) * a.k_a + kk];
  const int kb_ = kk - a.k_a;
  if (kb_ < a.k_b) return a.xb[(size_t)(a.b_row0 + kb_) * a.N + n];
  return 0.f;
}

// Fast input path (a.fast): the 16 samples of group `gi` belong to one pixel and every 16-feature input block is
// either all pixel features (one 16-byte load per lane, no per-element index arithmetic) or all rows of xb.
template <int KB1>
__device__ __forceinline__ void load_x_fast(const MlpArgs& a, int64_t gi, int j, int q, f32x4 (&x)[KB1]) {
  const int ka_blocks = a.k_a >> 4;
  const int64_t n = gi * 16 + j;
#pragma unroll
  for (int kb = 0; kb < KB1; ++kb) {
    if (kb < ka_blocks) {
      const int64_t pixel = a.spg_shift >= 0 ? (gi >> a.spg_shift) : gi / (a.S >> 4);
      x[kb] = *reinterpret_cast<const f32x4*>(a.xa + (size_t)pixel * a.k_a + 16 * kb + 4 * q);
    } else {
      const int row0 = 16 * (kb - ka_blocks) + 4 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + r;
        const float v = a.xb[(size_t)(a.b_row0 + min(row, a.k_b - 1)) * a.N + n];
        x[kb][r] = row < a.k_b ? v : 0.f;
      }
    }
  }
}
template <int KB1>
__device__ __forceinline__ void store_dx_fast(const MlpArgs& a, int64_t gi, int j, int q, const f32x4 (&dx)[KB1]) {
  const int ka_blocks = a.k_a >> 4;
  const int64_t n = gi * 16 + j;
#pragma unroll
  for (int kb = 0; kb < KB1; ++kb) {
    if (kb < ka_blocks) {
      if (a.dxa != nullptr) {
        if (a.dxa_group) {  // the group lies inside one pixel: reduce its 16 samples here, 16x less to write and re-read
          f32x4 sgrp;
#pragma unroll
          for (int r = 0; r < 4; ++r) sgrp[r] = row_sum_dpp(dx[kb][r]);
          if (j == 0) *reinterpret_cast<f32x4*>(a.dxa + (size_t)gi * a.k_a + 16 * kb + 4 * q) = sgrp;
        } else {
          *reinterpret_cast<f32x4*>(a.dxa + (size_t)n * a.k_a + 16 * kb + 4 * q) = dx[kb];
        }
      }
    } else if (a.dxb != nullptr) {
      const int row0 = 16 * (kb - ka_blocks) + 4 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row0 + r < a.k_b) a.dxb[(size_t)(row0 + r) * a.N + n] = dx[kb][r];
    }
  }
}
__device__ __forceinline__ f32x4 load_dy_fast(const MlpArgs& a, int64_t gi, int j, int q) {
  const int64_t n = gi * 16 + j;
  f32x4 g;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = a.y[(size_t)min(4 * q + r, a.out_dim - 1) * a.N + n];
    g[r] = 4 * q + r < a.out_dim ? v : 0.f;
  }
  return g;
}

// Loads whose issue point the compiler cannot move: written as source-level "prefetch into registers" the loads of
// the next group get sunk to their first use (register pressure) and their latency is paid in full each group.
// The compiler does not know these registers are pending, so every consumer must sit behind await_loads().
__device__ __forceinline__ void issue_load_b128(f32x4& dst, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void issue_load_b32(float& dst, const float* p) {
  asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void issue_load_b64(f32x2& dst, const void* p) {
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void issue_load_u16(float& dst, const void* p) {  // zero-extended 16 bits in a 32-bit register
  asm volatile("global_load_ushort %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void pin(f32x2& x) { asm volatile("" : "+v"(x)); }
// four 16-bit operands (bf16 / fp16) packed in two dwords -> fp32 (exact)
template <int HT>
__device__ __forceinline__ f32x4 unpack16(const f32x2& v) {
  const uint32_t u0 = __float_as_uint(v[0]), u1 = __float_as_uint(v[1]);
  if constexpr (HT == 2) return f32x4{widen16<2>(u0 & 0xFFFFu), widen16<2>(u0 >> 16), widen16<2>(u1 & 0xFFFFu), widen16<2>(u1 >> 16)};
  else return f32x4{__uint_as_float(u0 << 16), __uint_as_float(u0 & 0xFFFF0000u), __uint_as_float(u1 << 16),
                    __uint_as_float(u1 & 0xFFFF0000u)};
}
__device__ __forceinline__ void await_loads() {
  __builtin_amdgcn_sched_barrier(0);  // nothing (in particular no MFMA) may be scheduled across the wait
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// an empty volatile asm that "modifies" x: volatile asms keep their order, so a consumer of x cannot be scheduled
// above the await_loads() that precedes this call
__device__ __forceinline__ void pin(f32x4& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(float& x) { asm volatile("" : "+v"(x)); }
// The same issue-now loads in the scalar-base form: address = SGPR pair (wave-uniform base) + 32-bit VGPR offset + 13-bit
// immediate.  A saved-activation fragment of group gi sits at H + gi * 4096 bytes (+ block * 1024): with the group's base in
// SGPRs (two scalar instructions per group and layer) the 32 loads of a group need no per-load 64-bit vector address
// arithmetic at all (the flat form cost one v_lshl_add_u64 per load and ~150 scalar instructions per group).
template <int IMM> __device__ __forceinline__ void issue_load_b32_s(float& dst, const void* sbase, uint32_t voff) {
  asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "i"(IMM) : "memory");
}
template <int IMM> __device__ __forceinline__ void issue_load_b64_s(f32x2& dst, const void* sbase, uint32_t voff) {
  asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "i"(IMM) : "memory");
}
template <int IMM> __device__ __forceinline__ void issue_load_b128_s(f32x4& dst, const void* sbase, uint32_t voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "i"(IMM) : "memory");
}
template <int IMM> __device__ __forceinline__ void issue_load_u16_s(float& dst, const void* sbase, uint32_t voff) {
  asm volatile("global_load_ushort %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "i"(IMM) : "memory");
}
// stores in the same form (nt: streamed, as __builtin_nontemporal_store)
template <int IMM> __device__ __forceinline__ void store_b32_s(const void* sbase, uint32_t voff, float v) {
  asm volatile("global_store_dword %0, %1, %2 offset:%3" : : "v"(voff), "v"(v), "s"(sbase), "i"(IMM) : "memory");
}
template <int IMM> __device__ __forceinline__ void store_b32_s_nt(const void* sbase, uint32_t voff, uint32_t v) {
  asm volatile("global_store_dword %0, %1, %2 offset:%3 nt" : : "v"(voff), "v"(v), "s"(sbase), "i"(IMM) : "memory");
}
// (s_nop: a VMEM store of more than 64 bits reads its data registers after issue - a VALU write of those registers needs wait
//  states behind it, which the hazard recogniser only inserts for instructions it can see.  The stored value may be a temporary
//  whose registers are rewritten at once: round 5's scaled copies of the saved activations came out as the NEXT block's values.)
template <int IMM> __device__ __forceinline__ void store_b128_s_nt(const void* sbase, uint32_t voff, const f32x4& v) {
  asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 nt\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(sbase), "i"(IMM) : "memory");
}
// compile-time loop: f(std::integral_constant<int, 0>{}), ..., so that loop indices can be asm immediates
template <typename F, int... I> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// ---------------------------------------------------- forward, software-pipelined
// mlp_fwd_kernel below loads a tile's inputs at the top of its loop and uses them at once: loads and stores retire
// through one in-order counter (vmcnt), so that wait also drains every store of the previous tile, and a tile costs
// [store drain + load latency] + [compute] in sequence (measured: the density network's launch moved 0.74 GB in
// 0.176 ms = 4.2 TB/s).  Here the loads of the NEXT tile are issued (inline asm: the compiler would sink them to their
// first use) before the layer products of the current one, all stores of a tile (saved hidden fragments, outputs) are
// held back to the end of the tile, and the prefetch is awaited right before them: the wait covers loads that are one
// whole tile of MFMAs old, the stores drain under the next tile's MFMAs.
// Requires the fast input path, whole tiles (n_groups % (4 kG) == 0) and NH = 1 or 2 hidden layers.
// COMPACT (with SAVE): one bit per hidden unit and sample for every layer and nothing else (nesvor_mlp_t.compact_save; round 5 -
// rounds 3-4 also stored the values of the layers after the first): the density network's launch writes 0.08 GB instead of
// 0.74 GB (full save) / 0.35 GB (rounds 3-4) at N = 2^20 next to the 0.13 GB it reads.
// OUT1 (split mode, out_dim == 1: sigma_net, b_net): the output layer is a dot product per sample - 16 fp32 FMAs per lane and
// a sum over the four feature quads - instead of twelve MFMAs on 15/16 padding plus the 3-way split of the last hidden layer
// (4 fragments x 14 VALU), which nothing else needs.
constexpr int kFwdMinBlocks = 2;  // (round 4: with the scalar-base input addressing the split-mode instantiations need 144-156 VGPRs - three
                                  // workgroups would fit a CU; launch_kb explains why two are launched)
// SPLM: 0 fp32 MFMAs, 1 (true) the split mode, 2 the split mode's leading term alone (nesvor_mlp_t.bf16_operands == 4: scaled fp16
// operands, ONE MFMA per product - same scales, images and save formats, a third of the matrix work and half of the splitting)
// NOB (mode 4 only): a bias-free network (NULL nesvor_mlp_t.bias) - the accumulators start at zero, no bias is staged or added.
template <int KB1, int NH, int SPLM, bool SAVE, bool COMPACT = false, bool OUT1 = false, bool NOB = false>
__global__ __launch_bounds__(256, (SPLM != 0 && KB1 <= 2) ? kFwdMinBlocks : 1) void mlp_fwd_pf_kernel(const MlpArgs a) {
  constexpr bool SPL = SPLM != 0;
  static_assert(!NOB || SPLM == 2, "NOB: mode-4 instantiations only");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int k_in = a.k_a + a.k_b;
  constexpr int kBlk = 256;  // floats per image block (split mode: two fp16 planes)
  float* img1 = lds;
  float* imgh = img1 + kHB * KB1 * kBlk;
  float* imgo = imgh + (NH - 1) * kHB * kHB * kBlk;
  float* bias = imgo + 1 * kHB * kBlk;
  float* wout = bias + (NH + 1) * kWidth;  // OUT1: the single output row in fp32
  // split mode: the launch's scales (MlpScales).  unit[l] = units of layer l's accumulators, mult[l] = multiplier of the split
  // that feeds layer l (its input arrives in the previous layer's units; the network input in true units)
  float unit[NH + 1], inv_unit[NH + 1], mult[NH + 1];
#pragma unroll
  for (int l = 0; l <= NH; ++l) { unit[l] = 1.f; inv_unit[l] = 1.f; mult[l] = 1.f; }
  if constexpr (SPL) {
    const MlpScales sc = mlp_scales(a.prep, NH, a.k_a > 0, false);
#pragma unroll
    for (int l = 0; l <= NH; ++l) {
      unit[l] = uniform_f(sc.sw[l] * sc.sx[l]);
      inv_unit[l] = pow2_inv(unit[l]);
      mult[l] = l == 0 ? sc.sx[0] : uniform_f(sc.sx[l] * inv_unit[l - 1]);
    }
    if (a.wimg != nullptr) {  // prebuilt for the current weights (see wimg_plane)
      copy_image_ct<kHB * KB1 * kBlk, 256>(img1, a.wimg + wimg_offset(NH, KB1, 0));
#pragma unroll
      for (int l = 1; l < NH; ++l) copy_image_ct<kHB * kHB * kBlk, 256>(imgh + (l - 1) * kHB * kHB * kBlk, a.wimg + wimg_offset(NH, KB1, l));
      if constexpr (!OUT1) copy_image_ct<kHB * kBlk, 256>(imgo, a.wimg + wimg_offset(NH, KB1, NH));
    } else {
      build_image_ct<false, SPL, false, kHB, KB1, 256>(img1, a.W[0], kWidth, k_in, sc.sw[0]);
#pragma unroll
      for (int l = 1; l < NH; ++l) build_image_ct<false, SPL, false, kHB, kHB, 256>(imgh + (l - 1) * kHB * kHB * kBlk, a.W[l], kWidth, kWidth, sc.sw[l]);
      if constexpr (!OUT1) build_image_ct<false, SPL, false, 1, kHB, 256>(imgo, a.W[NH], a.out_dim, kWidth, sc.sw[NH]);
    }
  } else {
    build_image_ct<false, SPL, false, kHB, KB1, 256>(img1, a.W[0], kWidth, k_in);
    for (int l = 1; l < NH; ++l) build_image_ct<false, SPL, false, kHB, kHB, 256>(imgh + (l - 1) * kHB * kHB * kBlk, a.W[l], kWidth, kWidth);
    if constexpr (!OUT1) build_image_ct<false, SPL, false, 1, kHB, 256>(imgo, a.W[NH], a.out_dim, kWidth);
  }
  if constexpr (OUT1) {  // the VALU output layer consumes the last hidden layer in ITS units
    for (int e = threadIdx.x; e < kWidth; e += blockDim.x) wout[e] = a.W[NH][e] * inv_unit[NH - 1];
  }
  if constexpr (!NOB) {
    for (int e = threadIdx.x; e < (NH + 1) * kWidth; e += blockDim.x) {
      const int l = e / kWidth, o = e % kWidth;
      float us = 1.f;  // biases enter as the accumulators' initial values: in the layer's units (the OUT1 output stays fp32)
#pragma unroll
      for (int t = 0; t <= NH; ++t) us = (t == l && !(OUT1 && t == NH)) ? unit[t] : us;
      bias[e] = (l < NH || o < a.out_dim) ? a.b[l][o] * us : 0.f;
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int64_t n_tiles = (a.N >> 4) / (4 * kG);
  const int ka_blocks = a.k_a >> 4;
  // every element of an input block is one dword load; a pixel-feature block and a row block differ only in the address.
  // Scalar-base form (round 4): the lane's byte offsets inside a group - ((b_row0 + row) N + j) 4 for a row block, (16 kb +
  // 4 q + r) 4 for a pixel block - are tile-invariant and computed once (a.off32: they fit 32 bits); a tile adds two SGPR
  // bases per group.  The flat form re-derived sixteen 64-bit addresses per group and tile: ~40 scalar branches and several
  // hundred scalar / vector address instructions per tile and wave next to 168 MFMAs.
  uint32_t xoff[KB1][4];
#pragma unroll
  for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = max(min(16 * (kb - ka_blocks) + 4 * q + r, a.k_b - 1), 0);
      xoff[kb][r] = kb < ka_blocks ? (uint32_t)((16 * kb + 4 * q + r) * 4) : (uint32_t)(((int64_t)(a.b_row0 + row) * a.N + j) * 4);
    }
  uint32_t yoff[4];  // output rows 4 q + r of sample j (a.off32 covers out_dim rows)
#pragma unroll
  for (int r = 0; r < 4; ++r) yoff[r] = (uint32_t)(((int64_t)min(4 * q + r, a.out_dim - 1) * a.N + j) * 4);
  const int spg = a.S >> 4;
  auto issue_x = [&](int64_t tile, float (&xr)[kG][KB1][4]) __attribute__((always_inline)) {
    const int64_t g0 = (tile * 4 + wave) * kG;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int64_t gi = g0 + g;
      const int64_t pixel = a.spg_shift >= 0 ? (gi >> a.spg_shift) : gi / spg;
      const char* bbase = reinterpret_cast<const char*>(a.xb) + gi * 64;
      const char* abase = reinterpret_cast<const char*>(a.xa) + pixel * (int64_t)(a.k_a * 4);
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb) {
        const char* base = kb < ka_blocks ? abase : bbase;
#pragma unroll
        for (int r = 0; r < 4; ++r) issue_load_b32_s<0>(xr[g][kb][r], base, xoff[kb][r]);
      }
    }
  };
  auto settle_x = [&](float (&xr)[kG][KB1][4]) __attribute__((always_inline)) {
    await_loads();
#pragma unroll
    for (int g = 0; g < kG; ++g)
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) pin(xr[g][kb][r]);
  };
  float xr[kG][KB1][4];
#pragma unroll
  for (int g = 0; g < kG; ++g)
#pragma unroll
    for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) xr[g][kb][r] = 0.f;
  float y_mx = 0.f;
  if ((int64_t)blockIdx.x < n_tiles) { issue_x(blockIdx.x, xr); settle_x(xr); }
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t g0 = (tile * 4 + wave) * kG;
    f32x4 x[kG][KB1];
#pragma unroll
    for (int g = 0; g < kG; ++g)
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          // (a select, not an alias: x must be a COPY of the prefetch set.  The next tile's loads are requested into xr right
          //  below, while x is still in use; with x = xr the compiler gives the new xr other registers and moves them back
          //  for the loop - a register move that can read a register whose load has not landed.  Tried in round 4: whole
          //  16-sample groups of wrong outputs, at random, tools/diag_mlp.py.)
          x[g][kb][r] = (kb < ka_blocks || 16 * (kb - ka_blocks) + 4 * q + r < a.k_b) ? xr[g][kb][r] : 0.f;
    // the last tile of a workgroup re-requests a valid tile (no control flow between an issue and its settle)
    issue_x(min(tile + (int64_t)gridDim.x, n_tiles - 1), xr);
    f32x4 h[NH][kG][kHB];
    uint32_t hmask[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) hmask[g] = 0u;
#pragma unroll
    for (int l = 0; l < NH; ++l) {
#pragma unroll
      for (int ob = 0; ob < kHB; ++ob) {
        const f32x4 bq = NOB ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(bias + l * kWidth + 16 * ob + 4 * q);
#pragma unroll
        for (int g = 0; g < kG; ++g) h[l][g][ob] = bq;
      }
      if (l == 0) apply_layer<KB1, kHB, false, SPLM>(img1, x, h[0], lane, mult[0]);
      else apply_layer<kHB, kHB, false, SPLM>(imgh + (l - 1) * kHB * kHB * kBlk, h[l - 1], h[l], lane, mult[l]);
      if constexpr (SAVE && COMPACT) {
        // The gate bits of a layer from the SIGN bits of the pre-activations: v_alignbit_b32 sg, sg, x, 31 = (sg << 1) | (x >> 31)
        // shifts one sign in per instruction (rounds 1-3: v_min_u32 + v_lshl_or_b32 on the ReLU output, two per value).
        // Inserted from the highest bit index down, complemented once per layer: bit 4 ob + r = [x >= +0], which is [h > 0]
        // for every pre-activation but an exact +0 (there the gate lets a gradient through that ReLU'(0) = 0 drops; an
        // exact zero pre-activation only occurs for zero-padded units, whose incoming gradient is zero either way).
#pragma unroll
        for (int g = 0; g < kG; ++g) {
          uint32_t sg = 0u;
#pragma unroll
          for (int ob = kHB - 1; ob >= 0; --ob)
#pragma unroll
            for (int r = 3; r >= 0; --r) sg = __builtin_amdgcn_alignbit(sg, __float_as_uint(h[l][g][ob][r]), 31);
          hmask[g] = l == 0 ? (~sg & 0xFFFFu) : ((~sg << 16) | hmask[g]);
        }
      }
#pragma unroll
      for (int g = 0; g < kG; ++g)
#pragma unroll
        for (int ob = 0; ob < kHB; ++ob)
#pragma unroll
          for (int r = 0; r < 4; ++r) h[l][g][ob][r] = relu_f(h[l][g][ob][r]);
    }
    f32x4 o[kG][1];
    if constexpr (OUT1) {
      float part[kG];
#pragma unroll
      for (int g = 0; g < kG; ++g) part[g] = 0.f;
#pragma unroll
      for (int ob = 0; ob < kHB; ++ob) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wout + 16 * ob + 4 * q);
#pragma unroll
        for (int g = 0; g < kG; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) part[g] = fmaf(w[r], h[NH - 1][g][ob][r], part[g]);
      }
#pragma unroll
      for (int g = 0; g < kG; ++g) {
        part[g] += __shfl_xor(part[g], 16, 64);
        part[g] += __shfl_xor(part[g], 32, 64);
        o[g][0] = f32x4{NOB ? part[g] : part[g] + bias[NH * kWidth], 0.f, 0.f, 0.f};  // (only lanes q == 0 store it)
      }
    } else {
      const f32x4 bq = NOB ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(bias + NH * kWidth + 4 * q);
#pragma unroll
      for (int g = 0; g < kG; ++g) o[g][0] = bq;
      apply_layer<kHB, 1, false, SPLM>(imgo, h[NH - 1], o, lane, mult[NH]);
      if constexpr (SPL) {
#pragma unroll
        for (int g = 0; g < kG; ++g) o[g][0] *= inv_unit[NH];
      }
    }
    if (a.y_absmax != nullptr) {
#pragma unroll
      for (int g = 0; g < kG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) y_mx = fmaxf(y_mx, fabsf(o[g][0][r]));  // (rows beyond out_dim: zero weights and bias)
    }
    settle_x(xr);
    if constexpr (SAVE && !COMPACT) {  // (COMPACT: the gate bits below are all the backward needs - it recomputes the activations)
#pragma unroll
      for (int l = 0; l < NH; ++l)
#pragma unroll
        for (int g = 0; g < kG; ++g) {
          const char* hbase = reinterpret_cast<const char*>(a.H[l]) + (g0 + g) * (int64_t)(kHB * 64 * 16);
          // (split mode: the layer's values leave in true units - an exact multiplication by a power of two)
          static_for<kHB>([&](auto ob) {
            f32x4 hv = h[l][g][decltype(ob)::value];
            if constexpr (SPL) hv *= inv_unit[l];
            store_b128_s_nt<decltype(ob)::value * 64 * 16>(hbase, (uint32_t)lane * 16u, hv);
          });
        }
    }
    if constexpr (SAVE && COMPACT) {
#pragma unroll
      for (int g = 0; g < kG; ++g)
        store_b32_s_nt<0>(reinterpret_cast<const char*>(a.Hm) + (g0 + g) * 256, (uint32_t)lane * 4u, hmask[g]);
    }
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const char* ybase = reinterpret_cast<const char*>(a.y) + (g0 + g) * 64;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * q + r < a.out_dim) store_b32_s<0>(ybase, yoff[r], o[g][0][r]);
    }
  }
  if (a.y_absmax != nullptr) publish_absmax_wg(a.y_absmax, y_mx);
}

// ------------------------------------------------------------------- forward
// (the general kernel: any N, any input composition, up to three hidden layers; fp32 MFMAs or bf16-rounded operands - the
//  split mode lives in the pipelined kernel above, and shapes it does not take are evaluated here on the fp32 pipe, which is
//  always a valid evaluation of the split mode)
template <int KB1, int BF16 = 0>
__global__ __launch_bounds__(256) void mlp_fwd_kernel(const MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n_hidden = a.n_linear - 1;
  const int k_in = a.k_a + a.k_b;
  // LDS carve: [img1 | img hidden 2..n_hidden | img out | biases]   (an image block = 256 floats)
  constexpr int kBlk = 256;
  float* img1 = lds;
  float* imgh = img1 + kHB * KB1 * kBlk;
  float* imgo = imgh + (n_hidden - 1) * kHB * kHB * kBlk;
  float* bias = imgo + 1 * kHB * kBlk;
  build_image<BF16>(img1, a.W[0], kWidth, k_in, kHB, KB1);
  for (int l = 1; l < n_hidden; ++l) build_image<BF16>(imgh + (l - 1) * kHB * kHB * kBlk, a.W[l], kWidth, kWidth, kHB, kHB);
  build_image<BF16>(imgo, a.W[n_hidden], a.out_dim, kWidth, 1, kHB);
  for (int e = threadIdx.x; e < a.n_linear * kWidth; e += blockDim.x) {
    const int l = e / kWidth, o = e % kWidth;
    bias[e] = (l < n_hidden || o < a.out_dim) ? a.b[l][o] : 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int64_t n_groups = (a.N + 15) / 16;
  const int64_t n_tiles = (n_groups + 4 * kG - 1) / (4 * kG);
  float y_mx = 0.f;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t g0 = (tile * 4 + wave) * kG;
    f32x4 x[kG][KB1];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      if (a.fast) {
        load_x_fast<KB1>(a, min(g0 + g, n_groups - 1), j, q, x[g]);
      } else {
        const int64_t n = min((g0 + g) * 16 + j, a.N - 1);
#pragma unroll
        for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) x[g][kb][r] = fetch_input(a, 16 * kb + 4 * q + r, n);
      }
    }
    f32x4 h[kG][kHB];
#pragma unroll
    for (int ob = 0; ob < kHB; ++ob) {
      const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + 16 * ob + 4 * q);
#pragma unroll
      for (int g = 0; g < kG; ++g) h[g][ob] = bq;
    }
    apply_layer<KB1, kHB, BF16>(img1, x, h, lane);
    for (int l = 0;; ++l) {
      // ReLU + save fragments of hidden layer l
#pragma unroll
      for (int g = 0; g < kG; ++g)
#pragma unroll
        for (int ob = 0; ob < kHB; ++ob) {
#pragma unroll
          for (int r = 0; r < 4; ++r) h[g][ob][r] = relu_f(h[g][ob][r]);
          if (a.H[l] != nullptr && g0 + g < n_groups) {
            const size_t e = (((size_t)(g0 + g) * kHB + ob) * 64 + lane) * 4;
            // written once, read by the backward many kernels later: streaming stores (no L2 allocation)
            if constexpr (BF16) __builtin_nontemporal_store(pack16<BF16>(h[g][ob]), reinterpret_cast<s16x4*>(reinterpret_cast<__bf16*>(a.H[l]) + e));
            else __builtin_nontemporal_store(h[g][ob], reinterpret_cast<f32x4*>(a.H[l] + e));
          }
        }
      if (l + 1 >= n_hidden) break;
      f32x4 h2[kG][kHB];
#pragma unroll
      for (int ob = 0; ob < kHB; ++ob) {
        const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + (l + 1) * kWidth + 16 * ob + 4 * q);
#pragma unroll
        for (int g = 0; g < kG; ++g) h2[g][ob] = bq;
      }
      apply_layer<kHB, kHB, BF16>(imgh + l * kHB * kHB * kBlk, h, h2, lane);
#pragma unroll
      for (int g = 0; g < kG; ++g)
#pragma unroll
        for (int ob = 0; ob < kHB; ++ob) h[g][ob] = h2[g][ob];
    }
    f32x4 o[kG][1];
    {
      const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + n_hidden * kWidth + 4 * q);
#pragma unroll
      for (int g = 0; g < kG; ++g) o[g][0] = bq;
    }
    apply_layer<kHB, 1, BF16>(imgo, h, o, lane);
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int64_t n = (g0 + g) * 16 + j;
      if (n < a.N) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * q + r < a.out_dim) { a.y[(size_t)(4 * q + r) * a.N + n] = o[g][0][r]; y_mx = fmaxf(y_mx, fabsf(o[g][0][r])); }
      }
    }
  }
  if (a.y_absmax != nullptr) publish_absmax_wg(a.y_absmax, y_mx);
}

// (backward as a dX launch + a dW launch, for the shapes the wave-specialised kernel below does not take: since round 6 the wide
//  kernels of csrc/mlp_wide.hip at width 64 - same fragment layouts, one implementation instead of two; nesvor_mlp_backward_bounded.
//  The 16-bit operand modes have a pair of their own, right below.)

// ------------------------------------------------- backward, 16-bit operands: dX launch + dW launch
// The shapes of modes 1 / 3 (HT = 1 bf16, HT = 2 fp16) that the wave-specialised kernel below does not take: three hidden layers,
// three or four input blocks at two hidden layers, ragged N, S or k_a.  Any shape the 16-bit forward takes (width 64, 1-3 hidden
// layers, k_a + k_b <= 64, out_dim <= 16).  The pair reads what that forward saved - 16-bit fragments ([group][block][lane][4],
// 8 bytes per lane) - and rounds exactly the operands the 16-bit instantiations of mlp_bwd_ws_kernel round, with the same
// round-to-nearest-even conversions (pack16 / store16):
//   dX launch : dY -> 16 bit, times W_out^T (16-bit image);  per hidden layer l, from the top: gate with the saved h_l > 0 (fp32
//               compare of the widened 16-bit value), store the gated pre-activation gradient dpre_l in fp32, round it to 16 bit,
//               times W_l^T (16-bit image); the layer-0 product is dX (fp32).
//   dW launch : dW_out = sum_n rn16(dY) h_{NH-1}^T,  dW_l = sum_n rn16(dpre_l) h_{l-1}^T,  dW_0 = sum_n rn16(dpre_0) rn16(x)^T
//               (saved h are 16-bit already: exact);  db_out = sum_n dY,  db_l = sum_n dpre_l - fp32, unrounded, as the fused
//               kernel's chain-wave sums.
// fp32 accumulation everywhere; master weights and biases are never rounded.  In fp16 an operand beyond 65504 becomes inf and
// reaches the gradients unclamped (what the loss scaler looks for).  dpre scratch: n_pad * 64 fp32 per hidden layer (the fused
// kernel's dpre never leaves registers; here it is the hand-over between the two launches, kept in fp32 for the bias sums).
// Outputs as the wide pair: dxa per sample (N, k_a) (no group sums), dxb (k_b, N), dW_partial (n_partial, total_params) in
// nn.Linear order W0, b0, W1, b1, ... (bias columns always present, as fill_args counts them).  No atomics but the max of
// dx_absmax (order-free): two calls give the same bits.
// dX: all transposed images stay in LDS for the whole launch (16-bit: 26 KB at three hidden layers); the first layer's image is
// kept four blocks tall (zero rows beyond k_in) so that every product has compile-time shapes - at most 12 MFMAs of padding per
// group, on a path that is not the headline's.
constexpr int kBlk16 = 128;  // floats per 16-bit image block (256 elements)
size_t dx16_lds_bytes(int n_hidden) { return sizeof(float) * (size_t)kBlk16 * (kHB + (n_hidden - 1) * kHB * kHB + kHB * kHB); }

template <int HT>
__global__ __launch_bounds__(256) void mlp_bwd_dx16_kernel(const MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n_hidden = a.n_linear - 1, k_in = a.k_a + a.k_b, KB1 = (k_in + 15) >> 4;
  float* imgo = lds;                                      // W_out^T: ib = kHB, kb = 1
  float* imgh = imgo + kHB * kBlk16;                      // W_l^T, l = 1 .. n_hidden - 1: kHB x kHB
  float* img1 = imgh + (n_hidden - 1) * kHB * kHB * kBlk16;  // W_0^T: kHB x kHB (rows beyond k_in zero)
  build_image_T<HT>(imgo, a.W[n_hidden], a.out_dim, kWidth, kHB, 1);
  for (int l = 1; l < n_hidden; ++l) build_image_T<HT>(imgh + (l - 1) * kHB * kHB * kBlk16, a.W[l], kWidth, kWidth, kHB, kHB);
  build_image_T<HT>(img1, a.W[0], kWidth, k_in, kHB, kHB);
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int64_t n_groups = (a.N + 15) / 16;
  const int64_t n_tiles = (n_groups + 4 * kG - 1) / (4 * kG);
  const bool want_dx = a.dxa != nullptr || a.dxb != nullptr;
  float dx_mx = 0.f;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t g0 = (tile * 4 + wave) * kG;
    f32x4 go[kG][1], d[kG][kHB];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int64_t n = (g0 + g) * 16 + j;
#pragma unroll
      for (int r = 0; r < 4; ++r) go[g][0][r] = (n < a.N && 4 * q + r < a.out_dim) ? a.y[(size_t)(4 * q + r) * a.N + n] : 0.f;
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib) d[g][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    apply_layer<1, kHB, HT>(imgo, go, d, lane);
    for (int l = n_hidden - 1; l >= 0; --l) {
      // d: gradient w.r.t. the output of hidden layer l -> gated by the saved activation -> dpre_l
      const s16x4* H = reinterpret_cast<const s16x4*>(a.H[l]);
      f32x4* P = reinterpret_cast<f32x4*>(a.dpre[l]);
#pragma unroll
      for (int g = 0; g < kG; ++g) {
        const bool ok = g0 + g < n_groups;
#pragma unroll
        for (int ib = 0; ib < kHB; ++ib) {
          const size_t off = ((size_t)(g0 + g) * kHB + ib) * 64 + lane;
          f32x4 hv = f32x4{0.f, 0.f, 0.f, 0.f};
          if (ok) hv = unpack16<HT>(__builtin_bit_cast(f32x2, H[off]));
#pragma unroll
          for (int r = 0; r < 4; ++r) d[g][ib][r] = hv[r] > 0.f ? d[g][ib][r] : 0.f;
          if (ok) P[off] = d[g][ib];
        }
      }
      if (l > 0) {
        f32x4 d2[kG][kHB];
#pragma unroll
        for (int g = 0; g < kG; ++g)
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) d2[g][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        apply_layer<kHB, kHB, HT>(imgh + (l - 1) * kHB * kHB * kBlk16, d, d2, lane);
#pragma unroll
        for (int g = 0; g < kG; ++g)
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) d[g][ib] = d2[g][ib];
      } else if (want_dx) {
        f32x4 dx[kG][kHB];
#pragma unroll
        for (int g = 0; g < kG; ++g)
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) dx[g][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        apply_layer<kHB, kHB, HT>(img1, d, dx, lane);
#pragma unroll
        for (int g = 0; g < kG; ++g) {
          const int64_t n = (g0 + g) * 16 + j;
          if (n >= a.N) continue;
#pragma unroll
          for (int kb = 0; kb < kHB; ++kb) {
            if (kb >= KB1) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int kk = 16 * kb + 4 * q + r;
              if (kk < a.k_a) {
                if (a.dxa != nullptr) a.dxa[(size_t)n * a.k_a + kk] = dx[g][kb][r];
              } else if (kk - a.k_a < a.k_b && a.dxb != nullptr) {
                a.dxb[(size_t)(kk - a.k_a) * a.N + n] = dx[g][kb][r];
                dx_mx = fmaxf(dx_mx, fabsf(dx[g][kb][r]));
              }
            }
          }
        }
      }
    }
  }
  if (a.dx_absmax != nullptr && a.dxb != nullptr) publish_absmax(a, dx_mx);
}

// dW / db: one workgroup (4 waves) per partial row, layer after layer over its share of the sample groups (group gi = 16 samples
// = the k of one 16x16x16 MFMA):  dW_l[out][in] += A . B,  A lane (out feature i, sample quad q) = rn16(dpre_l or dY) of samples
// 4q .. 4q+3, B lane (in feature i, q) = the layer's 16-bit input of the same samples; D lane (in i, q) = dW rows 4q .. 4q+3.
__device__ __forceinline__ float frag_f32(const float* __restrict__ F, int64_t gi, int f, int s) {  // (feature f, sample s) of group gi
  return F[(((size_t)gi * kHB + (f >> 4)) * 64 + ((f & 15) >> 2) * 16 + s) * 4 + (f & 3)];
}
__device__ __forceinline__ unsigned short frag_u16(const unsigned short* __restrict__ F, int64_t gi, int f, int s) {
  return F[(((size_t)gi * kHB + (f >> 4)) * 64 + ((f & 15) >> 2) * 16 + s) * 4 + (f & 3)];
}
template <int HT>
__global__ __launch_bounds__(256) void mlp_bwd_dw16_kernel(const MlpArgs a) {
  __shared__ float red[4][kHB * 256];  // the four waves' accumulators of one output block (and, after them, their bias sums)
  const int n_hidden = a.n_linear - 1, k_in = a.k_a + a.k_b, KB1 = (k_in + 15) >> 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int64_t n_groups = (a.N + 15) / 16;
  float* out = a.dW_partial + (size_t)blockIdx.x * a.total_params;
  int poff = 0;
  for (int l = 0; l < a.n_linear; ++l) {
    const bool last = l == n_hidden;
    const int in_dim = l == 0 ? k_in : kWidth, out_dim = last ? a.out_dim : kWidth;
    const int IB = l == 0 ? KB1 : kHB, OB = last ? 1 : kHB;
    const unsigned short* Hin = l > 0 ? reinterpret_cast<const unsigned short*>(a.H[l - 1]) : nullptr;
    f32x4 acc[kHB][kHB];
    float db[kHB];
#pragma unroll
    for (int ob = 0; ob < kHB; ++ob) {
      db[ob] = 0.f;
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib) acc[ob][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t gi = (int64_t)blockIdx.x * 4 + wave; gi < n_groups; gi += (int64_t)gridDim.x * 4) {
      s16x4 pa[kHB], pb[kHB];
#pragma unroll
      for (int ob = 0; ob < kHB; ++ob) {
        f32x4 av = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ob < OB) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int64_t n = gi * 16 + 4 * q + t;
            if (last) av[t] = (n < a.N && i < a.out_dim) ? a.y[(size_t)i * a.N + n] : 0.f;
            else av[t] = n < a.N ? frag_f32(a.dpre[l], gi, 16 * ob + i, 4 * q + t) : 0.f;
          }
          db[ob] += (av[0] + av[1]) + (av[2] + av[3]);
        }
        pa[ob] = pack16<HT>(av);
      }
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib) {
        if (ib < IB) {
          if (l == 0) {
            f32x4 xv;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int64_t n = min(gi * 16 + 4 * q + t, a.N - 1);  // (a clamped sample beyond N meets a zero A operand)
              xv[t] = fetch_input(a, 16 * ib + i, n);
            }
            pb[ib] = pack16<HT>(xv);
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) pb[ib][t] = (short)frag_u16(Hin, gi, 16 * ib + i, 4 * q + t);
          }
        } else {
          pb[ib] = s16x4{0, 0, 0, 0};
        }
      }
#pragma unroll
      for (int ob = 0; ob < kHB; ++ob)
#pragma unroll
        for (int ib = 0; ib < kHB; ++ib)
          if (ob < OB && ib < IB) acc[ob][ib] = mfma16h<HT>(pa[ob], pb[ib], acc[ob][ib]);
    }
    // the four waves' partial sums through LDS, one output block at a time -> W (out, in)
#pragma unroll
    for (int ob = 0; ob < kHB; ++ob) {
      if (ob >= OB) break;  // (uniform)
      __syncthreads();
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib) *reinterpret_cast<f32x4*>(&red[wave][(ib * 64 + lane) * 4]) = acc[ob][ib];
      __syncthreads();
      for (int e = threadIdx.x; e < IB * 256; e += 256) {
        const float s = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        const int r = e & 3, ln = (e >> 2) & 63, ib = e >> 8;
        const int o = 16 * ob + 4 * (ln >> 4) + r, in = 16 * ib + (ln & 15);
        if (o < out_dim && in < in_dim) out[poff + o * in_dim + in] = s;
      }
    }
    // bias gradients: over the sample quads (lanes i, i + 16, i + 32, i + 48) and the waves
    __syncthreads();
#pragma unroll
    for (int ob = 0; ob < kHB; ++ob) red[wave][ob * 64 + lane] = db[ob];
    __syncthreads();
    for (int e = threadIdx.x; e < OB * 16; e += 256) {
      const int ob = e >> 4, ii = e & 15;
      float s = 0.f;
      for (int w = 0; w < 4; ++w)
        for (int qq = 0; qq < 4; ++qq) s += red[w][ob * 64 + qq * 16 + ii];
      if (e < out_dim) out[poff + out_dim * in_dim + e] = s;
    }
    poff += out_dim * in_dim + out_dim;
  }
}

// ------------------------------------------------- backward, fused dX + dW + db
// Staging tiles of the wave-specialised backward (fp32 / bf16-operand modes): 16 x 16 fp32, padded rows.
constexpr int kTileStride = 20;                    // floats per sample row of a staging tile (16 + pad, 16-B aligned)
constexpr int kTileFloats = 16 * kTileStride;      // one 16 x 16 tile

__device__ __forceinline__ void stage_tile(float* tile, const f32x4& frag, int j, int q) {
  *reinterpret_cast<f32x4*>(tile + j * kTileStride + 4 * q) = frag;  // lane (j,q): features 4q..4q+3 of sample j
}
__device__ __forceinline__ void read_operand(const float* tile, int i, int q, float (&v)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = tile[(4 * q + t) * kTileStride + i];  // feature i of samples 4q..4q+3
}

// Plane tiles (split mode of the wave-specialised backward): the chain wave hands a 16 x 16 dpre tile to its dW wave already
// split - two fp16 planes of 512 bytes - so that the dW wave's A operand (feature i, samples 4q..4q+3) is one 8-byte read
// per plane and needs no splitting of its own.  The chain wave stores each plane of its fragment as it holds it - one
// ds_write_b64 per plane, the lane's four halves (features 4q..4q+3 of sample j) at 8-byte chunk j + kPlaneQ q - and the dW
// wave reads it with gfx950's transposing LDS read: ds_read_b64_tr_b16 hands lane i of a 16-lane group the element (i & 3) of
// the chunks whose addresses the group's lanes 4t + (i >> 2), t = 0..3, supply.  Lane (feature i, sample quad q') therefore
// supplies the address of chunk (sample 4q' + (i >> 2), feature quad i & 3) and receives feature i of samples 4q'..4q'+3:
// the A operand, already split (tools/tr16_probe.hip prints the instruction's lane map).  With kPlaneQ = 16 the feature quads
// q and q + 2 of one read fall on the same banks (64 dwords); the chunk index of a sample is therefore XOR-ed with 4 for
// q >= 2 (a permutation inside each quad's 16 chunks: the store stays one dense 512-byte row per plane).
// (Rounds 1-3 staged fp32 tiles that both waves split; round 4 introduced the planes - then three bf16 planes per tile;
//  DESIGN_LOG.md keeps the measurements of the variants.)
constexpr int kPlaneQ = 16;
constexpr int kPlaneBytes = 512;
constexpr int kPlaneTileFloats = 2 * kPlaneBytes / 4;  // two planes of 256 fp16
constexpr int kTile0Stride = 16;                   // the dY tile stays fp32 (no padding)
constexpr int kTile0Floats = 16 * kTile0Stride;
__device__ __forceinline__ void stage_tile0(float* tile, const f32x4& frag, int j, int q) {
  *reinterpret_cast<f32x4*>(tile + j * kTile0Stride + 4 * q) = frag;
}
__device__ __forceinline__ void read_operand0(const float* tile, int i, int q, float (&v)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = tile[(4 * q + t) * kTile0Stride + i];
}
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
template <bool HI1 = false>
__device__ __forceinline__ void stage_planes(float* tile, const Split2& s, int j, int q) {
  char* p = reinterpret_cast<char*>(tile) + 8 * ((j ^ ((q >> 1) << 2)) + kPlaneQ * q);
  *reinterpret_cast<s16x4*>(p) = s.hi;
  if constexpr (!HI1) *reinterpret_cast<s16x4*>(p + kPlaneBytes) = s.lo;
}
// HI1: the high plane of a tile alone, as the A (feature i, samples 4q..4q+3) or B operand of a 16x16x16 product
__device__ __forceinline__ s16x4 read_plane_hi(const float* tile, int i, int q) {
  const int js = 4 * q + (i >> 2);
  const char* p = reinterpret_cast<const char*>(tile) + 8 * ((js ^ ((i & 2) << 1)) + kPlaneQ * (i & 3));
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
}
// The two A tuples of a dW block product - (lo | hi) and (hi | lo): each plane is needed in both halves of a register
// quadruple.  Every tuple is READ into place (four transposing reads per tile instead of two reads and four register
// moves: the LDS pipe has room, the VALU does not).  `dup` is an opaque zero (a VGPR written by an empty asm): added to the
// address it keeps the compiler from merging the repeated reads back into one read plus moves.
struct PlanesA { f16x8 lh, hl; };
__device__ __forceinline__ void read_planes2(const float* tile, int i, int q, uint32_t dup, PlanesA& a) {
  const int js = 4 * q + (i >> 2);  // the sample whose chunk this lane addresses; its feature quad is i & 3
  const char* p = reinterpret_cast<const char*>(tile) + 8 * ((js ^ ((i & 2) << 1)) + kPlaneQ * (i & 3));
  const char* p1 = p + dup;
  const s16x4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + kPlaneBytes));
  const s16x4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1));
  const s16x4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1 + kPlaneBytes));
  a.lh = join8h(l0, h0); a.hl = join8h(h1, l1);
}


// -DNESVOR_MLP_TIMELINE=1 (tools/mlp_timeline.py): lane 0 of every wave of the first 64 workgroups of the wave-specialised backward
// records s_memtime (100 MHz) at the start / end of its group loop and the ticks it spent inside pair_sync() and behind the
// prefetch waits; nesvor_debug_mlp_timeline() copies them out.  Who waits for whom in a wave pair, without a profiler in the way.
#ifndef NESVOR_MLP_TIMELINE
#define NESVOR_MLP_TIMELINE 0
#endif
#if NESVOR_MLP_TIMELINE
__device__ unsigned long long g_mlp_timeline[64][8][4];
#define MLP_TL(x) x
#else
#define MLP_TL(x)
#endif

// ------------------------------------------------- backward, wave-specialised (dX chain | dW)
// The fused kernel above runs ONE wave per SIMD (its dW accumulators fill the register file), so every LDS
// round trip, every layer-boundary dependency and every bit of index arithmetic is paid with an idle matrix
// pipe (measured: ~15 k cycles per 16-sample group for 7.2 k cycles of MFMA).  Here a workgroup is 8 waves:
//   waves 0-3 ("chain"): dY -> dpre of every layer -> dX, exactly the dX chain above; every dY / dpre fragment
//                        is also written as a transposed tile into LDS (double-buffered per wave pair);
//   waves 4-7 ("dW")   : own the dW / db accumulators; one group behind, they read the tiles as A operands,
//                        fetch the layer inputs (saved activations, network input) straight from global memory
//                        in B-operand layout, and run the dW MFMAs.
// Wave w and wave w+4 sit on the same SIMD, each issues half of the MFMAs, and whatever one of them waits for
// is covered by the other.  One workgroup barrier per group; both roles stay under 256 registers.
// Requires the fast input path (a.fast).
// NOB: a bias-free layer - no bias sums are staged or written (the partial row has no b columns)
template <int OB, int IB, bool NOB = false>
__device__ void flush_dw_ws(float* red /* 4 x OB x IB x 256 + 4 x kWidth floats */, const f32x4 (&acc)[OB][IB], const f32x4 (&dbc)[OB],
                            float* out, int out_dim, int in_dim, int slot /* 0..3: accumulator (dW) wave, -1: none */,
                            int chain /* 0..3: chain wave (owns the bias-gradient sums), -1: none */,
                            float w_scale = 1.f, float b_scale = 1.f /* split mode: 1 / units of the accumulators / of the sums */) {
  // One staging round per LAYER (two workgroup barriers) - rounds 1-3 staged one output block at a time, 24 barriers per launch,
  // a fixed cost that weighs on small batches.  The region holds the four dW waves' accumulators of the layer side by side,
  // then the four chain waves' bias sums.
  const int lane = threadIdx.x & 63;
  constexpr int kAcc = OB * IB * 256;
  float* redb = red + 4 * kAcc;
  __syncthreads();
  if (slot >= 0) {
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) *reinterpret_cast<f32x4*>(&red[slot * kAcc + ((ob * IB + ib) * 64 + lane) * 4]) = acc[ob][ib];
  }
  // bias gradient: the chain waves summed dpre per lane (sample j, features 4q..4q+3 of block ob) over their groups;
  // sum the 16 sample lanes of a row here, the four waves below
  if (!NOB && chain >= 0) {
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      f32x4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] = row_sum_dpp(dbc[ob][r]);
      if ((lane & 15) == 0) *reinterpret_cast<f32x4*>(&redb[chain * kWidth + 16 * ob + 4 * (lane >> 4)]) = t;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kAcc; e += blockDim.x) {
    const float s = (red[e] + red[kAcc + e]) + (red[2 * kAcc + e] + red[3 * kAcc + e]);
    const int r = e & 3, ln = (e >> 2) & 63, blk = e >> 8;
    const int ib = blk % IB, ob = blk / IB;
    const int o = 16 * ob + 4 * (ln >> 4) + r, in = 16 * ib + (ln & 15);
    if (o < out_dim && in < in_dim) out[o * in_dim + in] = s * w_scale;
  }
  if constexpr (!NOB) {
    for (int e = threadIdx.x; e < OB * 16; e += blockDim.x) {
      const float s = (redb[e] + redb[kWidth + e]) + (redb[2 * kWidth + e] + redb[3 * kWidth + e]);
      if (e < out_dim) out[out_dim * in_dim + e] = s * b_scale;
    }
  }
}

// dW accumulation from a staged A tile set and B operands already in registers
template <int OB, int IB, int BF16 = 0>
__device__ __forceinline__ void accumulate_dw_regs(const float* tiles, const f32x4 (&bv)[IB], f32x4 (&acc)[OB][IB], int i, int q) {
  float av[OB][4];
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) read_operand(tiles + ob * kTileFloats, i, q, av[ob]);
  if constexpr (BF16) {
    s16x4 pb[IB];
#pragma unroll
    for (int ib = 0; ib < IB; ++ib) pb[ib] = pack16<BF16>(bv[ib]);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      const s16x4 pa = pack16<BF16>(f32x4{av[ob][0], av[ob][1], av[ob][2], av[ob][3]});
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) acc[ob][ib] = mfma16h<BF16>(pa, pb[ib], acc[ob][ib]);
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) acc[ob][ib] = mfma4(av[ob][t], bv[ib][t], acc[ob][ib]);
}
// the B tuple (hi | lo) of a plane tile: feature i of samples 4q..4q+3 from both planes
__device__ __forceinline__ f16x8 read_planes_b(const float* tile, int i, int q) {
  const int js = 4 * q + (i >> 2);
  const char* p = reinterpret_cast<const char*>(tile) + 8 * ((js ^ ((i & 2) << 1)) + kPlaneQ * (i & 3));
  const s16x4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + kPlaneBytes));
  return join8h(h, l);
}

// dW accumulation on the fp16 pipe at fp32 accuracy (split mode).  The contraction runs over the 16 samples of ONE
// group, half of what v_mfma_f32_16x16x32_f16 contracts - but the split product is a sum of 16-sample products,
// and the k index of the instruction may be numbered freely: k-slots 0..3 of a lane carry one term's operands and
// slots 4..7 another's, so one instruction evaluates TWO terms,
//     (a_lo | a_hi) . (b_hi | b_lo)  =  a_lo b_hi + a_hi b_lo
//     (a_hi | a_lo) . (b_hi | b_lo)  =  a_hi b_hi + a_lo b_lo        (the fourth term comes for free here)
// two instructions (32 matrix-pipe cycles) per 16x16x16 block product instead of four v_mfma_f32_16x16x4_f32 (128
// cycles during which the SIMD issues no VALU work at all), smallest terms first; ONE B tuple serves both.
// This variant splits its A operand here (the dY tile comes out of LDS as fp32: `av`, requested by the caller); `ma` / `mb`:
// split multipliers of the A / B operands.
template <int IB>
__device__ __forceinline__ void accumulate_dw_split(const f32x4 (&bv)[IB], f32x4 (&acc)[1][IB], const float (&av)[4], float ma, float mb) {
  f16x8 b_hl[IB];
#pragma unroll
  for (int ib = 0; ib < IB; ++ib) {
    const Split2 sb = split2(bv[ib], mb);
    b_hl[ib] = join8h(sb.hi, sb.lo);
  }
  const Split2 sa = split2(f32x4{av[0], av[1], av[2], av[3]}, ma);
  const f16x8 a_lh = join8h(sa.lo, sa.hi), a_hl = join8h(sa.hi, sa.lo);
#pragma unroll
  for (int ib = 0; ib < IB; ++ib) acc[0][ib] = mfma32_f16(a_lh, b_hl[ib], acc[0][ib]);
#pragma unroll
  for (int ib = 0; ib < IB; ++ib) acc[0][ib] = mfma32_f16(a_hl, b_hl[ib], acc[0][ib]);
}

// The same products with the A operands arriving split (plane tiles, see stage_planes): `ap` holds the requested planes of
// the first tile; the next one (of this layer, or `next_tile`) is requested before the current one is multiplied - left to
// the scheduler every read sits right in front of its use and pays the LDS latency in full (this wave has ONE partner on its
// SIMD); a scheduling barrier keeps LDS reads from sinking.
template <int OB, int IB>
__device__ __forceinline__ void accumulate_dw_tuples(const float* tiles, const f16x8 (&b_hl)[IB], f32x4 (&acc)[OB][IB], int i, int q,
                                                     PlanesA& ap, const float* next_tile, uint32_t dup);
template <int OB, int IB>
__device__ __forceinline__ void accumulate_dw_planes(const float* tiles, const f32x4 (&bv)[IB], f32x4 (&acc)[OB][IB], int i, int q,
                                                     PlanesA& ap, const float* next_tile, uint32_t dup, float mb) {
  f16x8 b_hl[IB];
#pragma unroll
  for (int c = 0; c < IB; ++c) {
    const Split2 sb = split2(bv[c], mb);
    b_hl[c] = join8h(sb.hi, sb.lo);
  }
  accumulate_dw_tuples<OB, IB>(tiles, b_hl, acc, i, q, ap, next_tile, dup);
}
// ... with the B tuples (hi | lo) given (COMPACT: read from the dW wave's own plane tiles, see mlp_bwd_ws_kernel)
template <int OB, int IB>
__device__ __forceinline__ void accumulate_dw_tuples(const float* tiles, const f16x8 (&b_hl)[IB], f32x4 (&acc)[OB][IB], int i, int q,
                                                     PlanesA& ap, const float* next_tile, uint32_t dup) {
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    PlanesA an = ap;
    const float* nt = ob + 1 < OB ? tiles + (ob + 1) * kPlaneTileFloats : next_tile;
    if (nt != nullptr) read_planes2(nt, i, q, dup, an);
    __builtin_amdgcn_sched_barrier(0x047F);  // everything but LDS instructions may cross: the read above stays above
#pragma unroll
    for (int c = 0; c < IB; ++c) acc[ob][c] = mfma32_f16(ap.lh, b_hl[c], acc[ob][c]);
#pragma unroll
    for (int c = 0; c < IB; ++c) acc[ob][c] = mfma32_f16(ap.hl, b_hl[c], acc[ob][c]);
    ap = an;
  }
}

// HI1 (mode 4): the same products from the high planes alone - one 16x16x16 MFMA per block product; `ap` holds the requested high
// plane of the first A tile, the next one is requested before the current one is multiplied (as above)
template <int OB, int IB>
__device__ __forceinline__ void accumulate_dw_hi(const float* tiles, const s16x4 (&b_hi)[IB], f32x4 (&acc)[OB][IB], int i, int q,
                                                 s16x4& ap, const float* next_tile) {
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    s16x4 an = ap;
    const float* nt = ob + 1 < OB ? tiles + (ob + 1) * kPlaneTileFloats : next_tile;
    if (nt != nullptr) an = read_plane_hi(nt, i, q);
    __builtin_amdgcn_sched_barrier(0x047F);  // everything but LDS instructions may cross: the read above stays above
#pragma unroll
    for (int c = 0; c < IB; ++c) acc[ob][c] = mfma16_f16(ap, b_hi[c], acc[ob][c]);
    ap = an;
  }
}

// SPL: the dX chain (contraction over features, 32 at a time) AND the dW products (contraction over the 16 samples of a group,
// two terms per instruction: accumulate_dw_planes) run on split-fp16 operands - see split2() and MlpScales for the units.
// COMPACT (nesvor_mlp_t.compact_save): the chain waves gate with the saved sign bits (one word per lane and group instead of
// NH x 4 fragments), the dW waves recompute the first hidden layer from the network input.
// OUT1 (split mode, out_dim == 1): the output layer's two products are rank one - d h = w_out dy and dW_out = sum_s dy_s h_s -
// and run as fp32 VALU work (16 multiplies per lane in the chain wave, 16 FMAs in the dW wave) instead of 24 + 12 MFMAs on
// 15/16 padding and the splits of their operands.
// SPLM: as in mlp_fwd_pf_kernel (2 = HI1: the leading term of the split alone; COMPACT instantiations only - every operand still goes
// through split2(), stage_planes() and the transposing reads, minus their low planes: one MFMA per block product in the chain and the
// recomputation, one 16x16x16 MFMA per block product of a weight gradient)
// NOB (HI1 only): a bias-free network (NULL nesvor_mlp_t.bias) - no bias staging for the recomputation, no bias-gradient sums in
// the chain waves, and partial rows W0 | W1 | ... | W_out (out_dim rows) without b columns: a prefix of tinycudann's flat layout
template <int KB1, int NH, int BF16 = 0, int SPLM = 0, bool COMPACT = false, bool OUT1 = false, bool NOB = false>
__global__ __launch_bounds__(512) void mlp_bwd_ws_kernel(const MlpArgs a) {
  constexpr bool SPL = SPLM != 0;
  constexpr bool HI1 = SPLM == 2;
  static_assert(!HI1 || COMPACT, "HI1: compact-save instantiations only");
  static_assert(!NOB || HI1, "NOB: mode-4 instantiations only");
  static_assert(!COMPACT || (SPL && !BF16), "compact save: split-operand mode only");
  static_assert(!OUT1 || (SPL && !BF16), "OUT1: split-operand mode only");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int k_in = a.k_a + a.k_b;
  constexpr int kT = 1 + NH * kHB;                      // tiles per group: dY, then dpre of layers NH-1 .. 0
  constexpr int kBlk = 256;                             // floats per image block (split mode: two fp16 planes)
  float* imgo = lds;                                    // W_out^T : ib = 4, kb = 1
  float* imgh = imgo + kHB * 1 * kBlk;                  // W_l^T, l = 1..NH-1
  float* img1 = imgh + (NH - 1) * kHB * kHB * kBlk;     // W_1^T : ib = KB1, kb = 4
  // COMPACT: the forward images of every hidden layer (W_1: ob = 4, kb = KB1; W_l: 4 x 4) and their biases - the dW waves
  // recompute the hidden activations - and one set of kHB plane tiles per dW wave for the recomputed B operands
  float* imgf1 = img1 + KB1 * kHB * kBlk;
  float* imgf2 = imgf1 + (COMPACT ? kHB * KB1 * kBlk : 0);
  float* bias0 = imgf2 + (COMPACT ? (NH - 1) * kHB * kHB * kBlk : 0);   // [NH][kWidth], layer l in units sw[l] sx[l]
  float* bplanes = bias0 + (COMPACT ? NH * kWidth : 0);
  float* wout = bplanes + (COMPACT ? 4 * kHB * kPlaneTileFloats : 0);  // OUT1: the single output row in fp32
  float* tiles = wout + (OUT1 ? kWidth : 0);            // [pair][buffer][kT] tiles; reused as the flush buffer
  // split mode: the launch's scales (MlpScales).  Chain: dY is split with sd[NH]; the product W_{l+1}^T d_{l+1} leaves d_l in
  // units sw[l+1] sd[l+1], the split that feeds the next product (and the planes) takes it to sd[l]; dX leaves in sw[0] sd[0].
  // dW waves: B operands h_l are split with sx[l+1] (true units from HBM; the recomputed first layer arrives in sw[0] sx[0]),
  // the network input with sx[0]; accumulators of dW_l in sd[l] sx[l].
  MlpScales sc;
#pragma unroll
  for (int l = 0; l <= kMaxLayers; ++l) { sc.sx[l] = 1.f; sc.sd[l] = 1.f; if (l < kMaxLayers) sc.sw[l] = 1.f; }
  if constexpr (SPL) sc = mlp_scales(a.prep, NH, a.k_a > 0, true);
  float m_d[NH + 1];      // chain: multiplier of the split of d_l (l = NH: dY, true units)
  float inv_d[NH + 1];    // 1 / units d_l arrives in before its split (bias-gradient sums); inv_d[NH] = 1
  float inv_w[NH + 1];    // 1 / units of the dW_l accumulators
#pragma unroll
  for (int l = NH; l >= 0; --l) {
    const float units = l == NH ? 1.f : ((OUT1 && l == NH - 1) ? 1.f : uniform_f(sc.sw[l + 1] * sc.sd[l + 1]));  // (OUT1: d_{NH-1} = w dy in fp32)
    inv_d[l] = pow2_inv(units);
    m_d[l] = uniform_f(sc.sd[l] * inv_d[l]);
    inv_w[l] = pow2_inv(uniform_f(sc.sd[l] * sc.sx[l]));
  }
  const float inv_dx = pow2_inv(uniform_f(sc.sw[0] * sc.sd[0]));
  // COMPACT: units of the recomputed hidden layers and the multipliers of their splits (into the next layer's input scale)
  float unit_h[NH], m_h[NH];
#pragma unroll
  for (int l = 0; l < NH; ++l) {
    unit_h[l] = uniform_f(sc.sw[l] * sc.sx[l]);
    m_h[l] = uniform_f(sc.sx[l + 1] * pow2_inv(unit_h[l]));
  }
  // (SPL && !BF16: a prebuilt set may stand in for the builds - wimg_plane; T images at + 2 planes of a layer's range)
  const bool prebuilt = SPL && !BF16 && a.wimg != nullptr;
  if constexpr (OUT1) {
    for (int e = threadIdx.x; e < kWidth; e += blockDim.x) wout[e] = a.W[NH][e];
  } else {
    if (prebuilt) copy_image_ct<kHB * kBlk, 512>(imgo, a.wimg + wimg_offset(NH, KB1, NH) + 2 * wimg_plane(NH, KB1, NH));
    else build_image_ct<BF16, SPL, true, kHB, 1, 512>(imgo, a.W[NH], a.out_dim, kWidth, sc.sw[NH]);
  }
#pragma unroll
  for (int l = 1; l < NH; ++l) {
    if (prebuilt) copy_image_ct<kHB * kHB * kBlk, 512>(imgh + (l - 1) * kHB * kHB * kBlk, a.wimg + wimg_offset(NH, KB1, l) + 2 * wimg_plane(NH, KB1, l));
    else build_image_ct<BF16, SPL, true, kHB, kHB, 512>(imgh + (l - 1) * kHB * kHB * kBlk, a.W[l], kWidth, kWidth, sc.sw[l]);
  }
  if (prebuilt) copy_image_ct<KB1 * kHB * kBlk, 512>(img1, a.wimg + wimg_offset(NH, KB1, 0) + 2 * wimg_plane(NH, KB1, 0));
  else build_image_ct<BF16, SPL, true, KB1, kHB, 512>(img1, a.W[0], kWidth, k_in, sc.sw[0]);
  if constexpr (COMPACT) {
    if (prebuilt) {
      copy_image_ct<kHB * KB1 * kBlk, 512>(imgf1, a.wimg + wimg_offset(NH, KB1, 0));
#pragma unroll
      for (int l = 1; l < NH; ++l) copy_image_ct<kHB * kHB * kBlk, 512>(imgf2 + (l - 1) * kHB * kHB * kBlk, a.wimg + wimg_offset(NH, KB1, l));
    } else {
      build_image_ct<false, SPL, false, kHB, KB1, 512>(imgf1, a.W[0], kWidth, k_in, sc.sw[0]);
#pragma unroll
      for (int l = 1; l < NH; ++l) build_image_ct<false, SPL, false, kHB, kHB, 512>(imgf2 + (l - 1) * kHB * kHB * kBlk, a.W[l], kWidth, kWidth, sc.sw[l]);
    }
    if constexpr (!NOB) {
      for (int e = threadIdx.x; e < NH * kWidth; e += blockDim.x) {
        float us = unit_h[0];
#pragma unroll
        for (int l = 1; l < NH; ++l) us = e >= l * kWidth ? unit_h[l] : us;
        bias0[e] = a.b[e / kWidth][e % kWidth] * us;
      }
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;               // chain: sample j, feature quad q;  dW: feature j, sample quad q
  const int role = wave >> 2, pair = wave & 3;
  // The tiles are private to a pair (chain wave w, dW wave w + 4): the per-group hand-over needs the two waves of the
  // pair to meet, not all eight.  A two-party barrier on LDS flags (each side publishes the iteration it has finished and
  // waits for the other's; LDS operations of a wave complete in order, so the flag follows the tile traffic) keeps the four
  // pairs of a workgroup out of lockstep (the workgroup barrier in its place was measured; not kept).
  __shared__ int arrive[2][4];
  if (threadIdx.x < 8) arrive[threadIdx.x >> 2][threadIdx.x & 3] = 0;
  __syncthreads();
  MLP_TL(unsigned long long tl_sync = 0ull; unsigned long long tl_wait = 0ull; unsigned long long tl_t0 = 0ull;)
  auto pair_sync = [&](int it) __attribute__((always_inline)) {
    MLP_TL(const unsigned long long ts_ = __builtin_amdgcn_s_memtime();)
    constexpr int kSpinSleep = 1;  // s_sleep argument between two looks at the other side's flag
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(&arrive[role][pair], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (__hip_atomic_load(&arrive[1 - role][pair], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < it + 1)
      __builtin_amdgcn_s_sleep(kSpinSleep);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    MLP_TL(tl_sync += __builtin_amdgcn_s_memtime() - ts_;)
  };
  // split mode: tile 0 (dY) fp32 without padding, the NH x 4 dpre tiles as fp16 planes (see stage_planes)
  constexpr bool PLANES = SPL;
  constexpr int kBufFloats = PLANES ? kTile0Floats + NH * kHB * kPlaneTileFloats : kT * kTileFloats;
  float* my_tiles = tiles + pair * 2 * kBufFloats;
  const int64_t n_groups = a.N >> 4;
  const int64_t gstride = (int64_t)gridDim.x * 4;
  const int64_t wg_first = (int64_t)blockIdx.x * 4;
  const int n_it = wg_first < n_groups ? (int)((n_groups - wg_first + gstride - 1) / gstride) : 0;  // same for all 8 waves
  const int64_t g_first = wg_first + pair;

  f32x4 acc_o[1][kHB];
  float acc1[kHB] = {0.f, 0.f, 0.f, 0.f};  // OUT1: dW_out of feature j of block ib, partial over this lane's sample quads (dW waves)
  f32x4 acc1c[kHB];                         // OUT1 + COMPACT: the same sums in the chain layout (lane (sample j, q): features 4q..4q+3 of block ib)
#pragma unroll
  for (int x = 0; x < kHB; ++x) acc1c[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 acc_h[NH > 1 ? NH - 1 : 1][kHB][kHB];
  f32x4 acc_1[kHB][KB1];
  // bias-gradient sums, kept by the chain waves in their own layout: lane (sample j, q) adds dpre[features 4q..4q+3]
  f32x4 dbc_o[1], dbc_h[NH > 1 ? NH - 1 : 1][kHB], dbc_1[kHB];
  dbc_o[0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int x = 0; x < kHB; ++x) {
    dbc_1[x] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l) dbc_h[l][x] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // Both roles prefetch the next group's global inputs into a second register set while they work on the current one and
  // swap the two sets every iteration (the loop is unrolled by two): no register-to-register copies of the prefetch.
  constexpr int kHBytes = BF16 ? 2 : 4;                 // bytes per saved activation
  if (role == 0) {
    // ------------------------------------------------------------------ chain waves
    // saved activations: fp32 fragments (16 B per lane) or, in the bf16 mode, bf16 fragments (8 B per lane)
    using RawH = typename std::conditional<(BF16 != 0), f32x2, f32x4>::type;
    uint32_t yoff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) yoff[r] = (uint32_t)(((int64_t)min(4 * q + r, a.out_dim - 1) * a.N + j) * 4);
    auto issue_group = [&](int64_t gi, float (&gy)[4], RawH (&hs)[NH][kHB], float& mk) __attribute__((always_inline)) {
      // dY rows 4q .. 4q+3 of sample j: group base in SGPRs, the lane's part (row * N + j, below 2^30 floats: off32) in one VGPR each
      const char* ybase = reinterpret_cast<const char*>(a.y) + gi * 64;
#pragma unroll
      for (int r = 0; r < 4; ++r) issue_load_b32_s<0>(gy[r], ybase, yoff[r]);
      if constexpr (COMPACT) {
        issue_load_b32_s<0>(mk, reinterpret_cast<const char*>(a.Hm) + gi * 256, (uint32_t)lane * 4u);
      } else {
        const uint32_t voff = (uint32_t)lane * (4u * kHBytes);
#pragma unroll
        for (int l = 0; l < NH; ++l) {
          const char* base = reinterpret_cast<const char*>(a.H[l]) + gi * (int64_t)(kHB * 256 * kHBytes);  // wave-uniform
          static_for<kHB>([&](auto IB) {
            constexpr int ib = decltype(IB)::value;
            if constexpr (BF16) issue_load_b64_s<ib * 256 * kHBytes>(hs[l][ib], base, voff);
            else issue_load_b128_s<ib * 256 * kHBytes>(hs[l][ib], base, voff);
          });
        }
      }
    };
    auto settle_group = [&](float (&gy)[4], RawH (&hs)[NH][kHB], float& mk) __attribute__((always_inline)) {
      await_loads();
#pragma unroll
      for (int r = 0; r < 4; ++r) pin(gy[r]);
      if constexpr (COMPACT) {
        pin(mk);
      } else {
#pragma unroll
        for (int l = 0; l < NH; ++l)
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) pin(hs[l][ib]);
      }
    };
    float dx_mx = 0.f;
    // one iteration: the group whose inputs sit in (gy_c, hs_c); the next group's inputs are requested into (gy_n, hs_n)
    auto chain_iter = [&](int it, float (&gy_c)[4], RawH (&hs_c)[NH][kHB], float& mk_c, float (&gy_n)[4], RawH (&hs_n)[NH][kHB],
                          float& mk_n) __attribute__((always_inline)) {
      const int64_t gi = g_first + (int64_t)it * gstride;
      if (it < n_it && gi < n_groups) {
        f32x4 go;
#pragma unroll
        for (int r = 0; r < 4; ++r) go[r] = 4 * q + r < a.out_dim ? gy_c[r] : 0.f;
        f32x4 hs[NH][kHB];
        const uint32_t mbits = __float_as_uint(mk_c);  // COMPACT: bit 16 l + 4 ib + r = [h_l > 0] of this lane's fragment elements
        if constexpr (!COMPACT) {
#pragma unroll
          for (int l = 0; l < NH; ++l)
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib) {
              if constexpr (BF16) hs[l][ib] = unpack16<BF16>(hs_c[l][ib]);
              else hs[l][ib] = hs_c[l][ib];
            }
        }
        // next group's inputs, one whole group of MFMAs ahead of their settle_group().  No control flow may merge
        // between an issue and its settle (a register copy at the merge would read the in-flight registers), so the
        // last iteration simply re-requests its own group
        issue_group(min(gi + gstride, n_groups - 1), gy_n, hs_n, mk_n);
        float* buf = my_tiles + (it & 1) * kBufFloats;
        if constexpr (PLANES) stage_tile0(buf, go, j, q);
        else stage_tile(buf, go, j, q);
        if constexpr (!NOB) {
          dbc_o[0] += go;
          pin(dbc_o[0]);  // (the sum stays HERE: sunk to the end of the iteration it keeps `go` alive past its in-place split)
        }
        // Split mode, round 6: a power of two PER SAMPLE on top of the launch's scale.  The launch's scale maps the largest |dY| of
        // the whole batch to 2^15; a sample whose upstream gradient lies 2^-20 below that kept 14-16 bits of its input gradient
        // and one 2^-30 below it 4-8 (measured: tests/test_gpu_ops.py::test_fused_mlp_split_dynamic_range) - and AdamW turns the
        // smallest gradients into full-size steps.  The chain is linear per sample (a column of every product, the gates included),
        // so sample j runs it on dY_j 2^k_j with k_j = 13 - exponent(sd max_r |dY[r][j]|) clamped to [0, 24]: its values sit where
        // the launch's largest do (never above: the propagated bounds stay valid), the input gradient leaves multiplied by 2^-k_j,
        // the bias-gradient sums take d 2^-k_j (one FMA instead of one add), and the planes handed to the dW wave - whose sums over
        // the samples need the LAUNCH's units - are the chain's own split scaled back by 2^-k_j in fp16 (v_pk_mul_f16: exact down
        // to the subnormals, where the absolute resolution is the one a direct split in the launch's units has).
        float inv_pj = 1.f;
        uint32_t inv_pj_h2 = 0x3C003C00u;  // (1.0, 1.0) in fp16
        if constexpr (SPL && !BF16) {
          float mxj;
          if constexpr (OUT1) {
            mxj = fabsf(__shfl(go[0], j, 64));
          } else {
            mxj = fmaxf(fmaxf(fabsf(go[0]), fabsf(go[1])), fmaxf(fabsf(go[2]), fabsf(go[3])));
            // over the four feature quads of sample j (lanes j, j + 16, j + 32, j + 48) on the VALU: gfx950's row / half swaps
            // (v_permlane16_swap, v_permlane32_swap) instead of two ds_bpermute round trips at the head of the chain
            {
              typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
              const unsigned int b0 = __float_as_uint(mxj);
              const u32x2 s16 = __builtin_amdgcn_permlane16_swap(b0, b0, false, false);
              const float m16 = fmaxf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
              const unsigned int b1 = __float_as_uint(m16);
              const u32x2 s32 = __builtin_amdgcn_permlane32_swap(b1, b1, false, false);
              mxj = fmaxf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
            }
          }
          const int e = (int)((__float_as_uint(mxj * sc.sd[NH]) >> 23) & 0xFFu) - 127;  // zero / subnormal: -127 -> the clamp
          const int k = min(max(13 - e, 0), 24);
          const float pj = __uint_as_float((uint32_t)(127 + k) << 23);
          inv_pj = __uint_as_float((uint32_t)(127 - k) << 23);
          const uint32_t h = k <= 14 ? (uint32_t)(15 - k) << 10 : 1u << (24 - k);  // 2^-k in fp16 (subnormal beyond 2^-14)
          inv_pj_h2 = h | (h << 16);
#pragma unroll
          for (int r = 0; r < 4; ++r) go[r] *= pj;
        }
        f32x4 gov[1] = {go};
        f32x4 d[kHB];
        if constexpr (!SPL) {
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) d[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (OUT1) {
          const float dyj = __shfl(go[0], j, 64);  // dY of sample j sits in the q = 0 lane
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(wout + 16 * ib + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; ++r) d[ib][r] = w[r] * dyj;
          }
        } else {
          apply_layer_g1<1, kHB, BF16, SPLM, SPL>(imgo, gov, d, lane, m_d[NH]);
        }
#pragma unroll
        for (int l = NH - 1; l >= 0; --l) {
          Split2 ds[kHB];  // (PLANES)
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if constexpr (COMPACT) {  // v_bfe_i32 (0 or all ones) + v_and_b32 (written out: the compiler's own form is and + compare + select)
                uint32_t keep;
                asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(keep) : "v"(mbits), "n"(16 * l + 4 * ib + r));
                d[ib][r] = __uint_as_float(__float_as_uint(d[ib][r]) & keep);
              } else {
                d[ib][r] = hs[l][ib][r] > 0.f ? d[ib][r] : 0.f;
              }
            }
            // (the bias-gradient sums take d BEFORE the split, in the units d arrives in: flush_dw_ws scales them back; split mode:
            //  times the sample's 2^-k_j - an FMA where the other modes add)
            if constexpr (NOB) {
            } else if constexpr (SPL && !BF16) {
              f32x4& acc_b = l > 0 ? dbc_h[l > 0 ? l - 1 : 0][ib] : dbc_1[ib];
#pragma unroll
              for (int r = 0; r < 4; ++r) acc_b[r] = __builtin_fmaf(d[ib][r], inv_pj, acc_b[r]);
              pin(acc_b);
            } else {
              if (l > 0) { dbc_h[l > 0 ? l - 1 : 0][ib] += d[ib]; pin(dbc_h[l > 0 ? l - 1 : 0][ib]); }
              else { dbc_1[ib] += d[ib]; pin(dbc_1[ib]); }
            }
            if constexpr (PLANES) {
              __builtin_amdgcn_sched_barrier(0x07FC);  // VALU instructions stay on their side: the adds above, the split below
              ds[ib] = split2m<HI1>(d[ib], m_d[l]);  // once: for the planes and for this wave's own product below
              Split2 dp = ds[ib];
              if constexpr (!BF16) {  // the dW wave's sums run in the launch's units: the sample's scale comes off (fp16, packed)
                typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
                const h16x2 ip = __builtin_bit_cast(h16x2, inv_pj_h2);
                uint2 hh = __builtin_bit_cast(uint2, ds[ib].hi), ll = __builtin_bit_cast(uint2, ds[ib].lo);
                hh.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, hh.x) * ip);
                hh.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, hh.y) * ip);
                ll.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, ll.x) * ip);
                ll.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, ll.y) * ip);
                dp.hi = __builtin_bit_cast(s16x4, hh); dp.lo = __builtin_bit_cast(s16x4, ll);
              }
              stage_planes<HI1>(buf + kTile0Floats + ((NH - 1 - l) * kHB + ib) * kPlaneTileFloats, dp, j, q);
            } else {
              stage_tile(buf + (1 + (NH - 1 - l) * kHB + ib) * kTileFloats, d[ib], j, q);
            }
          }
          if (l > 0) {
            f32x4 d2[kHB];
            if constexpr (!SPL) {
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) d2[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if constexpr (PLANES) apply_layer_g1_s<kHB, kHB, true, HI1>(imgh + (l - 1) * kHB * kHB * kBlk, ds, d2, lane);
            else apply_layer_g1<kHB, kHB, BF16, SPLM, SPL>(imgh + (l - 1) * kHB * kHB * kBlk, d, d2, lane);
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib) d[ib] = d2[ib];
          } else if (a.dxa != nullptr || a.dxb != nullptr) {
            f32x4 dx[KB1];
            if constexpr (!SPL) {
#pragma unroll
              for (int ib = 0; ib < KB1; ++ib) dx[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if constexpr (PLANES) apply_layer_g1_s<kHB, KB1, true, HI1>(img1, ds, dx, lane);
            else apply_layer_g1<kHB, KB1, BF16, SPLM, SPL>(img1, d, dx, lane);
            if constexpr (SPL) {
              const float un = inv_dx * inv_pj;  // the accumulators' units and the sample's scale: both powers of two
#pragma unroll
              for (int kb = 0; kb < KB1; ++kb) dx[kb] *= un;
            }
            if (a.dx_absmax != nullptr) track_absmax<KB1>(a, dx, dx_mx);
            // drain the prefetch BEFORE the stores below: loads and stores share vmcnt, and the wait would otherwise
            // also cover the latency of these stores
            MLP_TL(const unsigned long long tw_ = __builtin_amdgcn_s_memtime();)
            settle_group(gy_n, hs_n, mk_n);
            MLP_TL(tl_wait += __builtin_amdgcn_s_memtime() - tw_;)
            store_dx_fast<KB1>(a, gi, j, q, dx);
          } else {
            settle_group(gy_n, hs_n, mk_n);
          }
        }
      } else {
        // (an iteration without a group: nothing was requested - the wait is free, and it tells a reader of the ASSEMBLY, where this
        //  branch is merged with the one above, that no path leaves an iteration with a prefetch in flight: tools/check_inflight_loads.py)
        await_loads();
      }
      pair_sync(it);
    };
    float gy_a[4] = {0.f, 0.f, 0.f, 0.f}, gy_b[4] = {0.f, 0.f, 0.f, 0.f};
    RawH hs_a[NH][kHB], hs_b[NH][kHB];
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib) {
        if constexpr (BF16) { hs_a[l][ib] = f32x2{0.f, 0.f}; hs_b[l][ib] = f32x2{0.f, 0.f}; }
        else { hs_a[l][ib] = f32x4{0.f, 0.f, 0.f, 0.f}; hs_b[l][ib] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      }
    float mk_a = 0.f, mk_b = 0.f;
    if (g_first < n_groups) { issue_group(g_first, gy_a, hs_a, mk_a); settle_group(gy_a, hs_a, mk_a); }
    MLP_TL(tl_t0 = __builtin_amdgcn_s_memtime();)
    for (int it = 0; it <= n_it; it += 2) {
      chain_iter(it, gy_a, hs_a, mk_a, gy_b, hs_b, mk_b);
      if (it + 1 <= n_it) chain_iter(it + 1, gy_b, hs_b, mk_b, gy_a, hs_a, mk_a);
    }
    if (a.dx_absmax != nullptr) publish_absmax(a, dx_mx);
  } else {
    // ------------------------------------------------------------------ dW waves
#pragma unroll
    for (int x = 0; x < kHB; ++x) {
      acc_o[0][x] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int y = 0; y < KB1; ++y) acc_1[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l) {
#pragma unroll
        for (int y = 0; y < kHB; ++y) acc_h[l][x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if constexpr (COMPACT) {
      // ---- bits-only save (round 5): this wave recomputes EVERY hidden layer of its group from the network input, in the chain
      // layout (H^T = W X^T, exactly the forward's products on the forward images), and turns each layer's activations into
      // the B operand of its weight-gradient product through LDS: split once (for the next layer's product AND the planes),
      // store the two fp16 planes as held, read them back with the transposing read (read_planes_b).  Nothing but the input and
      // the gate bits comes from HBM: the forward writes 16 bytes per sample and network instead of 272, this kernel reads the
      // input once instead of twice and no activations at all (0.75 -> 0.35 GB for the density network's launch at N = 2^20).
      // Order: dW_0 (input planes), then h_0 -> dW_1, ..., last the output layer - so that ONE set of kHB plane tiles per wave is
      // reused layer after layer (LDS operations of a wave execute in order: a layer's planes are read before the next are stored).
      const int ka_blocks = a.k_a >> 4;
      float* my_b = bplanes + pair * kHB * kPlaneTileFloats;
      auto issue_xc = [&](int64_t gi, float (&xc)[KB1][4]) __attribute__((always_inline)) {
        const int64_t pixel = a.spg_shift >= 0 ? (gi >> a.spg_shift) : gi / (a.S >> 4);
        const char* abase = a.xa != nullptr ? reinterpret_cast<const char*>(a.xa) + pixel * (int64_t)(a.k_a * 4) : reinterpret_cast<const char*>(a.xb);
        const char* bbase = reinterpret_cast<const char*>(a.xb) + gi * 64;
        const uint32_t n4 = (uint32_t)a.N * 4u;
        const uint32_t xc_offa = (uint32_t)(4 * q * 4);
        const uint32_t xc_offb = (uint32_t)(a.b_row0 + 4 * q) * n4 + (uint32_t)(j * 4);
        const uint32_t xc_lim = (uint32_t)(a.b_row0 + a.k_b - 1) * n4 + (uint32_t)(j * 4);  // the lane's sample in the last valid row
        static_for<KB1>([&](auto KB) {
          constexpr int kb = decltype(KB)::value;
          const bool is_a = kb < ka_blocks;  // wave-uniform
          const char* base = is_a ? abase : bbase;
          static_for<4>([&](auto R) {
            constexpr int r = decltype(R)::value;
            const uint32_t ub = (uint32_t)(16 * (kb - ka_blocks) + r) * n4;  // scalar
            const uint32_t off = is_a ? xc_offa + (uint32_t)((16 * kb + r) * 4) : min(xc_offb + ub, xc_lim);
            issue_load_b32_s<0>(xc[kb][r], base, off);
          });
        });
      };
      float xcr[KB1][4];
      uint32_t dup = 0u;  // an opaque zero (read_planes2)
      asm volatile("" : "+v"(dup));
      auto settle_xc = [&]() __attribute__((always_inline)) {
        await_loads();
#pragma unroll
        for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) pin(xcr[kb][r]);
      };
      auto dw_iter = [&](int it) __attribute__((always_inline)) {
        const int64_t gi = g_first + (int64_t)(it - 1) * gstride;
        if (it > 0 && gi < n_groups) {
          const int64_t gnext = min(gi + gstride, n_groups - 1);  // (the last iteration re-requests a valid group: no control flow between an issue and its settle)
          const float* buf = my_tiles + ((it - 1) & 1) * kBufFloats;
          const float* dt0 = buf + kTile0Floats + (NH - 1) * kHB * kPlaneTileFloats;  // planes of d pre-activation 0 (staged last by the chain wave)
          f32x4 xc[KB1];
#pragma unroll
          for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              // (a select, i.e. a COPY of the prefetch set, as in the forward: the set is re-requested below while the compiler is
              //  free to schedule uses of xc behind that request)
              xc[kb][r] = (kb < ka_blocks || 16 * (kb - ka_blocks) + 4 * q + r < a.k_b) ? xcr[kb][r] : 0.f;
          issue_xc(gnext, xcr);
          PlanesA ap;
          s16x4 ap1 = s16x4{0, 0, 0, 0};  // HI1: the high plane of the next A tile
          if constexpr (HI1) ap1 = read_plane_hi(dt0, j, q);
          else read_planes2(dt0, j, q, dup, ap);
          // the input: split once - the B operand of the first layer's product here and, through the planes, of dW_0
          Split2 xs[KB1];
#pragma unroll
          for (int kb = 0; kb < KB1; ++kb) {
            xs[kb] = split2m<HI1>(xc[kb], sc.sx[0]);
            stage_planes<HI1>(my_b + kb * kPlaneTileFloats, xs[kb], j, q);
          }
          f32x4 h[kHB];
#pragma unroll
          for (int ob = 0; ob < kHB; ++ob) h[ob] = NOB ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(bias0 + 16 * ob + 4 * q);
          apply_layer_g1_s<KB1, kHB, false, HI1>(imgf1, xs, h, lane);
#pragma unroll
          for (int ob = 0; ob < kHB; ++ob)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[ob][r] = relu_f(h[ob][r]);
          if constexpr (HI1) {
            s16x4 bx[KB1];
#pragma unroll
            for (int kb = 0; kb < KB1; ++kb) bx[kb] = read_plane_hi(my_b + kb * kPlaneTileFloats, j, q);
            accumulate_dw_hi<kHB, KB1>(dt0, bx, acc_1, j, q, ap1, NH > 1 ? dt0 - kHB * kPlaneTileFloats : nullptr);
          } else {
            f16x8 bx[KB1];
#pragma unroll
            for (int kb = 0; kb < KB1; ++kb) bx[kb] = read_planes_b(my_b + kb * kPlaneTileFloats, j, q);
            accumulate_dw_tuples<kHB, KB1>(dt0, bx, acc_1, j, q, ap, NH > 1 ? dt0 - kHB * kPlaneTileFloats : nullptr, dup);
          }
          // hidden layers 1 .. NH-1: h = activations of layer l - 1 (units unit_h[l - 1]) on entry
#pragma unroll
          for (int l = 1; l < NH; ++l) {
            const float* dtl = buf + kTile0Floats + (NH - 1 - l) * kHB * kPlaneTileFloats;  // planes of d pre-activation l
            Split2 hs[kHB];
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib) {
              hs[ib] = split2m<HI1>(h[ib], m_h[l - 1]);
              stage_planes<HI1>(my_b + ib * kPlaneTileFloats, hs[ib], j, q);
            }
#pragma unroll
            for (int ob = 0; ob < kHB; ++ob) h[ob] = NOB ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(bias0 + l * kWidth + 16 * ob + 4 * q);
            apply_layer_g1_s<kHB, kHB, false, HI1>(imgf2 + (l - 1) * kHB * kHB * kBlk, hs, h, lane);
#pragma unroll
            for (int ob = 0; ob < kHB; ++ob)
#pragma unroll
              for (int r = 0; r < 4; ++r) h[ob][r] = relu_f(h[ob][r]);
            if constexpr (HI1) {
              s16x4 bh[kHB];
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) bh[ib] = read_plane_hi(my_b + ib * kPlaneTileFloats, j, q);
              accumulate_dw_hi<kHB, kHB>(dtl, bh, acc_h[l - 1], j, q, ap1, l + 1 < NH ? dtl - kHB * kPlaneTileFloats : nullptr);
            } else {
              f16x8 bh[kHB];
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) bh[ib] = read_planes_b(my_b + ib * kPlaneTileFloats, j, q);
              accumulate_dw_tuples<kHB, kHB>(dtl, bh, acc_h[l - 1], j, q, ap, l + 1 < NH ? dtl - kHB * kPlaneTileFloats : nullptr, dup);
            }
          }
          // output layer: h = activations of the last hidden layer (units unit_h[NH - 1])
          if constexpr (OUT1) {
            const float dyj = buf[j * kTile0Stride];  // dY of sample j (row 0 of the fp32 tile)
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc1c[ib][r] = fmaf(dyj, h[ib][r], acc1c[ib][r]);
          } else {
            float av[4];
            read_operand0(buf, j, q, av);
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib) {
              const Split2 hs = split2m<HI1>(h[ib], m_h[NH - 1]);
              stage_planes<HI1>(my_b + ib * kPlaneTileFloats, hs, j, q);
            }
            const Split2 sa = split2m<HI1>(f32x4{av[0], av[1], av[2], av[3]}, m_d[NH]);
            if constexpr (HI1) {
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) acc_o[0][ib] = mfma16_f16(sa.hi, read_plane_hi(my_b + ib * kPlaneTileFloats, j, q), acc_o[0][ib]);
            } else {
              f16x8 bh[kHB];
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) bh[ib] = read_planes_b(my_b + ib * kPlaneTileFloats, j, q);
              const f16x8 a_lh = join8h(sa.lo, sa.hi), a_hl = join8h(sa.hi, sa.lo);
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) acc_o[0][ib] = mfma32_f16(a_lh, bh[ib], acc_o[0][ib]);
#pragma unroll
              for (int ib = 0; ib < kHB; ++ib) acc_o[0][ib] = mfma32_f16(a_hl, bh[ib], acc_o[0][ib]);
            }
          }
          MLP_TL(const unsigned long long tw_ = __builtin_amdgcn_s_memtime();)
          settle_xc();
          MLP_TL(tl_wait += __builtin_amdgcn_s_memtime() - tw_;)
        } else {
          await_loads();  // (as in the chain wave's iteration)
        }
        pair_sync(it);
      };
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) xcr[kb][r] = 0.f;
      if (g_first < n_groups) { issue_xc(g_first, xcr); settle_xc(); }
      MLP_TL(tl_t0 = __builtin_amdgcn_s_memtime();)
      for (int it = 0; it <= n_it; ++it) dw_iter(it);
    } else {
    // B operands (layer inputs) of one group: lane (feature j, sample quad q) holds feature j of samples 4q..4q+3
    const int ka_blocks = a.k_a >> 4;
    // The saved activations are prefetched a whole group ahead into a second register set (32 registers each, swapped every
    // iteration).  The network input - the operand an iteration uses LAST, two thirds of an iteration (~3 us) after its top -
    // has one register set: it is requested at the top of the iteration that uses it, BEFORE the next group's activations, and
    // awaited with vmcnt(activation loads) - loads retire in order, the younger ones may stay in flight.  (Issue and settle of
    // a register always sit in the same straight-line region: at a control-flow merge the compiler may copy registers, and a
    // copy of a register with a load in flight reads stale data.)
    constexpr int kL0 = 0;  // (every hidden layer's values are streamed from HBM on this path)
    auto issue_h = [&](int64_t gi, float (&hraw)[NH][kHB][4]) __attribute__((always_inline)) {
      // element (sample 4q + t, feature j of block ib) of the fragment layout [block][lane = (f >> 2) * 16 + sample][f & 3]
      const uint32_t voff = (uint32_t)((((j >> 2) * 16 + 4 * q) * 4 + (j & 3)) * kHBytes);
#pragma unroll
      for (int l = kL0; l < NH; ++l) {
        const char* base = reinterpret_cast<const char*>(a.H[l]) + gi * (int64_t)(kHB * 256 * kHBytes);  // wave-uniform
        static_for<kHB>([&](auto IB) {
          static_for<4>([&](auto T) {
            constexpr int ib = decltype(IB)::value, t = decltype(T)::value;
            if constexpr (BF16) issue_load_u16_s<(ib * 256 + 4 * t) * kHBytes>(hraw[l][ib][t], base, voff);
            else issue_load_b32_s<(ib * 256 + 4 * t) * kHBytes>(hraw[l][ib][t], base, voff);
          });
        });
      }
    };
    constexpr int kHLoads = (NH - kL0) * kHB * 4;  // activation loads per group
    auto issue_x = [&](int64_t gi, f32x4 (&xraw)[KB1], float (&xsraw)[KB1]) __attribute__((always_inline)) {
      // both candidate sources of every input block are requested (no branch between issue and settle); the block
      // type picks one after the loads have landed
      const int64_t pixel = a.spg_shift >= 0 ? (gi >> a.spg_shift) : gi / (a.S >> 4);
      const char* abase = a.xa != nullptr ? reinterpret_cast<const char*>(a.xa) + pixel * (int64_t)(a.k_a * 4) : reinterpret_cast<const char*>(a.xb);
      const char* bbase = reinterpret_cast<const char*>(a.xb) + gi * 64;
      // lane parts of the addresses (32-bit byte offsets, see off32): pixel feature 16 kb + j / row (b_row0 + row), samples 4q..
      // - formed here, per group, not kept in registers across the loop (the kernel sits at the 256-register limit)
      const uint32_t n4 = (uint32_t)a.N * 4u;
      static_for<KB1>([&](auto KB) {
        constexpr int kb = decltype(KB)::value;
        const bool is_a = kb < ka_blocks;
        const int row = is_a ? 0 : min(16 * (kb - ka_blocks) + j, a.k_b - 1);
        issue_load_b32_s<0>(xsraw[kb], abase, is_a ? (uint32_t)((16 * kb + j) * 4) : 0u);
        issue_load_b128_s<0>(xraw[kb], bbase, (uint32_t)(a.b_row0 + row) * n4 + (uint32_t)(16 * q));
      });
    };
    auto settle_h = [&](float (&hraw)[NH][kHB][4], auto pending) __attribute__((always_inline)) {  // `pending`: younger loads that may stay in flight
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(pending)::value) : "memory");
#pragma unroll
      for (int l = kL0; l < NH; ++l)
#pragma unroll
        for (int ib = 0; ib < kHB; ++ib)
#pragma unroll
          for (int t = 0; t < 4; ++t) pin(hraw[l][ib][t]);
    };
    auto settle_x = [&](f32x4 (&xraw)[KB1], float (&xsraw)[KB1], auto pending) __attribute__((always_inline)) {
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(pending)::value) : "memory");
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb) { pin(xraw[kb]); pin(xsraw[kb]); }
    };
    f32x4 xraw[KB1];
    float xsraw[KB1];
    uint32_t dup = 0u;  // an opaque zero (read_planes2)
    asm volatile("" : "+v"(dup));
    // one iteration: the group (one behind the chain wave) whose saved activations sit in hraw_c; the next group's go into hraw_n
    auto dw_iter = [&](int it, float (&hraw_c)[NH][kHB][4], float (&hraw_n)[NH][kHB][4]) __attribute__((always_inline)) {
      const int64_t gi = g_first + (int64_t)(it - 1) * gstride;
      if (it > 0 && gi < n_groups) {
        f32x4 hb[NH][kHB];
#pragma unroll
        for (int l = kL0; l < NH; ++l)
#pragma unroll
          for (int ib = 0; ib < kHB; ++ib)
#pragma unroll
            for (int t = 0; t < 4; ++t)
              hb[l][ib][t] = BF16 ? widen16<(BF16 == 2 ? 2 : 1)>(__float_as_uint(hraw_c[l][ib][t])) : hraw_c[l][ib][t];
        const int64_t gnext = min(gi + gstride, n_groups - 1);  // (the last iteration re-requests a valid group: no control flow between an issue and its settle)
        issue_x(gi, xraw, xsraw);
        // the next group's activations: a whole iteration ahead
        issue_h(gnext, hraw_n);
        const float* buf = my_tiles + ((it - 1) & 1) * kBufFloats;
        auto input_operands = [&](f32x4 (&xb_)[KB1]) __attribute__((always_inline)) {
          settle_x(xraw, xsraw, std::integral_constant<int, kHLoads>{});  // requested at the top, before the kHLoads that may fly on
#pragma unroll
          for (int kb = 0; kb < KB1; ++kb) {
            if (kb < ka_blocks) {
              const float v = xsraw[kb];
              xb_[kb] = f32x4{v, v, v, v};
            } else {
              xb_[kb] = xraw[kb];  // (rows beyond k_b: a clamped row's finite values; their dW columns are never written out, flush_dw_ws)
            }
          }
        };
        if constexpr (SPL) {
          // dY tile (fp32, split here) and the first plane tile are requested together; every later A operand one tile ahead
          PlanesA ap;
          if constexpr (OUT1) {
            float dy4[4];
            read_operand0(buf, 0, q, dy4);                    // row 0 of the dY tile: samples 4q..4q+3 (a broadcast read)
            read_planes2(buf + kTile0Floats, j, q, dup, ap);
            __builtin_amdgcn_sched_barrier(0x047F);
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib)
#pragma unroll
              for (int t = 0; t < 4; ++t) acc1[ib] = fmaf(dy4[t], hb[NH - 1][ib][t], acc1[ib]);
          } else {
            float av[4];
            read_operand0(buf, j, q, av);
            read_planes2(buf + kTile0Floats, j, q, dup, ap);
            __builtin_amdgcn_sched_barrier(0x047F);
            accumulate_dw_split<kHB>(hb[NH - 1], acc_o, av, m_d[NH], sc.sx[NH]);
          }
#pragma unroll
          for (int l = NH - 1; l >= 0; --l) {
            const float* dt = buf + kTile0Floats + (NH - 1 - l) * kHB * kPlaneTileFloats;
            if (l > 0) {
              // B operand: the activations of hidden layer l - 1 - from HBM in true units, or (COMPACT, l - 1 = 0) recomputed above
              accumulate_dw_planes<kHB, kHB>(dt, hb[l - 1], acc_h[l - 1], j, q, ap, dt + kHB * kPlaneTileFloats, dup,
                                             sc.sx[l]);
            } else {
              f32x4 xb_[KB1];
              input_operands(xb_);
              accumulate_dw_planes<kHB, KB1>(dt, xb_, acc_1, j, q, ap, nullptr, dup, sc.sx[0]);
            }
          }
        } else {
          accumulate_dw_regs<1, kHB, BF16>(buf, hb[NH - 1], acc_o, j, q);
#pragma unroll
          for (int l = NH - 1; l >= 0; --l) {
            const float* dt = buf + (1 + (NH - 1 - l) * kHB) * kTileFloats;
            if (l > 0) {
              accumulate_dw_regs<kHB, kHB, BF16>(dt, hb[l - 1], acc_h[l - 1], j, q);
            } else {
              f32x4 xb_[KB1];
              input_operands(xb_);
              accumulate_dw_regs<kHB, KB1, BF16>(dt, xb_, acc_1, j, q);
            }
          }
        }
        settle_h(hraw_n, std::integral_constant<int, 0>{});
        // The consumed set is dead, but its next definition (the request two iterations on) sits under that iteration's
        // condition, so to the compiler the registers stay live around the loop - and the in-place splits of the activations
        // copied every value first (one v_mov per value).  An empty asm that "defines" the set ends the old values here.
        if constexpr (SPL && !BF16) {
#pragma unroll
          for (int l = kL0; l < NH; ++l)
#pragma unroll
            for (int ib = 0; ib < kHB; ++ib)
#pragma unroll
              for (int t = 0; t < 4; ++t) asm volatile("" : "=v"(hraw_c[l][ib][t]));
        }
      } else {
        await_loads();  // (as in the chain wave's iteration)
      }
      pair_sync(it);
    };
    float hraw_a[NH][kHB][4], hraw_b[NH][kHB][4];
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib)
#pragma unroll
        for (int t = 0; t < 4; ++t) { hraw_a[l][ib][t] = 0.f; hraw_b[l][ib][t] = 0.f; }
#pragma unroll
    for (int kb = 0; kb < KB1; ++kb) {
      xraw[kb] = f32x4{0.f, 0.f, 0.f, 0.f}; xsraw[kb] = 0.f;
    }
    // iteration it works on group it - 1: its activations must sit in the set that iteration reads (odd iterations read set b)
    if (g_first < n_groups) {
      issue_h(g_first, hraw_b);
      settle_h(hraw_b, std::integral_constant<int, 0>{});
    }
    for (int it = 0; it <= n_it; it += 2) {
      dw_iter(it, hraw_a, hraw_b);
      if (it + 1 <= n_it) dw_iter(it + 1, hraw_b, hraw_a);
    }
    }  // (!COMPACT)
  }
  if constexpr (OUT1) {
    // the rank-one sums in the accumulator layout the flush expects: row 0 of the (1 x 64) gradient sits in the q = 0 lanes
    if (role == 1) {
#pragma unroll
      for (int ib = 0; ib < kHB; ++ib) {
        float t = acc1[ib];
        if constexpr (COMPACT) {
          // chain layout (lane (sample j, q'): features 4q' + r of the block, summed over this lane's groups) -> feature j: sum the
          // 16 sample lanes of a row, then lane j takes element j & 3 of row j >> 2
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = __shfl(row_sum_dpp(acc1c[ib][r]), 16 * (j >> 2), 64);
          t = (j & 3) == 0 ? v[0] : ((j & 3) == 1 ? v[1] : ((j & 3) == 2 ? v[2] : v[3]));
        } else {
          t += __shfl_xor(t, 16, 64);
          t += __shfl_xor(t, 32, 64);
        }
        acc_o[0][ib] = f32x4{q == 0 ? t : 0.f, 0.f, 0.f, 0.f};
      }
    }
  }
#if NESVOR_MLP_TIMELINE
  if (blockIdx.x < 64u && lane == 0) {
    unsigned long long* o = g_mlp_timeline[blockIdx.x][wave];
    o[0] = tl_t0; o[1] = __builtin_amdgcn_s_memtime(); o[2] = tl_sync; o[3] = tl_wait;
  }
#endif
  // epilogue: per-workgroup partial sums in nn.Linear parameter order W0,b0,W1,b1,... (NOB: W0,W1,...; accumulators live in waves 4-7)
  const int slot = role == 1 ? pair : -1, chain = role == 0 ? pair : -1;
  float* out = a.dW_partial + (size_t)blockIdx.x * a.total_params;
  float* red = tiles;
  int poff = 0;
  flush_dw_ws<kHB, KB1, NOB>(red, acc_1, dbc_1, out + poff, kWidth, k_in, slot, chain, inv_w[0], inv_d[0]);
  poff += kWidth * k_in + (NOB ? 0 : kWidth);
#pragma unroll
  for (int l = 1; l < NH; ++l) {
    flush_dw_ws<kHB, kHB, NOB>(red, acc_h[l - 1], dbc_h[l - 1], out + poff, kWidth, kWidth, slot, chain, inv_w[l], inv_d[l]);
    poff += kWidth * kWidth + (NOB ? 0 : kWidth);
  }
  flush_dw_ws<1, kHB, NOB>(red, acc_o, dbc_o, out + poff, a.out_dim, kWidth, slot, chain,
                      OUT1 ? (COMPACT ? pow2_inv(unit_h[NH - 1]) : 1.f) : inv_w[NH], 1.f);  // (OUT1: fp32 sums of dy h; a recomputed h arrives in its layer's units)
}

// ------------------------------------------------------------ nesvor_mlp_prepare
// absolute maximum of `rows` rows of `n` floats each (row r at x + r * ld) -> slotted bound `out` (publish_absmax_f32)
__global__ __launch_bounds__(256) void absmax_rows_kernel(const float* __restrict__ x, int rows, int64_t n, int64_t ld, float* __restrict__ out) {
  float m = 0.f;
  const int64_t n4 = n >> 2;
  for (int r = 0; r < rows; ++r) {
    const float* row = x + (size_t)r * ld;
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
      const float4* r4 = reinterpret_cast<const float4*>(row);
      for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = r4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
      }
      for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(row[i]));
    } else {
      for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(row[i]));
    }
  }
  publish_absmax_wg(out, m);
}
// One workgroup per linear layer: max |W|, largest row L1 norm, largest column L1 norm, max |b| (the matrix - at most 64 x 64 -
// goes through LDS: sixteen independent coalesced loads per thread, then row sums by 64 x 4 threads and column sums by 64 x 4).
// Workgroups past the layers (at most one): max |x[0..n_x)| into slot 0 of x_slots (the slice embedding table).
constexpr int kNormJobs = 3 * kMaxLayers;
struct NormJobs {
  const float* W[kNormJobs]; const float* b[kNormJobs]; float* dst[kNormJobs];  // dst: prep + NESVOR_MLP_PREP_LAYER0 + 4 l of the layer's network
  int out[kNormJobs], in[kNormJobs];
  _Float16* img[kNormJobs];                  // null, or the layer's range [F hi | F lo | T hi | T lo] of its network's image buffer (wimg_plane)
  int oblk[kNormJobs], iblk[kNormJobs];      // output / input blocks of the layer's images
  int n_jobs;
  const float* x; int64_t n_x; float* x_slots;
};
__global__ __launch_bounds__(256) void weight_norms_kernel(const NormJobs jobs) {
  __shared__ float w[64 * 65];
  __shared__ float wsg[64 * 65];  // the signed values (the images below)
  __shared__ float red[4][4];
  __builtin_amdgcn_s_setprio(3);  // (a short launch at the head of an iteration, next to the previous one's owner pass: csrc/transform_convert.hip::step_epilogue_kernel)
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= jobs.n_jobs) {
    float m = 0.f;
    for (int64_t i = tid; i < jobs.n_x; i += 256) m = fmaxf(m, fabsf(jobs.x[i]));
    m = wave_max_f32_dpp(m);
    if ((tid & 63) == 0) red[tid >> 6][0] = m;
    __syncthreads();
    if (tid == 0) jobs.x_slots[0] = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    return;
  }
  const int l = blockIdx.x, out_dim = jobs.out[l], in_dim = jobs.in[l];
  const float* W = jobs.W[l];
  const int total = out_dim * in_dim;  // <= 4096
  float v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) { const int e = tid + 256 * u; v[u] = W[e < total ? e : 0]; }
  float wmax = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = tid + 256 * u;
    if (e < total) { const float a = fabsf(v[u]); wmax = fmaxf(wmax, a); w[(e / in_dim) * 65 + e % in_dim] = a; wsg[(e / in_dim) * 65 + e % in_dim] = v[u]; }
  }
  __syncthreads();
  // rows: thread (o = tid >> 2, part = tid & 3) sums columns part, part + 4, ...; columns likewise
  float rown = 0.f, coln = 0.f, bmax = 0.f;
  {
    const int o = tid >> 2, part = tid & 3;
    float sr = 0.f, sc = 0.f;
    if (o < out_dim) for (int k = part; k < in_dim; k += 4) sr += w[o * 65 + k];
    if (o < in_dim) for (int r = part; r < out_dim; r += 4) sc += w[r * 65 + o];
    // the four parts sit in neighbouring lanes
    sr += __shfl_xor(sr, 1, 64); sr += __shfl_xor(sr, 2, 64);
    sc += __shfl_xor(sc, 1, 64); sc += __shfl_xor(sc, 2, 64);
    rown = sr; coln = sc;
    if (tid < out_dim && jobs.b[l] != nullptr) bmax = fabsf(jobs.b[l][tid]);  // (NULL: a bias-free layer, max |b| = 0)
  }
  float r4[4] = {wmax, rown, coln, bmax};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    r4[t] = wave_max_f32_dpp(r4[t]);
    if ((tid & 63) == 0) red[tid >> 6][t] = r4[t];
  }
  __syncthreads();
  if (tid < 4) jobs.dst[l][tid] = fmaxf(fmaxf(red[0][tid], red[1][tid]), fmaxf(red[2][tid], red[3][tid]));
  // The layer's operand images of the split mode, once per iteration instead of once per workgroup of every launch
  // (nesvor_mlp_t.weight_images; build_image_ct's arithmetic, element for element: scale = pow2_scale(max |W|) - the value just
  // written to dst[0], which is what mlp_scales() derives sw[l] from)
  _Float16* img = jobs.img[l];
  if (img != nullptr) {
    const float scale = pow2_scale(fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0])));
    const int oblk = jobs.oblk[l], iblk = jobs.iblk[l];
    const int E = oblk * iblk * 256;
    for (int e = tid; e < E; e += 256) {
      const int r = e & 3, lane = (e >> 2) & 63, blk = e >> 8;
      {  // forward image: rows = output features (oblk blocks), k = input features (iblk blocks)
        const int kb = blk % iblk, ab = blk / iblk;
        const int o = 16 * ab + (lane & 15), k = 16 * kb + 4 * (lane >> 4) + r;
        const float wv = (o < out_dim && k < in_dim) ? wsg[o * 65 + k] : 0.f;
        const float ws = wv * scale;
        const _Float16 hi = (_Float16)ws;
        img[e] = hi; img[E + e] = (_Float16)(ws - (float)hi);
      }
      {  // transposed image: rows = input features (iblk blocks), k = output features (oblk blocks)
        const int kb = blk % oblk, ab = blk / oblk;
        const int k = 16 * ab + (lane & 15), o = 16 * kb + 4 * (lane >> 4) + r;
        const float wv = (o < out_dim && k < in_dim) ? wsg[o * 65 + k] : 0.f;
        const float ws = wv * scale;
        const _Float16 hi = (_Float16)ws;
        img[2 * E + e] = hi; img[3 * E + e] = (_Float16)(ws - (float)hi);
      }
    }
  }
}

size_t ws_bwd_lds_bytes(int n_hidden, int kb1, bool split = false, bool compact = false) {
  constexpr size_t blk = 256;
  size_t img = (size_t)kHB * blk + (size_t)(n_hidden - 1) * kHB * kHB * blk + (size_t)kb1 * kHB * blk;
  // compact: forward images and biases of every hidden layer + one set of kHB plane tiles per dW wave (mlp_bwd_ws_kernel)
  if (compact) img += (size_t)kb1 * kHB * blk + (size_t)(n_hidden - 1) * kHB * kHB * blk + (size_t)n_hidden * kWidth + 4 * (size_t)kHB * kPlaneTileFloats;
  const bool planes = split;  // split mode: fp32 dY tile + plane tiles (mlp_bwd_ws_kernel::PLANES)
  size_t tiles = 4 * 2 * (planes ? (size_t)kTile0Floats + (size_t)n_hidden * kHB * kPlaneTileFloats : (size_t)(1 + n_hidden * kHB) * kTileFloats);
  // the epilogue stages one layer's accumulators of the four dW waves at once (flush_dw_ws)
  const size_t widest = (size_t)kHB * (size_t)((n_hidden > 1 && kHB > kb1) ? kHB : kb1);
  const size_t flush = 4 * widest * 256 + 4 * kWidth;
  if (tiles < flush) tiles = flush;
  return sizeof(float) * (img + tiles);
}

size_t fwd_lds_bytes(int n_linear, int kb1) {
  const int n_hidden = n_linear - 1;
  constexpr size_t blk = 256;
  return sizeof(float) * ((size_t)kHB * kb1 * blk + (size_t)(n_hidden - 1) * kHB * kHB * blk + kHB * blk + (size_t)n_linear * kWidth + kWidth);
}

// persistent_tiles > 0: the kernel walks `persistent_tiles` tiles with a grid-stride loop and wants as many workgroups as the
// device holds at once - CUs x min(occupancy of THIS instantiation at this LDS size, NESVOR_FWD_WGS_PER_CU); `grid` is then
// ignored.  Since round 4 the pipelined forward needs 144-156 VGPRs in the split mode and THREE workgroups fit a CU.  Alone,
// the launch is fastest that way (density / sigma network 0.116 / 0.086 ms against 0.125 / 0.095 with two).  Inside the
// training step it is a loss on most boxes: the step runs at 1.21-1.26 kW of socket power, the engine clock floats at
// 2.30-2.39 GHz under it, and the denser forward is paid for by the kernels behind it (in-job A/B, gpurun_out/r04i: forward
// -0.002 ms, the two backward launches +0.017, step 1.135 -> 1.170 ms; on a box with more headroom 1.10 vs 1.12 the other
// way).  Two per CU is the default; -DNESVOR_FWD_WGS_PER_CU=3 / NESVOR_FWD_GRID=768 for a box that has the headroom.
#ifndef NESVOR_FWD_WGS_PER_CU
#define NESVOR_FWD_WGS_PER_CU 2
#endif
template <typename K>
int launch_kb(K k1, K k2, K k3, K k4, int kb1, dim3 grid, size_t lds, hipStream_t st, const MlpArgs& a, int threads = 256,
              int64_t persistent_tiles = 0) {
  K k = kb1 == 1 ? k1 : kb1 == 2 ? k2 : kb1 == 3 ? k3 : k4;
  const void* fn = reinterpret_cast<const void*>(k);
  static std::mutex mu;
  int dev = 0;
  if ((lds > 48 * 1024 || persistent_tiles > 0) && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (lds > 48 * 1024) {
    // raise the dynamic-LDS limit once per (device, kernel) and size (not per launch: the call is a host-side
    // attribute change and must not happen inside a stream capture); the attribute is per function AND device
    static std::map<std::pair<int, const void*>, size_t> raised;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, fn);
    auto it = raised.find(key);
    if (it == raised.end() || it->second < lds) {
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      raised[key] = lds;
    }
  }
  if (persistent_tiles > 0) {
    // workgroups the CURRENT device holds at once, per (device, kernel, LDS size): a process that drives several devices - other CU
    // counts, other partition modes - sizes every device's persistent grid for itself (advisor, round 4)
    static std::map<std::tuple<int, const void*, size_t>, int> resident;
    static const int fixed = []() { const char* e = getenv("NESVOR_FWD_GRID"); return e ? atoi(e) : 0; }();  // A/B override (run-time)
    int n_wg = fixed;
    if (n_wg <= 0) {
      std::lock_guard<std::mutex> lock(mu);
      auto it = resident.find(std::make_tuple(dev, fn, lds));
      if (it == resident.end()) {
        int cus = 256, per_cu = 2;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, threads, lds) != hipSuccess || per_cu < 1) per_cu = 2;
        if (per_cu > NESVOR_FWD_WGS_PER_CU) per_cu = NESVOR_FWD_WGS_PER_CU;
        it = resident.emplace(std::make_tuple(dev, fn, lds), cus * per_cu).first;
      }
      n_wg = it->second;
    }
    grid = dim3((unsigned)(persistent_tiles < n_wg ? persistent_tiles : n_wg));
  }
  hipLaunchKernelGGL(k, grid, dim3(threads), lds, st, a);
  return (int)hipGetLastError();
}

// A bias-free network: weights given, every bias NULL (a descriptor without weight pointers - a shape query - counts as biased).
// Mode 4 only: fill_args refuses a NULL bias next to non-NULL ones, or in any other mode (nesvor_hip.h, nesvor_mlp_t.bias).
bool bias_free(const nesvor_mlp_t* d) {
  if (d->weight[0] == nullptr || d->n_hidden < 1 || d->n_hidden + 1 > kMaxLayers) return false;
  for (int l = 0; l <= d->n_hidden; ++l)
    if (d->bias[l] != nullptr) return false;
  return true;
}

int fill_args(MlpArgs* a, const nesvor_mlp_t* d, int64_t N) {
  if (d->width != kWidth || d->n_hidden < 1 || d->n_hidden + 1 > kMaxLayers || d->out_dim < 1 || d->out_dim > 16 ||
      d->k_a < 0 || d->k_b < 0 || d->k_a + d->k_b < 1 || d->k_a + d->k_b > 64 || d->samples_per_pixel < 1)
    return (int)hipErrorInvalidValue;
  a->N = N;
  a->n_linear = d->n_hidden + 1;
  a->k_a = d->k_a; a->k_b = d->k_b; a->b_row0 = d->b_row0; a->out_dim = d->out_dim; a->S = d->samples_per_pixel;
  const bool nob = bias_free(d);
  int n_null = 0;
  for (int l = 0; l < a->n_linear; ++l) n_null += d->bias[l] == nullptr ? 1 : 0;
  if (d->weight[0] != nullptr && n_null != 0 && !(nob && d->bf16_operands == NESVOR_MLP_MODE_FP16_SCALED)) return (int)hipErrorInvalidValue;
  int total = 0;
  for (int l = 0; l < a->n_linear; ++l) {
    a->W[l] = d->weight[l]; a->b[l] = d->bias[l];
    const int in = l == 0 ? d->k_a + d->k_b : kWidth, out = l == d->n_hidden ? d->out_dim : kWidth;
    total += in * out + (nob ? 0 : out);
  }
  for (int l = a->n_linear; l < kMaxLayers; ++l) { a->W[l] = nullptr; a->b[l] = nullptr; }
  a->total_params = total;
  const int S = d->samples_per_pixel;
  a->fast = (N % 16 == 0 && S % 16 == 0 && d->k_a % 16 == 0) ? 1 : 0;
  a->dxa_group = d->dxa_group_sums ? 1 : 0;
  a->bf16 = d->bf16_operands;  // NESVOR_MLP_MODE_*
  if (a->bf16 < NESVOR_MLP_MODE_FP32 || a->bf16 > NESVOR_MLP_MODE_FP16_SCALED) return (int)hipErrorInvalidValue;
  a->hi1 = 0;
  if (a->bf16 == NESVOR_MLP_MODE_FP16_SCALED) { a->bf16 = NESVOR_MLP_MODE_SPLIT; a->hi1 = 1; }  // (the split mode's scales, images and save formats; its leading term alone where a kernel has that form - every other kernel evaluates the full split or fp32 MFMAs: more accurate, always valid)
  a->half16 = a->bf16 == NESVOR_MLP_MODE_FP16 ? 1 : 0;
  if (a->half16) a->bf16 = NESVOR_MLP_MODE_BF16;  // (every host-side decision below is that of the 16-bit operand modes; the launches pick the type)
  a->prep = d->prep;
  a->y_absmax = d->y_absmax;
  a->wimg = (a->bf16 == 2) ? static_cast<const _Float16*>(d->weight_images) : nullptr;
  {
    const int64_t rows = (int64_t)(d->b_row0 + d->k_b > d->out_dim ? d->b_row0 + d->k_b : d->out_dim);
    a->off32 = rows * N * 4 + 64 < ((int64_t)1 << 32) ? 1 : 0;
  }
  a->spg_shift = -1;
  if (a->fast) {
    const int spg = S / 16;
    if ((spg & (spg - 1)) == 0) a->spg_shift = __builtin_ctz(spg);
  }
  return 0;
}

// NESVOR_MLP_OUT1=0: networks with one output row keep the MFMA output layer (A/B)
bool out1_on() {
  static const bool on = []() { const char* e = getenv("NESVOR_MLP_OUT1"); return e == nullptr || atoi(e) != 0; }();
  return on;
}

// Which configurations can save compactly: those the pipelined forward AND the wave-specialised backward both take in the
// split-operand mode, with at most two input blocks (the recomputation's registers).
// Depends on SHAPE fields only (a.fast / a.off32 are functions of N, S, k_a, k_b, b_row0, out_dim): the fake kernel of the
// custom op (nesvor_amd/ops.py::_mlp_fake) sizes the saved buffers from a descriptor without pointers.
bool compact_ok(const MlpArgs& a, const nesvor_mlp_t* net, int64_t N) {
  static const bool use_pf = []() { const char* e = getenv("NESVOR_MLP_FWD_PF"); return e == nullptr || atoi(e) != 0; }();
  static const bool use_ws = []() { const char* e = getenv("NESVOR_MLP_BWD_WS"); return e == nullptr || atoi(e) != 0; }();
  static const bool on = []() { const char* e = getenv("NESVOR_MLP_COMPACT"); return e == nullptr || atoi(e) != 0; }();
  const int kb1 = (net->k_a + net->k_b + 15) / 16;
  return on && use_pf && use_ws && a.bf16 == 2 && a.fast && a.off32 && net->n_hidden <= 2 && kb1 <= 2 && ((N >> 4) % (4 * kG)) == 0;
}

// shapes the wave-specialised fused backward (dX + dW + db in one launch, no dpre scratch) takes
bool ws_ok(const MlpArgs& a, const nesvor_mlp_t* net) {
  static const bool use_ws = []() { const char* e = getenv("NESVOR_MLP_BWD_WS"); return e == nullptr || atoi(e) != 0; }();
  const int kb1 = (net->k_a + net->k_b + 15) / 16;
  return use_ws && a.fast && a.off32 && net->n_hidden <= 2 && (kb1 <= 2 || net->n_hidden == 1);  // (wider inputs at two hidden layers would spill)
}

}  // namespace

#if NESVOR_MLP_TIMELINE
extern "C" int nesvor_debug_mlp_timeline(unsigned long long* dst_host) {
  return (int)hipMemcpyFromSymbol(dst_host, HIP_SYMBOL(g_mlp_timeline), sizeof(unsigned long long) * 64 * 8 * 4);
}
#endif

extern "C" int nesvor_mlp_backward_fused_ok(const nesvor_mlp_t* net, int64_t N) {
  if (net == nullptr || N <= 0) return 0;
  MlpArgs a{};
  if (fill_args(&a, net, N)) return 0;
  if (bias_free(net)) return compact_ok(a, net, N) ? 1 : 0;  // (bias-free: the compact mode-4 kernel only; every other shape runs the wide pair)
  return ws_ok(a, net) ? 1 : 0;
}

extern "C" int nesvor_mlp_bias_free_ok(const nesvor_mlp_t* net, int64_t N) {
  if (net == nullptr || N <= 0 || net->weight[0] == nullptr) return 0;
  nesvor_mlp_t d = *net;
  for (int l = 0; l < kMaxLayers; ++l) d.bias[l] = nullptr;
  MlpArgs a{};
  if (fill_args(&a, &d, N) || !bias_free(&d)) return 0;
  for (int l = 0; l <= d.n_hidden; ++l)
    if (d.weight[l] == nullptr) return 0;
  // forward: the pipelined kernel or the wide kernels (any shape fill_args takes, k_b >= 1); backward: the compact kernel or the
  // wide pair - both take every such shape
  return d.k_b >= 1 ? 1 : 0;
}

extern "C" int64_t nesvor_mlp_weight_images_bytes(const nesvor_mlp_t* net) {
  if (net == nullptr || net->n_hidden < 1 || net->n_hidden + 1 > kMaxLayers || net->width != kWidth || net->k_a + net->k_b < 1 ||
      net->k_a + net->k_b > 64 || net->out_dim < 1 || net->out_dim > 16)
    return 0;
  const int kb1 = (net->k_a + net->k_b + 15) / 16;
  return (int64_t)sizeof(_Float16) * wimg_offset(net->n_hidden, kb1, net->n_hidden + 1);
}

extern "C" int nesvor_mlp_prepare_weights_images(const nesvor_mlp_t* const* nets, float* const* preps, void* const* images, int n_nets,
                                                 const float* x, int64_t n_x, float* x_slots, void* stream) {
  if (n_nets < 0 || n_nets > 3 || (n_nets > 0 && (nets == nullptr || preps == nullptr))) return (int)hipErrorInvalidValue;
  NormJobs jobs{};
  int nj = 0;
  for (int i = 0; i < n_nets; ++i) {
    const nesvor_mlp_t* net = nets[i];
    if (net == nullptr || preps[i] == nullptr || net->n_hidden < 1 || net->n_hidden + 1 > kMaxLayers || net->width != kWidth ||
        net->k_a + net->k_b > 64 || net->out_dim > 64)
      return (int)hipErrorInvalidValue;
    _Float16* img = (images != nullptr && net->out_dim <= 16) ? static_cast<_Float16*>(images[i]) : nullptr;
    const int kb1 = (net->k_a + net->k_b + 15) / 16;
    for (int l = 0; l <= net->n_hidden; ++l, ++nj) {
      jobs.W[nj] = net->weight[l]; jobs.b[nj] = net->bias[l];
      jobs.in[nj] = l == 0 ? net->k_a + net->k_b : net->width;
      jobs.out[nj] = l == net->n_hidden ? net->out_dim : net->width;
      jobs.dst[nj] = preps[i] + NESVOR_MLP_PREP_LAYER0 + 4 * l;
      jobs.img[nj] = img != nullptr ? img + wimg_offset(net->n_hidden, kb1, l) : nullptr;
      jobs.oblk[nj] = l == net->n_hidden ? 1 : kHB;
      jobs.iblk[nj] = l == 0 ? kb1 : kHB;
      if (jobs.W[nj] == nullptr) return (int)hipErrorInvalidValue;  // (a NULL bias: a bias-free layer, max |b| = 0)
    }
  }
  jobs.n_jobs = nj;
  const bool with_x = x != nullptr && x_slots != nullptr && n_x > 0;
  jobs.x = x; jobs.n_x = with_x ? n_x : 0; jobs.x_slots = x_slots;
  if (nj + (with_x ? 1 : 0) == 0) return 0;
  hipLaunchKernelGGL(weight_norms_kernel, dim3((unsigned)(nj + (with_x ? 1 : 0))), dim3(256), 0, (hipStream_t)stream, jobs);
  return (int)hipGetLastError();
}

extern "C" int nesvor_mlp_prepare_weights(const nesvor_mlp_t* const* nets, float* const* preps, int n_nets, const float* x, int64_t n_x,
                                          float* x_slots, void* stream) {
  return nesvor_mlp_prepare_weights_images(nets, preps, nullptr, n_nets, x, n_x, x_slots, stream);
}

extern "C" int nesvor_mlp_prepare(const nesvor_mlp_t* net, const float* xa, const float* xb, const float* dy, int64_t N, float* prep,
                                  int what, void* stream) {
  if (net == nullptr || prep == nullptr || N <= 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int S = net->samples_per_pixel > 0 ? net->samples_per_pixel : 1;
  auto absmax = [&](const float* x, int rows, int64_t n, int64_t ld, float* out) -> int {
    if (hipMemsetAsync(out, 0, sizeof(float) * NESVOR_ABSMAX_FLOATS, st) != hipSuccess) return (int)hipGetLastError();
    if (x == nullptr || rows <= 0 || n <= 0) return 0;
    const int64_t work = ((int64_t)rows * n + 1023) / 1024;
    hipLaunchKernelGGL(absmax_rows_kernel, dim3((unsigned)(work < 2048 ? (work < 1 ? 1 : work) : 2048)), dim3(256), 0, st, x, rows, n, ld, out);
    return (int)hipGetLastError();
  };
  if (what & NESVOR_MLP_WHAT_INPUT) {
    int e = absmax(net->k_a > 0 ? xa : nullptr, 1, (N / S) * (int64_t)net->k_a, 0, prep + NESVOR_MLP_PREP_XA);
    if (e) return e;
    e = absmax(xb != nullptr ? xb + (size_t)net->b_row0 * N : nullptr, net->k_b, N, N, prep + NESVOR_MLP_PREP_XB);
    if (e) return e;
  }
  if (what & NESVOR_MLP_WHAT_DY) {
    const int e = absmax(dy, net->out_dim, N, N, prep + NESVOR_MLP_PREP_DY);
    if (e) return e;
  }
  if (what & NESVOR_MLP_WHAT_WEIGHTS) return nesvor_mlp_prepare_weights(&net, &prep, 1, nullptr, 0, nullptr, stream);
  return (int)hipGetLastError();
}

extern "C" int nesvor_mlp_compact_save_ok(const nesvor_mlp_t* net, int64_t N) {
  if (net == nullptr || N <= 0) return 0;
  MlpArgs a{};
  if (fill_args(&a, net, N)) return 0;
  return compact_ok(a, net, N) ? 1 : 0;
}

extern "C" int nesvor_mlp_forward(const nesvor_mlp_t* net, const float* xa, const float* xb, float* y,
                                  float* const* saved_hidden, int64_t N, void* stream) {
  if (N <= 0) return 0;
  MlpArgs a{};
  int e = fill_args(&a, net, N);
  if (e) return e;
  a.xa = xa; a.xb = xb; a.y = y;
  for (int l = 0; l < kMaxLayers; ++l) a.H[l] = (saved_hidden != nullptr && l < net->n_hidden) ? saved_hidden[l] : nullptr;
  const int kb1 = (net->k_a + net->k_b + 15) / 16;
  const int64_t n_tiles = ((N + 15) / 16 + 4 * kG - 1) / (4 * kG);
  // the pipelined kernels are persistent: as many workgroups as the device holds at once (launch_kb asks the occupancy of
  // the instantiation: 3 per CU in the split mode); the plain kernel keeps two per CU
  dim3 grid((unsigned)(n_tiles < 512 ? n_tiles : 512));
  // software-pipelined kernel: fp32 data (both evaluation modes), fast inputs, whole tiles, one or two hidden layers
  static const bool use_pf = []() { const char* e = getenv("NESVOR_MLP_FWD_PF"); return e == nullptr || atoi(e) != 0; }();
  bool save_all = saved_hidden != nullptr, save_none = saved_hidden == nullptr;
  const bool compact = net->compact_save != 0 && save_all;
  if (a.bf16 == 2 && a.prep == nullptr) return (int)hipErrorInvalidValue;  // the split mode needs its operand bounds (nesvor_mlp_prepare)
  if (bias_free(net)) {
    // bias-free (mode 4): the pipelined kernel's NOB instantiations for a compact save and for inference; every other case - a full
    // save, shapes the pipelined kernel does not take - on the wide kernels at width 64 (fp32 MFMAs: a valid evaluation of mode 4,
    // the saved fragments in the full-save layout the wide backward reads), with one pass over y for the optional bound
    const size_t lds = fwd_lds_bytes(a.n_linear, kb1);
    const bool pf = use_pf && a.fast && a.off32 && net->n_hidden <= 2 && kb1 <= 2 && ((N >> 4) % (4 * kG)) == 0;
    if (compact) {
      if (!compact_ok(a, net, N)) return (int)hipErrorInvalidValue;
      a.Hm = reinterpret_cast<uint32_t*>(saved_hidden[0]);
      a.H[0] = nullptr;
      if (net->out_dim == 1 && out1_on()) {
        if (net->n_hidden == 1)
          return launch_kb(mlp_fwd_pf_kernel<1, 1, 2, true, true, true, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true, true, true>,
                           mlp_fwd_pf_kernel<2, 1, 2, true, true, true, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true, true, true>, kb1, grid,
                           lds, (hipStream_t)stream, a, 256, n_tiles);
        return launch_kb(mlp_fwd_pf_kernel<1, 2, 2, true, true, true, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true, true, true>,
                         mlp_fwd_pf_kernel<2, 2, 2, true, true, true, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true, true, true>, kb1, grid,
                         lds, (hipStream_t)stream, a, 256, n_tiles);
      }
      if (net->n_hidden == 1)
        return launch_kb(mlp_fwd_pf_kernel<1, 1, 2, true, true, false, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true, false, true>,
                         mlp_fwd_pf_kernel<2, 1, 2, true, true, false, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true, false, true>, kb1, grid,
                         lds, (hipStream_t)stream, a, 256, n_tiles);
      return launch_kb(mlp_fwd_pf_kernel<1, 2, 2, true, true, false, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true, false, true>,
                       mlp_fwd_pf_kernel<2, 2, 2, true, true, false, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true, false, true>, kb1, grid,
                       lds, (hipStream_t)stream, a, 256, n_tiles);
    }
    if (pf && save_none) {
      if (net->n_hidden == 1)
        return launch_kb(mlp_fwd_pf_kernel<1, 1, 2, false, false, false, true>, mlp_fwd_pf_kernel<2, 1, 2, false, false, false, true>,
                         mlp_fwd_pf_kernel<2, 1, 2, false, false, false, true>, mlp_fwd_pf_kernel<2, 1, 2, false, false, false, true>, kb1,
                         grid, lds, (hipStream_t)stream, a, 256, n_tiles);
      return launch_kb(mlp_fwd_pf_kernel<1, 2, 2, false, false, false, true>, mlp_fwd_pf_kernel<2, 2, 2, false, false, false, true>,
                       mlp_fwd_pf_kernel<2, 2, 2, false, false, false, true>, mlp_fwd_pf_kernel<2, 2, 2, false, false, false, true>, kb1,
                       grid, lds, (hipStream_t)stream, a, 256, n_tiles);
    }
    nesvor_mlp_wide_t w{};
    w.width = kWidth; w.n_hidden = net->n_hidden; w.out_dim = net->out_dim; w.k_a = net->k_a; w.k_b = net->k_b; w.b_row0 = net->b_row0;
    w.samples_per_pixel = net->samples_per_pixel;
    for (int l = 0; l <= net->n_hidden; ++l) { w.weight[l] = net->weight[l]; w.bias[l] = nullptr; }
    e = nesvor_mlp_wide_forward(&w, xa, xb, y, save_all ? saved_hidden : nullptr, N, stream);
    if (e || a.y_absmax == nullptr) return e;
    const int64_t work = ((int64_t)net->out_dim * N + 1023) / 1024;
    hipLaunchKernelGGL(absmax_rows_kernel, dim3((unsigned)(work < 2048 ? (work < 1 ? 1 : work) : 2048)), dim3(256), 0, (hipStream_t)stream, y,
                       net->out_dim, N, N, a.y_absmax);
    return (int)hipGetLastError();
  }
  if (compact) {
    if (!compact_ok(a, net, N)) return (int)hipErrorInvalidValue;  // (the caller asks nesvor_mlp_compact_save_ok first)
    a.Hm = reinterpret_cast<uint32_t*>(saved_hidden[0]);
    a.H[0] = nullptr;
    const size_t lds = fwd_lds_bytes(a.n_linear, kb1);
    if (a.hi1) {  // mode 4: the leading term alone
      if (net->out_dim == 1 && out1_on()) {
        if (net->n_hidden == 1)
          return launch_kb(mlp_fwd_pf_kernel<1, 1, 2, true, true, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true, true>,
                           mlp_fwd_pf_kernel<2, 1, 2, true, true, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true, true>, kb1, grid, lds,
                           (hipStream_t)stream, a, 256, n_tiles);
        return launch_kb(mlp_fwd_pf_kernel<1, 2, 2, true, true, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true, true>,
                         mlp_fwd_pf_kernel<2, 2, 2, true, true, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true, true>, kb1, grid, lds,
                         (hipStream_t)stream, a, 256, n_tiles);
      }
      if (net->n_hidden == 1)
        return launch_kb(mlp_fwd_pf_kernel<1, 1, 2, true, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true>, mlp_fwd_pf_kernel<2, 1, 2, true, true>,
                         mlp_fwd_pf_kernel<2, 1, 2, true, true>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles);
      return launch_kb(mlp_fwd_pf_kernel<1, 2, 2, true, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true>, mlp_fwd_pf_kernel<2, 2, 2, true, true>,
                       mlp_fwd_pf_kernel<2, 2, 2, true, true>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles);
    }
    if (net->out_dim == 1 && out1_on()) {  // single output row: VALU output layer
      if (net->n_hidden == 1)
        return launch_kb(mlp_fwd_pf_kernel<1, 1, true, true, true, true>, mlp_fwd_pf_kernel<2, 1, true, true, true, true>,
                         mlp_fwd_pf_kernel<2, 1, true, true, true, true>, mlp_fwd_pf_kernel<2, 1, true, true, true, true>, kb1, grid, lds,
                         (hipStream_t)stream, a, 256, n_tiles);
      return launch_kb(mlp_fwd_pf_kernel<1, 2, true, true, true, true>, mlp_fwd_pf_kernel<2, 2, true, true, true, true>,
                       mlp_fwd_pf_kernel<2, 2, true, true, true, true>, mlp_fwd_pf_kernel<2, 2, true, true, true, true>, kb1, grid, lds,
                       (hipStream_t)stream, a, 256, n_tiles);
    }
    if (net->n_hidden == 1)
      return launch_kb(mlp_fwd_pf_kernel<1, 1, true, true, true>, mlp_fwd_pf_kernel<2, 1, true, true, true>, mlp_fwd_pf_kernel<2, 1, true, true, true>,
                       mlp_fwd_pf_kernel<2, 1, true, true, true>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles);
    return launch_kb(mlp_fwd_pf_kernel<1, 2, true, true, true>, mlp_fwd_pf_kernel<2, 2, true, true, true>, mlp_fwd_pf_kernel<2, 2, true, true, true>,
                     mlp_fwd_pf_kernel<2, 2, true, true, true>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles);
  }
  if (use_pf && a.bf16 != 1 && a.fast && a.off32 && net->n_hidden <= 2 && ((N >> 4) % (4 * kG)) == 0 && (save_all || save_none)) {
    const bool x6 = a.bf16 == 2;
    const size_t lds = fwd_lds_bytes(a.n_linear, kb1);
    if (x6 && a.hi1 && save_none && kb1 <= 2) {  // mode 4, nothing saved (inference): the leading term alone
      if (net->n_hidden == 1)
        return launch_kb(mlp_fwd_pf_kernel<1, 1, 2, false>, mlp_fwd_pf_kernel<2, 1, 2, false>, mlp_fwd_pf_kernel<2, 1, 2, false>,
                         mlp_fwd_pf_kernel<2, 1, 2, false>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles);
      return launch_kb(mlp_fwd_pf_kernel<1, 2, 2, false>, mlp_fwd_pf_kernel<2, 2, 2, false>, mlp_fwd_pf_kernel<2, 2, 2, false>,
                       mlp_fwd_pf_kernel<2, 2, 2, false>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles);
    }
#define NESVOR_PF(NH, SPL, SAVE) launch_kb(mlp_fwd_pf_kernel<1, NH, SPL, SAVE>, mlp_fwd_pf_kernel<2, NH, SPL, SAVE>, \
      mlp_fwd_pf_kernel<3, NH, SPL, SAVE>, mlp_fwd_pf_kernel<4, NH, SPL, SAVE>, kb1, grid, lds, (hipStream_t)stream, a, 256, n_tiles)
    if (net->n_hidden == 1) {
      if (x6) return save_all ? NESVOR_PF(1, true, true) : NESVOR_PF(1, true, false);
      return save_all ? NESVOR_PF(1, false, true) : NESVOR_PF(1, false, false);
    }
    if (x6) return save_all ? NESVOR_PF(2, true, true) : NESVOR_PF(2, true, false);
    return save_all ? NESVOR_PF(2, false, true) : NESVOR_PF(2, false, false);
#undef NESVOR_PF
  }
  // (the split mode of a shape the pipelined kernel does not take: the plain fp32 MFMAs - always a valid evaluation of it)
  if (a.bf16 == 1 && a.half16)
    return launch_kb(mlp_fwd_kernel<1, 2>, mlp_fwd_kernel<2, 2>, mlp_fwd_kernel<3, 2>, mlp_fwd_kernel<4, 2>, kb1,
                     grid, fwd_lds_bytes(a.n_linear, kb1), (hipStream_t)stream, a);
  if (a.bf16 == 1)
    return launch_kb(mlp_fwd_kernel<1, true>, mlp_fwd_kernel<2, true>, mlp_fwd_kernel<3, true>, mlp_fwd_kernel<4, true>, kb1,
                     grid, fwd_lds_bytes(a.n_linear, kb1), (hipStream_t)stream, a);
  return launch_kb(mlp_fwd_kernel<1>, mlp_fwd_kernel<2>, mlp_fwd_kernel<3>, mlp_fwd_kernel<4>, kb1, grid,
                   fwd_lds_bytes(a.n_linear, kb1), (hipStream_t)stream, a);
}

extern "C" int nesvor_mlp_backward(const nesvor_mlp_t* net, const float* xa, const float* xb, const float* dy,
                                   float* const* saved_hidden, float* const* dpre_scratch, float* dxa, float* dxb,
                                   float* dw_partial, int n_partial, int64_t N, void* stream) {
  return nesvor_mlp_backward_bounded(net, xa, xb, dy, saved_hidden, dpre_scratch, dxa, dxb, dw_partial, n_partial, N, nullptr, stream);
}

extern "C" int nesvor_mlp_backward_bounded(const nesvor_mlp_t* net, const float* xa, const float* xb, const float* dy,
                                           float* const* saved_hidden, float* const* dpre_scratch, float* dxa, float* dxb,
                                           float* dw_partial, int n_partial, int64_t N, float* dxb_absmax, void* stream) {
  if (N <= 0) return 0;
  MlpArgs a{};
  int e = fill_args(&a, net, N);
  if (e) return e;
  a.dx_absmax = dxb != nullptr ? dxb_absmax : nullptr;
  if (saved_hidden == nullptr || dpre_scratch == nullptr || dw_partial == nullptr || n_partial < 1) return (int)hipErrorInvalidValue;
  const bool split = a.bf16 == 2;  // fp32 data everywhere; only the MFMA sites differ
  const bool compact = net->compact_save != 0;
  if (split && a.prep == nullptr) return (int)hipErrorInvalidValue;  // the split mode needs its operand bounds (nesvor_mlp_prepare)
  if (compact && (!compact_ok(a, net, N) || dpre_scratch[0] != nullptr)) return (int)hipErrorInvalidValue;
  if (split) a.bf16 = 0;
  a.xa = xa; a.xb = xb; a.y = const_cast<float*>(dy); a.dxa = dxa; a.dxb = dxb; a.dW_partial = dw_partial;
  for (int l = 0; l < kMaxLayers; ++l) {
    a.H[l] = l < net->n_hidden ? saved_hidden[l] : nullptr;
    a.dpre[l] = l < net->n_hidden ? dpre_scratch[l] : nullptr;
  }
  const int kb1 = (net->k_a + net->k_b + 15) / 16;
  if (a.dxa_group && !(a.fast && net->n_hidden <= 2 && dpre_scratch[0] == nullptr)) return (int)hipErrorInvalidValue;
  const bool nob = bias_free(net);
  if (nob && compact) {  // bias-free (mode 4): the compact kernel's NOB instantiations
    a.Hm = reinterpret_cast<uint32_t*>(saved_hidden[0]);
    a.H[0] = nullptr;
    if (net->out_dim == 1 && out1_on()) {
      const size_t lds_o = ws_bwd_lds_bytes(net->n_hidden, kb1, true, true) + sizeof(float) * kWidth;
      if (net->n_hidden == 1)
        return launch_kb(mlp_bwd_ws_kernel<1, 1, 0, 2, true, true, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true, true, true>,
                         mlp_bwd_ws_kernel<2, 1, 0, 2, true, true, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true, true, true>, kb1,
                         dim3((unsigned)n_partial), lds_o, (hipStream_t)stream, a, 512);
      return launch_kb(mlp_bwd_ws_kernel<1, 2, 0, 2, true, true, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true, true, true>,
                       mlp_bwd_ws_kernel<2, 2, 0, 2, true, true, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true, true, true>, kb1,
                       dim3((unsigned)n_partial), lds_o, (hipStream_t)stream, a, 512);
    }
    const size_t lds_c = ws_bwd_lds_bytes(net->n_hidden, kb1, true, true);
    if (net->n_hidden == 1)
      return launch_kb(mlp_bwd_ws_kernel<1, 1, 0, 2, true, false, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true, false, true>,
                       mlp_bwd_ws_kernel<2, 1, 0, 2, true, false, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true, false, true>, kb1,
                       dim3((unsigned)n_partial), lds_c, (hipStream_t)stream, a, 512);
    return launch_kb(mlp_bwd_ws_kernel<1, 2, 0, 2, true, false, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true, false, true>,
                     mlp_bwd_ws_kernel<2, 2, 0, 2, true, false, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true, false, true>, kb1,
                     dim3((unsigned)n_partial), lds_c, (hipStream_t)stream, a, 512);
  }
  // (bias-free without the compact save: the wide pair below - never the wave-specialised kernels above, which write b columns)
  if (nob && dpre_scratch[0] == nullptr) return (int)hipErrorInvalidValue;  // (nesvor_mlp_backward_fused_ok said 0: pass dpre scratch)
  if (compact) {
    a.Hm = reinterpret_cast<uint32_t*>(saved_hidden[0]);
    a.H[0] = nullptr;
    if (a.hi1) {  // mode 4: the leading term alone
      if (net->out_dim == 1 && out1_on()) {
        const size_t lds_o = ws_bwd_lds_bytes(net->n_hidden, kb1, true, true) + sizeof(float) * kWidth;
        if (net->n_hidden == 1)
          return launch_kb(mlp_bwd_ws_kernel<1, 1, 0, 2, true, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true, true>,
                           mlp_bwd_ws_kernel<2, 1, 0, 2, true, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true, true>, kb1,
                           dim3((unsigned)n_partial), lds_o, (hipStream_t)stream, a, 512);
        return launch_kb(mlp_bwd_ws_kernel<1, 2, 0, 2, true, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true, true>,
                         mlp_bwd_ws_kernel<2, 2, 0, 2, true, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true, true>, kb1,
                         dim3((unsigned)n_partial), lds_o, (hipStream_t)stream, a, 512);
      }
      const size_t lds_c = ws_bwd_lds_bytes(net->n_hidden, kb1, true, true);
      if (net->n_hidden == 1)
        return launch_kb(mlp_bwd_ws_kernel<1, 1, 0, 2, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true>, mlp_bwd_ws_kernel<2, 1, 0, 2, true>,
                         mlp_bwd_ws_kernel<2, 1, 0, 2, true>, kb1, dim3((unsigned)n_partial), lds_c, (hipStream_t)stream, a, 512);
      return launch_kb(mlp_bwd_ws_kernel<1, 2, 0, 2, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true>, mlp_bwd_ws_kernel<2, 2, 0, 2, true>,
                       mlp_bwd_ws_kernel<2, 2, 0, 2, true>, kb1, dim3((unsigned)n_partial), lds_c, (hipStream_t)stream, a, 512);
    }
    if (net->out_dim == 1 && out1_on()) {  // single output row: VALU output layer
      const size_t lds_o = ws_bwd_lds_bytes(net->n_hidden, kb1, true, true) + sizeof(float) * kWidth;
      if (net->n_hidden == 1)
        return launch_kb(mlp_bwd_ws_kernel<1, 1, false, true, true, true>, mlp_bwd_ws_kernel<2, 1, false, true, true, true>,
                         mlp_bwd_ws_kernel<2, 1, false, true, true, true>, mlp_bwd_ws_kernel<2, 1, false, true, true, true>, kb1,
                         dim3((unsigned)n_partial), lds_o, (hipStream_t)stream, a, 512);
      return launch_kb(mlp_bwd_ws_kernel<1, 2, false, true, true, true>, mlp_bwd_ws_kernel<2, 2, false, true, true, true>,
                       mlp_bwd_ws_kernel<2, 2, false, true, true, true>, mlp_bwd_ws_kernel<2, 2, false, true, true, true>, kb1,
                       dim3((unsigned)n_partial), lds_o, (hipStream_t)stream, a, 512);
    }
    const size_t lds_c = ws_bwd_lds_bytes(net->n_hidden, kb1, true, true);
    if (net->n_hidden == 1)
      return launch_kb(mlp_bwd_ws_kernel<1, 1, false, true, true>, mlp_bwd_ws_kernel<2, 1, false, true, true>, mlp_bwd_ws_kernel<2, 1, false, true, true>,
                       mlp_bwd_ws_kernel<2, 1, false, true, true>, kb1, dim3((unsigned)n_partial), lds_c, (hipStream_t)stream, a, 512);
    return launch_kb(mlp_bwd_ws_kernel<1, 2, false, true, true>, mlp_bwd_ws_kernel<2, 2, false, true, true>, mlp_bwd_ws_kernel<2, 2, false, true, true>,
                     mlp_bwd_ws_kernel<2, 2, false, true, true>, kb1, dim3((unsigned)n_partial), lds_c, (hipStream_t)stream, a, 512);
  }
  if (net->n_hidden <= 2 && dpre_scratch[0] == nullptr) {
    // fused dX + dW + db (the caller signals it by passing no dpre scratch); grid = n_partial workgroups
    if (ws_ok(a, net)) {  // wave-specialised: 8 waves per workgroup
      const size_t lds_ws = ws_bwd_lds_bytes(net->n_hidden, kb1);
      if (a.bf16 && a.half16) {
        if (net->n_hidden == 1)
          return launch_kb(mlp_bwd_ws_kernel<1, 1, 2>, mlp_bwd_ws_kernel<2, 1, 2>, mlp_bwd_ws_kernel<3, 1, 2>,
                           mlp_bwd_ws_kernel<4, 1, 2>, kb1, dim3((unsigned)n_partial), lds_ws, (hipStream_t)stream, a, 512);
        // (ws_ok admits two hidden layers with at most two input blocks: the wider instantiations are never launched - and the
        //  build's assembly check rejects the register allocation the compiler finds for <4, 2, fp16>)
        return launch_kb(mlp_bwd_ws_kernel<1, 2, 2>, mlp_bwd_ws_kernel<2, 2, 2>, mlp_bwd_ws_kernel<2, 2, 2>,
                         mlp_bwd_ws_kernel<2, 2, 2>, kb1, dim3((unsigned)n_partial), lds_ws, (hipStream_t)stream, a, 512);
      }
      if (a.bf16) {
        if (net->n_hidden == 1)
          return launch_kb(mlp_bwd_ws_kernel<1, 1, true>, mlp_bwd_ws_kernel<2, 1, true>, mlp_bwd_ws_kernel<3, 1, true>,
                           mlp_bwd_ws_kernel<4, 1, true>, kb1, dim3((unsigned)n_partial), lds_ws, (hipStream_t)stream, a, 512);
        return launch_kb(mlp_bwd_ws_kernel<1, 2, true>, mlp_bwd_ws_kernel<2, 2, true>, mlp_bwd_ws_kernel<3, 2, true>,
                         mlp_bwd_ws_kernel<4, 2, true>, kb1, dim3((unsigned)n_partial), lds_ws, (hipStream_t)stream, a, 512);
      }
      if (split) {
        const size_t lds_x6 = ws_bwd_lds_bytes(net->n_hidden, kb1, true);
        if (net->n_hidden == 1)
          return launch_kb(mlp_bwd_ws_kernel<1, 1, false, true>, mlp_bwd_ws_kernel<2, 1, false, true>, mlp_bwd_ws_kernel<3, 1, false, true>,
                           mlp_bwd_ws_kernel<4, 1, false, true>, kb1, dim3((unsigned)n_partial), lds_x6, (hipStream_t)stream, a, 512);
        // (ws_ok admits two hidden layers with at most two input blocks: wider instantiations would never be launched)
        return launch_kb(mlp_bwd_ws_kernel<1, 2, false, true>, mlp_bwd_ws_kernel<2, 2, false, true>, mlp_bwd_ws_kernel<2, 2, false, true>,
                         mlp_bwd_ws_kernel<2, 2, false, true>, kb1, dim3((unsigned)n_partial), lds_x6, (hipStream_t)stream, a, 512);
      }
      if (net->n_hidden == 1)
        return launch_kb(mlp_bwd_ws_kernel<1, 1>, mlp_bwd_ws_kernel<2, 1>, mlp_bwd_ws_kernel<3, 1>, mlp_bwd_ws_kernel<4, 1>,
                         kb1, dim3((unsigned)n_partial), lds_ws, (hipStream_t)stream, a, 512);
      return launch_kb(mlp_bwd_ws_kernel<1, 2>, mlp_bwd_ws_kernel<2, 2>, mlp_bwd_ws_kernel<3, 2>, mlp_bwd_ws_kernel<4, 2>,
                       kb1, dim3((unsigned)n_partial), lds_ws, (hipStream_t)stream, a, 512);
    }
    // no scratch and a shape the wave-specialised kernel does not take (ragged N, S or k_a not multiples of 16, three input
    // blocks at two hidden layers): the caller asks nesvor_mlp_backward_fused_ok first and passes dpre scratch for the
    // two-kernel path below.  (Rounds 1-4 carried a single-role fused kernel for these shapes.)
    return (int)hipErrorInvalidValue;
  }
  if (a.bf16) {
    // modes 1 / 3: the 16-bit pair (mlp_bwd_dx16_kernel, mlp_bwd_dw16_kernel) on the 16-bit fragments the forward saved
    if (xb == nullptr || dy == nullptr || (a.k_a > 0 && xa == nullptr)) return (int)hipErrorInvalidValue;
    for (int l = 0; l < net->n_hidden; ++l)
      if (saved_hidden[l] == nullptr || dpre_scratch[l] == nullptr) return (int)hipErrorInvalidValue;
    if (a.k_a == 0) a.dxa = nullptr;
    const int64_t n_tiles = ((N + 15) / 16 + 4 * kG - 1) / (4 * kG);
    const dim3 grid((unsigned)(n_tiles < 512 ? n_tiles : 512));
    const size_t lds = dx16_lds_bytes(net->n_hidden);
    hipStream_t st = (hipStream_t)stream;
    if (a.half16) {
      hipLaunchKernelGGL(mlp_bwd_dx16_kernel<2>, grid, dim3(256), lds, st, a);
      hipLaunchKernelGGL(mlp_bwd_dw16_kernel<2>, dim3((unsigned)n_partial), dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL(mlp_bwd_dx16_kernel<1>, grid, dim3(256), lds, st, a);
      hipLaunchKernelGGL(mlp_bwd_dw16_kernel<1>, dim3((unsigned)n_partial), dim3(256), 0, st, a);
    }
    return (int)hipGetLastError();
  }
  // dX launch + dW launch on fp32 MFMAs (always a valid evaluation of the split mode): the wide kernels at width 64
  nesvor_mlp_wide_t w{};
  w.width = kWidth; w.n_hidden = net->n_hidden; w.out_dim = net->out_dim; w.k_a = net->k_a; w.k_b = net->k_b; w.b_row0 = net->b_row0;
  w.samples_per_pixel = net->samples_per_pixel;
  for (int l = 0; l <= net->n_hidden; ++l) { w.weight[l] = net->weight[l]; w.bias[l] = net->bias[l]; }  // (bias-free: all NULL)
  return nesvor_mlp_wide_backward_bounded(&w, xa, xb, dy, saved_hidden, dpre_scratch, dxa, dxb, dw_partial, n_partial, N,
                                          dxb != nullptr ? dxb_absmax : nullptr, stream);
}
