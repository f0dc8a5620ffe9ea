// Row toolkit of the fine-tune heads (classify.hip, classify_wide.hip, vqa.hip, grounding.hip): a 256-thread workgroup, four waves,
// works on one row (or, in single-workgroup kernels, on rows t, t + 256, ...).  Plain fp32 VALU code and libm; no atomics.
// The summation order, stated here once: a thread adds its own elements in index order, columns in groups of four as (x + y) + (z + w); the 64
// lanes of a wave by the xor butterfly (wave_sum / wave_max); the four waves as (w0 + w1) + (w2 + w3).  Two runs therefore give the same bits.
// Not for heads.hip: its block_reduce adds the waves left to right behind a leading barrier and gives other bits.
#pragma once
#include "x2_common.h"
#include <math.h>

#define ROW_THREADS 256          // every kernel built on this header launches with exactly this many threads
#define ROW_WAVES (ROW_THREADS / 64)
static_assert(ROW_WAVES == 4, "row_block_sum / row_block_max combine exactly four waves");

// sum / max over the workgroup; red: ROW_WAVES floats of LDS, reusable after the call (two barriers)
__device__ __forceinline__ float row_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ float row_block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}

__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

// erf-GELU through libm, not x2_common.h's fast forms: a few thousand elements per row, and a logit sums H of them.  Two forms of y Phi(y) that
// differ in the last bits and are NOT interchangeable:
//   gelu_erf    1 + erff(.): absolute accuracy, for a value that stays in fp32 (classify.hip's logits accumulate it)
//   gelu_erfc   Phi(y) = erfc(-y / sqrt 2) / 2: erfcf keeps its relative accuracy in the negative tail, where 1 + erff(.) cancels - for a result
//               that is rounded to bf16 (classify_wide.hip's GEMM operand), whose ulp is relative
__device__ __forceinline__ float gelu_erf(float y) { return 0.5f * y * (1.f + erff(y * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erfc(float y) { return 0.5f * y * erfcf(y * -0.70710678118654752f); }
// the derivative of either: Phi(y) + y * phi(y)
__device__ __forceinline__ float dgelu(float y) {
  return 0.5f * (1.f + erff(y * 0.70710678118654752f)) + y * 0.3989422804014327f * expf(-0.5f * y * y);
}

// LayerNorm statistics of one row of n4 float4 groups (H = 4 * n4 columns), two passes: the mean, then the centred sum of squares (biased variance)
__device__ __forceinline__ void row_ln_stats(const float4* __restrict__ x4, int n4, int H, float eps, float* red, float& mean, float& rstd) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n4; i += ROW_THREADS) s += sum4(x4[i]);
  mean = row_block_sum(s, red) / (float)H;
  float q = 0.f;
  for (int i = threadIdx.x; i < n4; i += ROW_THREADS) {
    float4 v = x4[i];
    v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
    q += dot4(v, v);
  }
  rstd = 1.f / sqrtf(row_block_sum(q, red) / (float)H + eps);
}

// The LayerNorm -> GELU backward of a row (cls_tail_bwd_rows_kernel, lngelu_bwd_rows_kernel) is NOT here: with its skeleton as a function template
// over "the upstream da of column group i" hipcc schedules cls_tail_bwd_rows_kernel differently, so both kernels keep their own loops.
