// Wide-label classification head (XVLMForClassification, XVLMForVQAClassification; models/model_classification.py, VQA_msrvtt.py): what stands
// around the logits GEMM of a build_mlp head with hundreds or thousands of labels.  csrc/classify.hip keeps all C accumulators of a row in registers
// and stops at C = 16; here the logits [R, Cp] come from the MFMA GEMM (x2_gemm_nt on the bf16 activation and the zero-padded bf16 weight) and these
// kernels do the row work before and after it:
//   x2_lngelu_fwd         per row: mean / biased variance (two passes), erf-GELU(xhat * gamma + beta) -> bf16 act (the GEMM operand), {mean, rstd}
//   x2_soft_ce_fwd        per row: lse over columns [0, C), rowloss = sum_j w_j (lse - z[t_j]) over the row's entries offs[r] .. offs[r+1]-1; then
//                         one workgroup: stat = {sum rowloss / denom, denom}, denom = R or the number of non-skipped entries
//   x2_kl_ce_fwd          per row: lse of the logits and of the teacher, rowloss = sum_c p_c ((t_c - lse_t) - (z_c - lse)); stat = {sum / R, R}
//   x2_soft_ce_bwd        per row: dlogits bf16 [R, Cp] = g_logits + g_loss / denom (Wr softmax(z) - sum_{j: t_j = c} w_j), pad columns zero
//   x2_kl_ce_bwd          per row: dlogits bf16 [R, Cp] = g_logits + g_loss / R (softmax(z) - p), pad columns zero
//   x2_lngelu_bwd         per row: dy = dact gelu'(y), LayerNorm's backward -> dh; then one thread per column walks the rows for dgamma / dbeta
//   x2_cls_accuracy_rows  per row: pred = lowest index of the maximum over [0, C), hit = (pred == label); then one workgroup: counts += {sum hit, R}
// The pad columns [C, Cp) of the logits hold 0 (zero weight rows, zero bias), not -inf: every kernel reads columns [0, C) only, and never a column
// at or beyond C of any input (tests fill them with NaN).
// Plain fp32 arithmetic, no atomics, libm erff / erfcf / expf / logf.  Fixed summation orders, so two runs give the same bits:
//   a row sum      x2_rowblock.h's order over groups of four columns (group i = columns 4i .. 4i+3, missing columns contribute the neutral
//                  element); row maxima the same way (order-free anyway).  Whether a group is read as one float4 (16-byte aligned base and a
//                  leading dimension % 4 == 0) or as four scalars does not change the arithmetic.
//   entries        rowloss, Wr and the per-column sum over duplicate targets run over the row's entries in index order (one thread; the backward
//                  stages the entries in LDS in chunks of 256 and every column's owner walks each chunk in index order) - no maximum k.
//   over rows      launch two of a forward: thread t adds rows t, t + 256, ... in order, then the block sum above; the non-skipped count is an
//                  integer.  dgamma / dbeta: one thread's walk over rows 0..R-1.
// An entry whose target is outside [0, C) (the -100 of ignore_index) is skipped: it adds nothing to rowloss, Wr, the count or dlogits.  A row
// without entries has rowloss 0 and only g_logits in its dlogits.  denom_mode 1 with no non-skipped entry at all gives 0 / 0 = NaN, as
// F.cross_entropy(ignore_index=-100) does.  A teacher probability that underflows to 0 contributes 0 (torch's xlogy rule).
// Tie rule of the accuracy: the lowest index of bit-equal maxima wins (prediction.max(1)); NaN logits are outside the contract; a label of -100
// (or any label that is no column) is a miss.
#include "x2_rowblock.h"
#include <limits.h>

#define CW_THREADS ROW_THREADS
#define CW_COLS 64               // lngelu backward launch two: columns per workgroup, rows per staged chunk of {mean, rstd}
#define CW_CHUNK 256             // entries of a row staged in LDS at a time
#define CW_MAXR 65536
#define CW_MAXH 16384
#define CW_MAXC (1 << 20)
static_assert(CW_CHUNK == CW_THREADS, "one staged entry per thread");

#define CW_ALIGNED(p, n) ((((uintptr_t)(p)) & ((n) - 1)) == 0)
#define CW_VEC(p, ld) (CW_ALIGNED(p, 16) && (ld) % 4 == 0)          // rows may be read as float4

// columns 4g .. 4g+3 of a row of C readable columns; a column at or beyond C is never read and comes back as `fill`
__device__ __forceinline__ float4 cw_load4(const float* __restrict__ row, int g, int C, bool vec, float fill) {
  const int c = g << 2;
  if (vec && c + 3 < C) return *reinterpret_cast<const float4*>(row + c);
  float4 v;
  v.x = c < C ? row[c] : fill;
  v.y = c + 1 < C ? row[c + 1] : fill;
  v.z = c + 2 < C ? row[c + 2] : fill;
  v.w = c + 3 < C ? row[c + 3] : fill;
  return v;
}
__device__ __forceinline__ void cw_store_bf16x4(bf16_t* __restrict__ dst, const float4& v) {
  uint2 o;
  o.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
  o.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
  *reinterpret_cast<uint2*>(dst) = o;
}

// log-sum-exp of columns [0, C) of a row: the maximum, then the sum of exp(z - max)
__device__ __forceinline__ float cw_row_lse(const float* __restrict__ row, int C, bool vec, float* red) {
  const int ng = (C + 3) >> 2;
  float m = -INFINITY;
  for (int g = threadIdx.x; g < ng; g += CW_THREADS) {
    const float4 v = cw_load4(row, g, C, vec, -INFINITY);
    m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
  }
  m = row_block_max(m, red);
  float s = 0.f;
  for (int g = threadIdx.x; g < ng; g += CW_THREADS) {
    const float4 v = cw_load4(row, g, C, vec, -INFINITY);           // exp(-inf - m) = 0: the neutral element of the sum
    float4 e;
    e.x = expf(v.x - m); e.y = expf(v.y - m); e.z = expf(v.z - m); e.w = expf(v.w - m);
    s += sum4(e);
  }
  s = row_block_sum(s, red);
  return m + logf(s);
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm -> GELU, forward
__global__ __launch_bounds__(CW_THREADS) void lngelu_fwd_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int H, float eps, bf16_t* __restrict__ act, int lda,
                                                                float* __restrict__ rowstat) {
  __shared__ float red[CW_THREADS / 64];
  const int r = blockIdx.x, n4 = H >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(h + (size_t)r * ldh);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  bf16_t* arow = act + (size_t)r * lda;
  float mean, rstd;
  row_ln_stats(x4, n4, H, eps, red, mean, rstd);
  for (int i = threadIdx.x; i < n4; i += CW_THREADS) {
    const float4 v = x4[i], g = g4[i], b = b4[i];
    float4 a;
    a.x = gelu_erfc((v.x - mean) * rstd * g.x + b.x); a.y = gelu_erfc((v.y - mean) * rstd * g.y + b.y);
    a.z = gelu_erfc((v.z - mean) * rstd * g.z + b.z); a.w = gelu_erfc((v.w - mean) * rstd * g.w + b.w);
    cw_store_bf16x4(arow + 4 * i, a);
  }
  if (threadIdx.x == 0) {
    rowstat[2 * r] = mean;
    rowstat[2 * r + 1] = rstd;
  }
}

#define CW_REQUIRE_RH(name)                                                                                                        \
  X2_REQUIRE(R >= 1 && R <= CW_MAXR, name ": R=%d must be in 1..%d", R, CW_MAXR);                                                   \
  X2_REQUIRE(H >= 4 && H <= CW_MAXH && H % 4 == 0, name ": H=%d must be a multiple of 4 in 4..%d", H, CW_MAXH)
#define CW_REQUIRE_RC(name)                                                                                                        \
  X2_REQUIRE(R >= 1 && R <= CW_MAXR, name ": R=%d must be in 1..%d", R, CW_MAXR);                                                   \
  X2_REQUIRE(C >= 2 && C <= CW_MAXC, name ": C=%d must be in 2..%d", C, CW_MAXC)

extern "C" int x2_lngelu_fwd(const float* h, int ldh, const float* gamma, const float* beta, int R, int H, float eps, void* act, int lda,
                             float* rowstat, void* stream) {
  X2_REQUIRE(h && gamma && beta && act && rowstat, "x2_lngelu_fwd: null tensor");
  CW_REQUIRE_RH("x2_lngelu_fwd");
  X2_REQUIRE(ldh >= H && ldh % 4 == 0, "x2_lngelu_fwd: ldh=%d must be a multiple of 4 and at least H=%d", ldh, H);
  X2_REQUIRE(lda >= H && lda % 4 == 0, "x2_lngelu_fwd: lda=%d must be a multiple of 4 and at least H=%d", lda, H);
  X2_REQUIRE(CW_ALIGNED(h, 16) && CW_ALIGNED(gamma, 16) && CW_ALIGNED(beta, 16) && CW_ALIGNED(act, 8),
             "x2_lngelu_fwd: h, gamma and beta must be 16-byte aligned, act 8-byte aligned");
  hipLaunchKernelGGL(lngelu_fwd_kernel, dim3(R), dim3(CW_THREADS), 0, (hipStream_t)stream, h, ldh, gamma, beta, H, eps, (bf16_t*)act, lda, rowstat);
  return x2_check_launch("x2_lngelu_fwd");
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm -> GELU, backward
// launch one: a workgroup per row -> dh
__global__ __launch_bounds__(CW_THREADS) void lngelu_bwd_rows_kernel(const float* __restrict__ dact, int ldd, const float* __restrict__ h, int ldh,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ rowstat, int H, float* __restrict__ dh, int lddh) {
  __shared__ float red[CW_THREADS / 64];
  const int r = blockIdx.x, n4 = H >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(h + (size_t)r * ldh);
  const float4* a4 = reinterpret_cast<const float4*>(dact + (size_t)r * ldd);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  float4* d4 = reinterpret_cast<float4*>(dh + (size_t)r * lddh);
  const float mean = rowstat[2 * r], rstd = rowstat[2 * r + 1];
  // dxhat = dact * gelu'(y) * gamma of four columns, and their xhat
  auto dxhat4 = [&](int i, float4& xh) -> float4 {
    const float4 v = x4[i], g = g4[i], b = b4[i], da = a4[i];
    xh.x = (v.x - mean) * rstd; xh.y = (v.y - mean) * rstd; xh.z = (v.z - mean) * rstd; xh.w = (v.w - mean) * rstd;
    float4 d;
    d.x = da.x * dgelu(xh.x * g.x + b.x) * g.x; d.y = da.y * dgelu(xh.y * g.y + b.y) * g.y;
    d.z = da.z * dgelu(xh.z * g.z + b.z) * g.z; d.w = da.w * dgelu(xh.w * g.w + b.w) * g.w;
    return d;
  };
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < n4; i += CW_THREADS) {
    float4 xh;
    const float4 d = dxhat4(i, xh);
    s1 += sum4(d);
    s2 += dot4(d, xh);
  }
  s1 = row_block_sum(s1, red) / (float)H;
  s2 = row_block_sum(s2, red) / (float)H;
  for (int i = threadIdx.x; i < n4; i += CW_THREADS) {          // the same arithmetic again instead of an [H] row kept somewhere
    float4 xh;
    float4 d = dxhat4(i, xh);
    d.x = rstd * (d.x - s1 - xh.x * s2); d.y = rstd * (d.y - s1 - xh.y * s2);
    d.z = rstd * (d.z - s1 - xh.z * s2); d.w = rstd * (d.w - s1 - xh.w * s2);
    d4[i] = d;
  }
}

// launch two: one thread per column j walks rows 0..R-1 in order; a workgroup owns CW_COLS columns and stages {mean, rstd} of CW_COLS rows at a time
__global__ __launch_bounds__(CW_COLS) void lngelu_bwd_cols_kernel(const float* __restrict__ dact, int ldd, const float* __restrict__ h, int ldh,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ rowstat, int R, int H, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta) {
  __shared__ float smean[CW_COLS], srstd[CW_COLS];
  const int t = threadIdx.x, j = blockIdx.x * CW_COLS + t;
  const bool active = j < H;
  const float gam = active ? gamma[j] : 0.f, bet = active ? beta[j] : 0.f;
  float dg = 0.f, db = 0.f;
  for (int r0 = 0; r0 < R; r0 += CW_COLS) {
    __syncthreads();                                  // the previous chunk has been read by every column
    if (r0 + t < R) {
      smean[t] = rowstat[2 * (r0 + t)];
      srstd[t] = rowstat[2 * (r0 + t) + 1];
    }
    __syncthreads();
    const int nr = min(CW_COLS, R - r0);
    if (active) {
      const float* col = h + (size_t)r0 * ldh + j;
      const float* dcol = dact + (size_t)r0 * ldd + j;
#pragma unroll 4
      for (int k = 0; k < nr; ++k) {
        const float xh = (col[(size_t)k * ldh] - smean[k]) * srstd[k];
        const float dy = dcol[(size_t)k * ldd] * dgelu(xh * gam + bet);
        dg += dy * xh;
        db += dy;
      }
    }
  }
  if (active) {
    dgamma[j] = dg;
    dbeta[j] = db;
  }
}

extern "C" int x2_lngelu_bwd(const float* dact, int ldd, const float* h, int ldh, const float* gamma, const float* beta, const float* rowstat, int R,
                             int H, float* dh, int lddh, float* dgamma, float* dbeta, void* stream) {
  X2_REQUIRE(dact && h && gamma && beta && rowstat && dh && dgamma && dbeta, "x2_lngelu_bwd: null tensor");
  CW_REQUIRE_RH("x2_lngelu_bwd");
  X2_REQUIRE(ldd >= H && ldd % 4 == 0 && ldh >= H && ldh % 4 == 0 && lddh >= H && lddh % 4 == 0,
             "x2_lngelu_bwd: ldd=%d, ldh=%d and lddh=%d must be multiples of 4 and at least H=%d", ldd, ldh, lddh, H);
  X2_REQUIRE(CW_ALIGNED(dact, 16) && CW_ALIGNED(h, 16) && CW_ALIGNED(gamma, 16) && CW_ALIGNED(beta, 16) && CW_ALIGNED(dh, 16),
             "x2_lngelu_bwd: dact, h, gamma, beta and dh must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lngelu_bwd_rows_kernel, dim3(R), dim3(CW_THREADS), 0, st, dact, ldd, h, ldh, gamma, beta, rowstat, H, dh, lddh);
  hipLaunchKernelGGL(lngelu_bwd_cols_kernel, dim3((H + CW_COLS - 1) / CW_COLS), dim3(CW_COLS), 0, st, dact, ldd, h, ldh, gamma, beta, rowstat, R, H,
                     dgamma, dbeta);
  return x2_check_launch("x2_lngelu_bwd");
}

// ---------------------------------------------------------------------------------------------------------------- soft cross-entropy, forward
// launch one: a workgroup per row.  targets == NULL: only lse is written (no loss asked for).
__global__ __launch_bounds__(CW_THREADS) void soft_ce_rows_kernel(const float* __restrict__ logits, int ldl, int vec, int C,
                                                                  const int* __restrict__ offs, const long* __restrict__ targets,
                                                                  const float* __restrict__ weights, float* __restrict__ lse,
                                                                  float* __restrict__ rowloss) {
  __shared__ float red[CW_THREADS / 64];
  const int r = blockIdx.x;
  const float* row = logits + (size_t)r * ldl;
  const float l = cw_row_lse(row, C, vec != 0, red);
  if (threadIdx.x == 0) {
    lse[r] = l;
    if (targets) {
      float out = 0.f;
      const int e1 = offs[r + 1];
      for (int e = offs[r]; e < e1; ++e) {                          // index order
        const long t = targets[e];
        if (t >= 0 && t < C) out += (weights ? weights[e] : 1.f) * (l - row[t]);
      }
      rowloss[r] = out;
    }
  }
}

// launch two: one workgroup.  stat = {sum_r rowloss / denom, denom}; denom = R (mode 0) or the number of non-skipped entries of all rows (mode 1)
__global__ __launch_bounds__(CW_THREADS) void soft_ce_mean_kernel(const float* __restrict__ rowloss, int R, int C, const int* __restrict__ offs,
                                                                  const long* __restrict__ targets, int denom_mode, float* __restrict__ stat) {
  __shared__ float red[CW_THREADS / 64];
  __shared__ int ired[CW_THREADS / 64];
  float s = 0.f;
  for (int r = threadIdx.x; r < R; r += CW_THREADS) s += rowloss[r];
  s = row_block_sum(s, red);
  float denom = (float)R;
  if (denom_mode == 1) {
    int n = 0;
    const int e1 = offs[R];
    for (int e = offs[0] + threadIdx.x; e < e1; e += CW_THREADS) {
      const long t = targets[e];
      n += (t >= 0 && t < C) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) ired[threadIdx.x >> 6] = n;
    __syncthreads();
    denom = (float)((ired[0] + ired[1]) + (ired[2] + ired[3]));
  }
  if (threadIdx.x == 0) {
    stat[0] = s / denom;
    stat[1] = denom;
  }
}

extern "C" int x2_soft_ce_fwd(const float* logits, int ldl, int R, int C, const int* offs, const long* targets, const float* weights, int denom_mode,
                              float* lse, float* rowloss, float* stat, void* stream) {
  X2_REQUIRE(logits && lse, "x2_soft_ce_fwd: null tensor");
  X2_REQUIRE(offs, "x2_soft_ce_fwd: null offs (int32 [R + 1] is required)");
  X2_REQUIRE(!targets || (rowloss && stat), "x2_soft_ce_fwd: targets need rowloss and stat");
  X2_REQUIRE(targets || !weights, "x2_soft_ce_fwd: weights without targets");
  CW_REQUIRE_RC("x2_soft_ce_fwd");
  X2_REQUIRE(ldl >= C, "x2_soft_ce_fwd: ldl=%d must be at least C=%d", ldl, C);
  X2_REQUIRE(denom_mode == 0 || denom_mode == 1, "x2_soft_ce_fwd: denom_mode=%d must be 0 (rows) or 1 (non-skipped entries)", denom_mode);
  X2_REQUIRE(CW_ALIGNED(logits, 4) && CW_ALIGNED(lse, 4) && CW_ALIGNED(offs, 4) && CW_ALIGNED(targets, 8) && CW_ALIGNED(weights, 4),
             "x2_soft_ce_fwd: tensors must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(soft_ce_rows_kernel, dim3(R), dim3(CW_THREADS), 0, st, logits, ldl, CW_VEC(logits, ldl) ? 1 : 0, C, offs, targets, weights, lse,
                     rowloss);
  if (targets) hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(CW_THREADS), 0, st, rowloss, R, C, offs, targets, denom_mode, stat);
  return x2_check_launch("x2_soft_ce_fwd");
}

// ---------------------------------------------------------------------------------------------------------------- KL to a dense teacher, forward
__global__ __launch_bounds__(CW_THREADS) void kl_ce_rows_kernel(const float* __restrict__ logits, int ldl, int vec, const float* __restrict__ teacher,
                                                                int ldt, int vect, int C, float* __restrict__ lse, float* __restrict__ lse_t,
                                                                float* __restrict__ rowloss) {
  __shared__ float red[CW_THREADS / 64];
  const int r = blockIdx.x, ng = (C + 3) >> 2;
  const float* zrow = logits + (size_t)r * ldl;
  const float* trow = teacher + (size_t)r * ldt;
  const float lz = cw_row_lse(zrow, C, vec != 0, red);
  const float lt = cw_row_lse(trow, C, vect != 0, red);
  auto term = [&](float t, float z) -> float {
    const float p = expf(t - lt);                     // t = -inf on a missing column: p = 0
    return p > 0.f ? p * ((t - lt) - (z - lz)) : 0.f;
  };
  float s = 0.f;
  for (int g = threadIdx.x; g < ng; g += CW_THREADS) {
    const float4 t = cw_load4(trow, g, C, vect != 0, -INFINITY), z = cw_load4(zrow, g, C, vec != 0, 0.f);
    float4 k;
    k.x = term(t.x, z.x); k.y = term(t.y, z.y); k.z = term(t.z, z.z); k.w = term(t.w, z.w);
    s += sum4(k);
  }
  s = row_block_sum(s, red);
  if (threadIdx.x == 0) {
    lse[r] = lz;
    lse_t[r] = lt;
    rowloss[r] = s;
  }
}

extern "C" int x2_kl_ce_fwd(const float* logits, int ldl, const float* teacher, int ldt, int R, int C, float* lse, float* lse_t, float* rowloss,
                            float* stat, void* stream) {
  X2_REQUIRE(logits && teacher && lse && lse_t && rowloss && stat, "x2_kl_ce_fwd: null tensor");
  CW_REQUIRE_RC("x2_kl_ce_fwd");
  X2_REQUIRE(ldl >= C && ldt >= C, "x2_kl_ce_fwd: ldl=%d and ldt=%d must be at least C=%d", ldl, ldt, C);
  X2_REQUIRE(CW_ALIGNED(logits, 4) && CW_ALIGNED(teacher, 4) && CW_ALIGNED(lse, 4) && CW_ALIGNED(lse_t, 4) && CW_ALIGNED(rowloss, 4),
             "x2_kl_ce_fwd: tensors must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kl_ce_rows_kernel, dim3(R), dim3(CW_THREADS), 0, st, logits, ldl, CW_VEC(logits, ldl) ? 1 : 0, teacher, ldt,
                     CW_VEC(teacher, ldt) ? 1 : 0, C, lse, lse_t, rowloss);
  hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(CW_THREADS), 0, st, rowloss, R, C, (const int*)nullptr, (const long*)nullptr, 0, stat);
  return x2_check_launch("x2_kl_ce_fwd");
}

// ---------------------------------------------------------------------------------------------------------------- backward: dlogits as bf16 [R, Cp]
// One workgroup per row; thread t owns column groups t, t + 256, ... of the Cp / 4 groups.  mode 0: g_logits only; 1: soft CE; 2: KL.
__global__ __launch_bounds__(CW_THREADS) void ce_bwd_kernel(int mode, const float* __restrict__ logits, int ldl, int vec, int C, int Cp,
                                                            const int* __restrict__ offs, const long* __restrict__ targets,
                                                            const float* __restrict__ weights, const float* __restrict__ teacher, int ldt, int vect,
                                                            const float* __restrict__ lse, const float* __restrict__ lse_t,
                                                            const float* __restrict__ stat, float inv_rows, const float* __restrict__ g_loss,
                                                            const float* __restrict__ g_logits, int ldg, int vecg, bf16_t* __restrict__ dl, int lddl) {
  __shared__ int st[CW_CHUNK];                        // staged targets (-1: skipped)
  __shared__ float sw[CW_CHUNK];                      // staged weights
  __shared__ float s_wr;
  const int r = blockIdx.x, ngp = Cp >> 2;
  const float* zrow = logits ? logits + (size_t)r * ldl : nullptr;
  const float* trow = teacher ? teacher + (size_t)r * ldt : nullptr;
  const float* grow = g_logits ? g_logits + (size_t)r * ldg : nullptr;
  bf16_t* drow = dl + (size_t)r * lddl;
  float scale = 0.f, lz = 0.f, lt = 0.f, wr = 0.f;
  int e0 = 0, ne = 0;
  if (mode != 0) {
    scale = mode == 1 ? g_loss[0] / stat[1] : g_loss[0] * inv_rows;
    lz = lse[r];
  }
  if (mode == 2) lt = lse_t[r];
  // stage entries e0 + c0 .. of the row: one per thread
  auto stage = [&](int c0) {
    const int i = c0 + threadIdx.x;
    if (i < ne) {
      const long t = targets[e0 + i];
      const bool ok = t >= 0 && t < C;
      st[threadIdx.x] = ok ? (int)t : -1;
      sw[threadIdx.x] = ok ? (weights ? weights[e0 + i] : 1.f) : 0.f;
    }
  };
  if (mode == 1) {
    e0 = offs[r];
    ne = max(offs[r + 1] - e0, 0);
    for (int c0 = 0; c0 < ne; c0 += CW_CHUNK) {                     // Wr: the non-skipped weights in index order
      __syncthreads();
      stage(c0);
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = min(CW_CHUNK, ne - c0);
        for (int i = 0; i < n; ++i)
          if (st[i] >= 0) wr += sw[i];
      }
    }
    if (threadIdx.x == 0) s_wr = wr;
    __syncthreads();
    wr = s_wr;
  }
  const bool one = ne <= CW_CHUNK;                    // the chunk staged above is the whole row: it stays
  for (int g0 = 0; g0 < ngp; g0 += CW_THREADS) {      // uniform trip count: every thread takes part in the staging
    const int g = g0 + threadIdx.x, c = g << 2;
    float4 sub = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode == 1) {
      for (int c0 = 0; c0 < ne; c0 += CW_CHUNK) {
        if (!one) {
          __syncthreads();
          stage(c0);
          __syncthreads();
        }
        const int n = min(CW_CHUNK, ne - c0);
        for (int i = 0; i < n; ++i) {                               // LDS broadcasts; duplicates of a column add in index order
          const int t = st[i];
          if ((t >> 2) == g) {                                      // t = -1 gives -1: no group
            const float w = sw[i];
            const int k = t & 3;
            if (k == 0) sub.x += w; else if (k == 1) sub.y += w; else if (k == 2) sub.z += w; else sub.w += w;
          }
        }
      }
    }
    if (g < ngp) {
      float4 d = grow ? cw_load4(grow, g, C, vecg != 0, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (mode != 0 && c < C) {
        const float4 z = cw_load4(zrow, g, C, vec != 0, -INFINITY);   // exp(-inf) = 0 on a pad column
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        float mul = wr;
        if (mode == 2) {
          const float4 t = cw_load4(trow, g, C, vect != 0, -INFINITY);
          p.x = expf(t.x - lt); p.y = expf(t.y - lt); p.z = expf(t.z - lt); p.w = expf(t.w - lt);
          mul = 1.f;
        } else {
          p = sub;
        }
        d.x += scale * (mul * expf(z.x - lz) - p.x); d.y += scale * (mul * expf(z.y - lz) - p.y);
        d.z += scale * (mul * expf(z.z - lz) - p.z); d.w += scale * (mul * expf(z.w - lz) - p.w);
        if (c + 1 >= C) d.y = 0.f;                                  // pad columns: exactly zero whatever scale is (inf * 0)
        if (c + 2 >= C) d.z = 0.f;
        if (c + 3 >= C) d.w = 0.f;
      }
      cw_store_bf16x4(drow + c, d);
    }
  }
}

#define CW_REQUIRE_DL(name)                                                                                                                  \
  X2_REQUIRE(Cp >= C && Cp % 4 == 0 && lddl >= Cp && lddl % 4 == 0, name ": Cp=%d must be a multiple of 4 and at least C=%d, lddl=%d a multiple of 4 " \
             "and at least Cp", Cp, C, lddl);                                                                                               \
  X2_REQUIRE(!g_logits || ldg >= C, name ": ldg=%d must be at least C=%d", ldg, C);                                                           \
  X2_REQUIRE(CW_ALIGNED(dl, 8) && CW_ALIGNED(logits, 4) && CW_ALIGNED(g_logits, 4), name ": dl must be 8-byte aligned, fp32 tensors 4-byte aligned")

extern "C" int x2_soft_ce_bwd(const float* logits, int ldl, int R, int C, const int* offs, const long* targets, const float* weights, const float* lse,
                              const float* stat, const float* g_loss, const float* g_logits, int ldg, void* dl, int lddl, int Cp, void* stream) {
  X2_REQUIRE(dl, "x2_soft_ce_bwd: null dl");
  X2_REQUIRE(!g_loss || (logits && offs && targets && lse && stat), "x2_soft_ce_bwd: g_loss needs logits, offs, targets, lse and the forward's stat");
  CW_REQUIRE_RC("x2_soft_ce_bwd");
  X2_REQUIRE(!g_loss || ldl >= C, "x2_soft_ce_bwd: ldl=%d must be at least C=%d", ldl, C);
  CW_REQUIRE_DL("x2_soft_ce_bwd");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(R), dim3(CW_THREADS), 0, (hipStream_t)stream, g_loss ? 1 : 0, logits, ldl, CW_VEC(logits, ldl) ? 1 : 0, C, Cp,
                     offs, targets, weights, (const float*)nullptr, 0, 0, lse, (const float*)nullptr, stat, 0.f, g_loss, g_logits, ldg,
                     CW_VEC(g_logits, ldg) ? 1 : 0, (bf16_t*)dl, lddl);
  return x2_check_launch("x2_soft_ce_bwd");
}

extern "C" int x2_kl_ce_bwd(const float* logits, int ldl, const float* teacher, int ldt, int R, int C, const float* lse, const float* lse_t,
                            const float* g_loss, const float* g_logits, int ldg, void* dl, int lddl, int Cp, void* stream) {
  X2_REQUIRE(dl, "x2_kl_ce_bwd: null dl");
  X2_REQUIRE(!g_loss || (logits && teacher && lse && lse_t), "x2_kl_ce_bwd: g_loss needs logits, teacher, lse and lse_t");
  CW_REQUIRE_RC("x2_kl_ce_bwd");
  X2_REQUIRE(!g_loss || (ldl >= C && ldt >= C), "x2_kl_ce_bwd: ldl=%d and ldt=%d must be at least C=%d", ldl, ldt, C);
  CW_REQUIRE_DL("x2_kl_ce_bwd");
  X2_REQUIRE(CW_ALIGNED(teacher, 4), "x2_kl_ce_bwd: teacher must be 4-byte aligned");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(R), dim3(CW_THREADS), 0, (hipStream_t)stream, g_loss ? 2 : 0, logits, ldl, CW_VEC(logits, ldl) ? 1 : 0, C, Cp,
                     (const int*)nullptr, (const long*)nullptr, (const float*)nullptr, teacher, ldt, CW_VEC(teacher, ldt) ? 1 : 0, lse, lse_t,
                     (const float*)nullptr, 1.f / (float)R, g_loss, g_logits, ldg, CW_VEC(g_logits, ldg) ? 1 : 0, (bf16_t*)dl, lddl);
  return x2_check_launch("x2_kl_ce_bwd");
}

// ---------------------------------------------------------------------------------------------------------------- accuracy
// launch one: a workgroup per row.  (value, index) pairs; the better pair has the larger value, on bit-equal values the lower index.
__device__ __forceinline__ void cw_better(float& m, int& idx, float om, int oi) {
  if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
}
__global__ __launch_bounds__(CW_THREADS) void cls_argmax_rows_kernel(const float* __restrict__ logits, int ldl, int vec, const long* __restrict__ labels,
                                                                     int C, int* __restrict__ pred, int* __restrict__ hit) {
  __shared__ float rm[CW_THREADS / 64];
  __shared__ int ri[CW_THREADS / 64];
  const int r = blockIdx.x, ng = (C + 3) >> 2;
  const float* row = logits + (size_t)r * ldl;
  float m = -INFINITY;
  int idx = INT_MAX;                                  // a thread without columns, or with -inf only, defers to any real column
  for (int g = threadIdx.x; g < ng; g += CW_THREADS) {
    const float4 v = cw_load4(row, g, C, vec != 0, -INFINITY);
    const int c = g << 2;
    cw_better(m, idx, v.x, c);                        // ascending columns: a strict > keeps the lowest index, the == arm only replaces INT_MAX
    if (c + 1 < C) cw_better(m, idx, v.y, c + 1);
    if (c + 2 < C) cw_better(m, idx, v.z, c + 2);
    if (c + 3 < C) cw_better(m, idx, v.w, c + 3);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    cw_better(m, idx, om, oi);
  }
  if ((threadIdx.x & 63) == 0) { rm[threadIdx.x >> 6] = m; ri[threadIdx.x >> 6] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < CW_THREADS / 64; ++w) cw_better(m, idx, rm[w], ri[w]);
    pred[r] = idx;
    hit[r] = labels[r] == (long)idx ? 1 : 0;
  }
}

// launch two: one workgroup; the count is an integer sum.  Launches on one stream are ordered: a plain read-modify-write accumulates.
__global__ __launch_bounds__(CW_THREADS) void cls_hits_kernel(const int* __restrict__ hit, int R, long* __restrict__ counts) {
  __shared__ int red[CW_THREADS / 64];
  int n = 0;
  for (int r = threadIdx.x; r < R; r += CW_THREADS) n += hit[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] += (long)((red[0] + red[1]) + (red[2] + red[3]));
    counts[1] += (long)R;
  }
}

extern "C" int x2_cls_accuracy_rows(const float* logits, int ldl, const long* labels, int R, int C, int* pred, int* hit, long* counts, void* stream) {
  X2_REQUIRE(logits && labels && pred && hit && counts, "x2_cls_accuracy_rows: null tensor");
  CW_REQUIRE_RC("x2_cls_accuracy_rows");
  X2_REQUIRE(ldl >= C, "x2_cls_accuracy_rows: ldl=%d must be at least C=%d", ldl, C);
  X2_REQUIRE(CW_ALIGNED(logits, 4) && CW_ALIGNED(labels, 8) && CW_ALIGNED(pred, 4) && CW_ALIGNED(hit, 4) && CW_ALIGNED(counts, 8),
             "x2_cls_accuracy_rows: tensors must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cls_argmax_rows_kernel, dim3(R), dim3(CW_THREADS), 0, st, logits, ldl, CW_VEC(logits, ldl) ? 1 : 0, labels, C, pred, hit);
  hipLaunchKernelGGL(cls_hits_kernel, dim3(1), dim3(CW_THREADS), 0, st, hit, R, counts);
  return x2_check_launch("x2_cls_accuracy_rows");
}
