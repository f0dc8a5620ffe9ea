// Classification fine-tunes (XVLMForNLVR, models/model_classification.py; NLVR.py): the tail of a build_mlp head behind its first Linear,
// LayerNorm(1e-5) -> GELU -> Linear(H -> C) -> F.cross_entropy(ignore_index=-100), and the evaluation loop's accuracy.
//   x2_cls_tail_fwd   per row: mean / variance (two passes), xhat * gamma + beta, erf-GELU, the C dot products + bias, the row's nll; then the mean
//                     over the valid rows in a second, single-workgroup launch (skipped without labels)
//   x2_cls_tail_bwd   per row: dlogits, dlogits @ w, GELU', LayerNorm's backward -> dh; then one thread per column walks the rows in index order
//                     for dgamma / dbeta / dw (and dbias), recomputing xhat, y and gelu(y) from h and {mean, rstd}
//   x2_cls_accuracy   pred = lowest index of the row maximum (prediction.max(1)), counts += {rows with pred == label, R}, one workgroup
// Replaces ops.layer_norm + ops.gelu + ops.linear + ops.cross_entropy: four launches forward and about a dozen backward (with their partial-sum
// reductions).  H is at most 16384 and C at most 16, so this is plain fp32 VALU code; what it saves is launches and the [R, H] intermediates: nothing
// of that size lives between forward and backward besides h itself.
// No atomics.  Every sum has a fixed order (x2_rowblock.h; the column sums of the backward are one thread's walk over rows 0..R-1), so two runs
// give the same bits.  The GELU is x2_rowblock.h's gelu_erf.
// Sub-gradients: none - LayerNorm, erf-GELU and log-softmax are smooth.  Tie rule of the accuracy: strict >, so the lowest index of equal maxima wins.
// Labels: [0, C) or -100 is the caller's contract; any label outside [0, C) is treated as ignored and never used as an index.  With every label
// ignored n_valid is 0 and the loss is 0 / 0 = NaN, as F.cross_entropy gives.  NaN logits are outside x2_cls_accuracy's contract.
#include "x2_rowblock.h"

#define CL_THREADS ROW_THREADS
#define CL_COLS 64               // backward launch two: columns per workgroup, and rows per staged chunk of dlogits
#define CL_MAXR 65536
#define CL_MAXH 16384
#define CL_MAXC 16

#define CL_ALIGNED(p) ((((uintptr_t)(p)) & 15) == 0)          // rows are read and written as float4

// dlogits of one row: g_logits (or 0) + scale * (softmax(logits) - onehot(label)) on a valid row; scale = g_loss / n_valid (0 without g_loss)
template <int CM>
__device__ __forceinline__ void cl_dlogits(const float* __restrict__ lrow, const float* __restrict__ grow, bool has_label, long label, float scale,
                                           int C, float dl[CM]) {
  float l[CM], m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    l[c] = c < C ? lrow[c] : -INFINITY;
    dl[c] = (grow && c < C) ? grow[c] : 0.f;
    m = fmaxf(m, l[c]);
  }
  if (!has_label || label < 0 || label >= C) return;
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    l[c] = c < C ? expf(l[c] - m) : 0.f;
    sum += l[c];
  }
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) dl[c] += scale * (l[c] / sum - (c == (int)label ? 1.f : 0.f));
}

// ---- forward, launch one: a workgroup per row
template <int CM>
__global__ __launch_bounds__(CL_THREADS) void cls_tail_fwd_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, const long* __restrict__ labels, int H, int C,
                                                                  float eps, float* __restrict__ logits, float* __restrict__ rowstat,
                                                                  float* __restrict__ nll) {
  __shared__ float red[CL_THREADS / 64];
  __shared__ float part[CL_THREADS / 64][CM];
  __shared__ float lg[CM];
  const int r = blockIdx.x, n4 = H >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(h + (size_t)r * ldh);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  const float4* w4 = reinterpret_cast<const float4*>(w);
  float mean, rstd;
  row_ln_stats(x4, n4, H, eps, red, mean, rstd);
  float acc[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) acc[c] = 0.f;
  for (int i = threadIdx.x; i < n4; i += CL_THREADS) {
    const float4 v = x4[i], g = g4[i], b = b4[i];
    float4 a;
    a.x = gelu_erf((v.x - mean) * rstd * g.x + b.x); a.y = gelu_erf((v.y - mean) * rstd * g.y + b.y);
    a.z = gelu_erf((v.z - mean) * rstd * g.z + b.z); a.w = gelu_erf((v.w - mean) * rstd * g.w + b.w);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) acc[c] += dot4(a, w4[(size_t)c * n4 + i]);
  }
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {                                      // C is uniform: whole waves take the butterfly
      const float v = wave_sum(acc[c]);
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = v;
    }
  __syncthreads();
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    const float v = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + bias[c];
    lg[c] = v;
    logits[(size_t)r * C + c] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rowstat[2 * r] = mean;
    rowstat[2 * r + 1] = rstd;
    if (labels) {
      const long lab = labels[r];
      float out = 0.f;
      if (lab >= 0 && lab < C) {
        float m = lg[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, lg[c]);
        float sum = 0.f;
        for (int c = 0; c < C; ++c) sum += expf(lg[c] - m);
        out = (m + logf(sum)) - lg[lab];
      }
      nll[r] = out;
    }
  }
}

// ---- forward, launch two: stat = {sum nll / n_valid, n_valid}; one workgroup, thread t adds rows t, t + 256, ... in index order
__global__ __launch_bounds__(CL_THREADS) void cls_loss_mean_kernel(const float* __restrict__ nll, const long* __restrict__ labels, int R, int C,
                                                                   float* __restrict__ stat) {
  __shared__ float red[CL_THREADS / 64];
  float s = 0.f, n = 0.f;
  for (int r = threadIdx.x; r < R; r += CL_THREADS) {
    const long lab = labels[r];
    if (lab >= 0 && lab < C) { s += nll[r]; n += 1.f; }
  }
  s = row_block_sum(s, red);
  n = row_block_sum(n, red);                          // at most 65536: exact in fp32
  if (threadIdx.x == 0) {
    stat[0] = s / n;
    stat[1] = n;
  }
}

template <int CM>
static void cl_launch_fwd(const float* h, int ldh, const float* gamma, const float* beta, const float* w, const float* bias, const long* labels, int R,
                          int H, int C, float eps, float* logits, float* rowstat, float* nll, hipStream_t st) {
  hipLaunchKernelGGL(cls_tail_fwd_kernel<CM>, dim3(R), dim3(CL_THREADS), 0, st, h, ldh, gamma, beta, w, bias, labels, H, C, eps, logits, rowstat,
                     nll);
}

#define CL_REQUIRE_SHAPE(name)                                                                                                     \
  X2_REQUIRE(R >= 1 && R <= CL_MAXR, name ": R=%d must be in 1..%d", R, CL_MAXR);                                                   \
  X2_REQUIRE(H >= 4 && H <= CL_MAXH && H % 4 == 0, name ": H=%d must be a multiple of 4 in 4..%d", H, CL_MAXH);                      \
  X2_REQUIRE(C >= 2 && C <= CL_MAXC, name ": C=%d must be in 2..%d", C, CL_MAXC)

extern "C" int x2_cls_tail_fwd(const float* h, int ldh, const float* gamma, const float* beta, const float* w, const float* bias, const long* labels,
                               int R, int H, int C, float eps, float* logits, float* rowstat, float* nll, float* stat, void* stream) {
  X2_REQUIRE(h && gamma && beta && w && bias && logits && rowstat, "x2_cls_tail_fwd: null tensor");
  X2_REQUIRE(!labels || (nll && stat), "x2_cls_tail_fwd: labels need nll and stat");
  CL_REQUIRE_SHAPE("x2_cls_tail_fwd");
  X2_REQUIRE(ldh >= H && ldh % 4 == 0, "x2_cls_tail_fwd: ldh=%d must be a multiple of 4 and at least H=%d", ldh, H);
  X2_REQUIRE(CL_ALIGNED(h) && CL_ALIGNED(gamma) && CL_ALIGNED(beta) && CL_ALIGNED(w), "x2_cls_tail_fwd: h, gamma, beta and w must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (C <= 2) cl_launch_fwd<2>(h, ldh, gamma, beta, w, bias, labels, R, H, C, eps, logits, rowstat, nll, st);
  else if (C <= 4) cl_launch_fwd<4>(h, ldh, gamma, beta, w, bias, labels, R, H, C, eps, logits, rowstat, nll, st);
  else cl_launch_fwd<CL_MAXC>(h, ldh, gamma, beta, w, bias, labels, R, H, C, eps, logits, rowstat, nll, st);
  if (labels) hipLaunchKernelGGL(cls_loss_mean_kernel, dim3(1), dim3(CL_THREADS), 0, st, nll, labels, R, C, stat);
  return x2_check_launch("x2_cls_tail_fwd");
}

// ---- backward, launch one: a workgroup per row -> dh
template <int CM>
__global__ __launch_bounds__(CL_THREADS) void cls_tail_bwd_rows_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, const float* __restrict__ w,
                                                                       const float* __restrict__ rowstat, const float* __restrict__ logits,
                                                                       const long* __restrict__ labels, const float* __restrict__ stat,
                                                                       const float* __restrict__ g_loss, const float* __restrict__ g_logits, int H,
                                                                       int C, float* __restrict__ dh, int lddh) {
  __shared__ float red[CL_THREADS / 64];
  const int r = blockIdx.x, n4 = H >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(h + (size_t)r * ldh);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  const float4* w4 = reinterpret_cast<const float4*>(w);
  float4* d4 = reinterpret_cast<float4*>(dh + (size_t)r * lddh);
  const float mean = rowstat[2 * r], rstd = rowstat[2 * r + 1];
  const bool has_label = labels != nullptr && g_loss != nullptr;
  float dl[CM];                                       // every thread computes the row's C values itself: no exchange
  cl_dlogits<CM>(logits + (size_t)r * C, g_logits ? g_logits + (size_t)r * C : nullptr, has_label, has_label ? labels[r] : -100,
                 has_label ? g_loss[0] / stat[1] : 0.f, C, dl);
  // dxhat = (dlogits @ w) * gelu'(y) * gamma of four columns, and their xhat
  auto dxhat4 = [&](int i, float4& xh) -> float4 {
    const float4 v = x4[i], g = g4[i], b = b4[i];
    xh.x = (v.x - mean) * rstd; xh.y = (v.y - mean) * rstd; xh.z = (v.z - mean) * rstd; xh.w = (v.w - mean) * rstd;
    float4 da = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) {
        const float4 wv = w4[(size_t)c * n4 + i];
        da.x += dl[c] * wv.x; da.y += dl[c] * wv.y; da.z += dl[c] * wv.z; da.w += dl[c] * wv.w;
      }
    float4 d;
    d.x = da.x * dgelu(xh.x * g.x + b.x) * g.x; d.y = da.y * dgelu(xh.y * g.y + b.y) * g.y;
    d.z = da.z * dgelu(xh.z * g.z + b.z) * g.z; d.w = da.w * dgelu(xh.w * g.w + b.w) * g.w;
    return d;
  };
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < n4; i += CL_THREADS) {
    float4 xh;
    const float4 d = dxhat4(i, xh);
    s1 += sum4(d);
    s2 += dot4(d, xh);
  }
  s1 = row_block_sum(s1, red) / (float)H;
  s2 = row_block_sum(s2, red) / (float)H;
  for (int i = threadIdx.x; i < n4; i += CL_THREADS) {          // the same arithmetic again instead of an [H] row kept somewhere
    float4 xh;
    float4 d = dxhat4(i, xh);
    d.x = rstd * (d.x - s1 - xh.x * s2); d.y = rstd * (d.y - s1 - xh.y * s2);
    d.z = rstd * (d.z - s1 - xh.z * s2); d.w = rstd * (d.w - s1 - xh.w * s2);
    d4[i] = d;
  }
}

// ---- backward, launch two: one thread per column j walks rows 0..R-1 in order.  A workgroup owns CL_COLS columns and stages the dlogits, mean and
// rstd of CL_COLS rows at a time in LDS (thread t computes row r0 + t's), which every column then reads as broadcasts.  Workgroup 0 also sums dbias.
template <int CM>
__global__ __launch_bounds__(CL_COLS) void cls_tail_bwd_cols_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* __restrict__ w,
                                                                    const float* __restrict__ rowstat, const float* __restrict__ logits,
                                                                    const long* __restrict__ labels, const float* __restrict__ stat,
                                                                    const float* __restrict__ g_loss, const float* __restrict__ g_logits, int R, int H,
                                                                    int C, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                    float* __restrict__ dw, float* __restrict__ dbias) {
  __shared__ float sdl[CL_COLS][CM];
  __shared__ float smean[CL_COLS], srstd[CL_COLS];
  const int t = threadIdx.x, j = blockIdx.x * CL_COLS + t;
  const bool active = j < H;
  const bool has_label = labels != nullptr && g_loss != nullptr;
  const float scale = has_label ? g_loss[0] / stat[1] : 0.f;
  const float gam = active ? gamma[j] : 0.f, bet = active ? beta[j] : 0.f;
  float wj[CM], dwj[CM], dg = 0.f, db = 0.f, dbs = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    wj[c] = (active && c < C) ? w[(size_t)c * H + j] : 0.f;
    dwj[c] = 0.f;
  }
  for (int r0 = 0; r0 < R; r0 += CL_COLS) {
    __syncthreads();                                  // the previous chunk has been read by every column
    if (r0 + t < R) {
      const int r = r0 + t;
      float dl[CM];
      cl_dlogits<CM>(logits + (size_t)r * C, g_logits ? g_logits + (size_t)r * C : nullptr, has_label, has_label ? labels[r] : -100, scale, C, dl);
#pragma unroll
      for (int c = 0; c < CM; ++c) sdl[t][c] = dl[c];
      smean[t] = rowstat[2 * r];
      srstd[t] = rowstat[2 * r + 1];
    }
    __syncthreads();
    const int nr = min(CL_COLS, R - r0);
    if (active) {
      const float* col = h + (size_t)r0 * ldh + j;
#pragma unroll 4
      for (int k = 0; k < nr; ++k) {
        const float xh = (col[(size_t)k * ldh] - smean[k]) * srstd[k];
        const float y = xh * gam + bet;
        float da = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c) da += sdl[k][c] * wj[c];
        const float dy = da * dgelu(y), a = gelu_erf(y);
        dg += dy * xh;
        db += dy;
#pragma unroll
        for (int c = 0; c < CM; ++c) dwj[c] += sdl[k][c] * a;
      }
    }
    if (blockIdx.x == 0 && t < C)
      for (int k = 0; k < nr; ++k) dbs += sdl[k][t];
  }
  if (active) {
    dgamma[j] = dg;
    dbeta[j] = db;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) dw[(size_t)c * H + j] = dwj[c];
  }
  if (blockIdx.x == 0 && t < C) dbias[t] = dbs;
}

template <int CM>
static void cl_launch_bwd(const float* h, int ldh, const float* gamma, const float* beta, const float* w, const float* rowstat, const float* logits,
                          const long* labels, const float* stat, const float* g_loss, const float* g_logits, int R, int H, int C, float* dh, int lddh,
                          float* dgamma, float* dbeta, float* dw, float* dbias, hipStream_t st) {
  hipLaunchKernelGGL(cls_tail_bwd_rows_kernel<CM>, dim3(R), dim3(CL_THREADS), 0, st, h, ldh, gamma, beta, w, rowstat, logits, labels, stat, g_loss,
                     g_logits, H, C, dh, lddh);
  hipLaunchKernelGGL(cls_tail_bwd_cols_kernel<CM>, dim3((H + CL_COLS - 1) / CL_COLS), dim3(CL_COLS), 0, st, h, ldh, gamma, beta, w, rowstat, logits,
                     labels, stat, g_loss, g_logits, R, H, C, dgamma, dbeta, dw, dbias);
}

extern "C" int x2_cls_tail_bwd(const float* h, int ldh, const float* gamma, const float* beta, const float* w, const float* rowstat, const float* logits,
                               const long* labels, const float* stat, const float* g_loss, const float* g_logits, int R, int H, int C, float* dh,
                               int lddh, float* dgamma, float* dbeta, float* dw, float* dbias, void* stream) {
  X2_REQUIRE(h && gamma && beta && w && rowstat && logits && dh && dgamma && dbeta && dw && dbias, "x2_cls_tail_bwd: null tensor");
  X2_REQUIRE(!(labels && g_loss) || stat, "x2_cls_tail_bwd: labels with g_loss need the forward's stat");
  CL_REQUIRE_SHAPE("x2_cls_tail_bwd");
  X2_REQUIRE(ldh >= H && ldh % 4 == 0 && lddh >= H && lddh % 4 == 0, "x2_cls_tail_bwd: ldh=%d and lddh=%d must be multiples of 4 and at least H=%d", ldh,
             lddh, H);
  X2_REQUIRE(CL_ALIGNED(h) && CL_ALIGNED(gamma) && CL_ALIGNED(beta) && CL_ALIGNED(w) && CL_ALIGNED(dh),
             "x2_cls_tail_bwd: h, gamma, beta, w and dh must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (C <= 2) cl_launch_bwd<2>(h, ldh, gamma, beta, w, rowstat, logits, labels, stat, g_loss, g_logits, R, H, C, dh, lddh, dgamma, dbeta, dw, dbias, st);
  else if (C <= 4) cl_launch_bwd<4>(h, ldh, gamma, beta, w, rowstat, logits, labels, stat, g_loss, g_logits, R, H, C, dh, lddh, dgamma, dbeta, dw, dbias, st);
  else cl_launch_bwd<CL_MAXC>(h, ldh, gamma, beta, w, rowstat, logits, labels, stat, g_loss, g_logits, R, H, C, dh, lddh, dgamma, dbeta, dw, dbias, st);
  return x2_check_launch("x2_cls_tail_bwd");
}

// ---- evaluation: one workgroup; thread t takes rows t, t + 256, ...; the count is an integer sum, so its order does not matter
__global__ __launch_bounds__(CL_THREADS) void cls_accuracy_kernel(const float* __restrict__ logits, const long* __restrict__ labels, int R, int C,
                                                                  int* __restrict__ pred, long* __restrict__ counts) {
  __shared__ int red[CL_THREADS / 64];
  int hit = 0;
  for (int r = threadIdx.x; r < R; r += CL_THREADS) {
    const float* row = logits + (size_t)r * C;
    int best = 0;
    float m = row[0];
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > m) { m = v; best = c; }                 // strict: the lowest index of equal maxima stays
    }
    pred[r] = best;
    hit += labels[r] == (long)best ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = hit;
  __syncthreads();
  if (threadIdx.x == 0) {                             // launches on one stream are ordered: a plain read-modify-write accumulates
    counts[0] += (long)((red[0] + red[1]) + (red[2] + red[3]));
    counts[1] += (long)R;
  }
}

extern "C" int x2_cls_accuracy(const float* logits, const long* labels, int R, int C, int* pred, long* counts, void* stream) {
  X2_REQUIRE(logits && labels && pred && counts, "x2_cls_accuracy: null tensor");
  X2_REQUIRE(R >= 1 && R <= CL_MAXR, "x2_cls_accuracy: R=%d must be in 1..%d", R, CL_MAXR);
  X2_REQUIRE(C >= 2 && C <= CL_MAXC, "x2_cls_accuracy: C=%d must be in 2..%d", C, CL_MAXC);
  hipLaunchKernelGGL(cls_accuracy_kernel, dim3(1), dim3(CL_THREADS), 0, (hipStream_t)stream, logits, labels, R, C, pred, counts);
  return x2_check_launch("x2_cls_accuracy");
}
