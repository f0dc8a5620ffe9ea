// Image-text retrieval fine-tune and evaluation (XVLMForRetrieval; models/model_retrieval.py, Retrieval.py): the soft-label contrastive loss of
// XVLMBase.get_contrastive_loss(idx=...) (xvlm.py:805-826), the hard-negative draw with a per-row "no negative" flag, and the recall counts of
// itm_eval (Retrieval.py:171-215).
//   x2_itc_soft_fwd             z = logits [N, ld] fp32 (already divided by temp), idx int64 [N] the group ids, pos_ij = (idx[i] == idx[j]).
//                               row i:    cnt_i = sum_j pos_ij, lse_i = max_j z_ij + log sum_j exp(z_ij - max), li_i = lse_i - (sum_j pos_ij z_ij) / cnt_i
//                               column j: the same over z_.j -> lt_j
//                               out[0] = (sum_i li_i / N + sum_j lt_j / N) / 2;  loss_rows [2N] = {li, lt};  rowstat / colstat [N][3] =
//                               {max, log sum exp(z - max), cnt}: lse in its two parts.  At temp = 0.001 the logits reach +-1000 and one fp32
//                               lse is 6e-5 coarse, which the backward's exp(z - lse) would turn into a relative error of 3e-5; (z - max)
//                               is exact where it matters and the log-sum is small
//   x2_itc_soft_bwd             dz_ij = g / (2N) * ((exp(z_ij - lse_i) - pos_ij / cnt_i) + (exp(z_ij - lse^col_j) - pos_ij / cnt_j)), g a device scalar
//   x2_sample_negatives_checked x2_sample_negatives (x2_negatives.h: the same device function, the same bits) plus no_negative [n]
//   x2_retrieval_ranks          per query row of scores [R, ld]: the best rank of its ground-truth columns, then counts += {R@1, R@5, R@10, R}
// Launches: the forward two (statistics, then the mean), the backward one, the sampler one, the ranks two.
// The statistics launch has N workgroups for the rows and ceil(N / 64) for the columns.  A column workgroup owns 64 adjacent columns and reads the
// matrix ROW-MAJOR: wave w takes rows w, w + 4, ..., lane l column c0 + l, so every load of a wave is 256 contiguous bytes; no transpose exists
// anywhere and no lane walks a column with stride ld on its own.  The four waves' partials of a column meet in LDS.
// Plain fp32 VALU arithmetic, libm expf / logf, no atomics, one writer per output element.  Fixed summation orders, so two runs give the same bits:
//   a row          thread t adds columns t, t + 256, ... in index order; then x2_rowblock.h's block sum (xor butterfly, (w0 + w1) + (w2 + w3))
//   a column       wave w adds rows w, w + 4, ... in index order; the four waves' partials as (p0 + p1) + (p2 + p3); maxima likewise
//   the mean       thread t adds entries t, t + 256, ... of li, then of lt, in index order; then the block sum
// The losses are formed relative to the maximum as well: li_i = log-sum - (sum_j pos_ij (z_ij - max)) / cnt_i, which is lse_i - mean of the positives
// without the cancellation of two numbers near 1000.  Counts are integers kept as floats (N <= 1024: exact).  Pad columns [N, ld) of logits and
// dlogits are never read and never written.
// Tie rule of the ranks: rank = the number of columns c < N with s[c] STRICTLY greater than the ground truth's score.  np.argsort(...)[::-1] has
// no defined order among equal scores, so this is the reference's rank whenever the ground truth's score is not tied; with the -100 fill of
// rerank_scores a ground truth outside the top k_test gets rank k_test here and some rank >= k_test there: R@1 / R@5 / R@10 agree for
// k_test >= 10.  A ground-truth id outside [0, N) is skipped and never dereferenced; a row without a ground truth gets INT_MAX (the reference's
// 1e20): it counts in no recall and does count in the denominator.  NaN scores are outside the contract.
#include "x2_negatives.h"
#include "x2_rowblock.h"
#include <limits.h>

#define RT_THREADS ROW_THREADS
#define RT_COLS 64               // columns of a column workgroup: one per lane
#define RT_MAXN 1024             // x2_sample_negatives' bound: the all-gathered batch
#define RT_GT 8                  // ground truths of a row counted per pass over the row
#define RT_MAXCOLS 65536
static_assert(RT_COLS == 64 && RT_THREADS == 4 * RT_COLS, "a column workgroup is four waves over the same 64 columns");

#define RT_ALIGNED(p, n) ((((uintptr_t)(p)) & ((n) - 1)) == 0)

__device__ __forceinline__ int rt_block_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- soft-label ITC, forward
// launch one: workgroups [0, N) own a row each, workgroups [N, N + ceil(N / 64)) 64 columns each
__global__ __launch_bounds__(RT_THREADS) void itc_soft_stats_kernel(const float* __restrict__ logits, int ld, const long* __restrict__ idx, int N,
                                                                    float* __restrict__ rowstat, float* __restrict__ colstat,
                                                                    float* __restrict__ loss_rows) {
  __shared__ float red[ROW_WAVES];
  __shared__ float part[3][ROW_WAVES][RT_COLS];
  if ((int)blockIdx.x < N) {
    const int i = blockIdx.x;
    const float* row = logits + (size_t)i * ld;
    const long gi = idx[i];
    float m = -INFINITY;
    for (int c = threadIdx.x; c < N; c += RT_THREADS) m = fmaxf(m, row[c]);
    m = row_block_max(m, red);
    float s = 0.f, ps = 0.f, n = 0.f;
    for (int c = threadIdx.x; c < N; c += RT_THREADS) {
      const float z = row[c];
      s += expf(z - m);
      if (idx[c] == gi) { ps += z - m; n += 1.f; }
    }
    s = row_block_sum(s, red);
    ps = row_block_sum(ps, red);
    n = row_block_sum(n, red);
    if (threadIdx.x == 0) {
      const float ls = logf(s);
      rowstat[3 * i] = m;
      rowstat[3 * i + 1] = ls;
      rowstat[3 * i + 2] = n;
      loss_rows[i] = ls - ps / n;
    }
    return;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int j = ((int)blockIdx.x - N) * RT_COLS + l;
  const bool active = j < N;
  const long gj = active ? idx[j] : 0;
  float m = -INFINITY;
  if (active)
    for (int r = w; r < N; r += ROW_WAVES) m = fmaxf(m, logits[(size_t)r * ld + j]);
  part[0][w][l] = m;
  __syncthreads();
  m = fmaxf(fmaxf(part[0][0][l], part[0][1][l]), fmaxf(part[0][2][l], part[0][3][l]));
  __syncthreads();
  float s = 0.f, ps = 0.f, n = 0.f;
  if (active)
    for (int r = w; r < N; r += ROW_WAVES) {
      const float z = logits[(size_t)r * ld + j];
      s += expf(z - m);
      if (idx[r] == gj) { ps += z - m; n += 1.f; }
    }
  part[0][w][l] = s;
  part[1][w][l] = ps;
  part[2][w][l] = n;
  __syncthreads();
  if (w == 0 && active) {
    s = (part[0][0][l] + part[0][1][l]) + (part[0][2][l] + part[0][3][l]);
    ps = (part[1][0][l] + part[1][1][l]) + (part[1][2][l] + part[1][3][l]);
    n = (part[2][0][l] + part[2][1][l]) + (part[2][2][l] + part[2][3][l]);
    const float ls = logf(s);
    colstat[3 * j] = m;
    colstat[3 * j + 1] = ls;
    colstat[3 * j + 2] = n;
    loss_rows[N + j] = ls - ps / n;
  }
}

// launch two: one workgroup.  out[0] = (mean li + mean lt) / 2
__global__ __launch_bounds__(RT_THREADS) void itc_soft_mean_kernel(const float* __restrict__ loss_rows, int N, float* __restrict__ out) {
  __shared__ float red[ROW_WAVES];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < N; i += RT_THREADS) a += loss_rows[i];
  for (int i = threadIdx.x; i < N; i += RT_THREADS) b += loss_rows[N + i];
  a = row_block_sum(a, red);
  b = row_block_sum(b, red);
  if (threadIdx.x == 0) out[0] = (a / (float)N + b / (float)N) * 0.5f;
}

#define RT_REQUIRE_N(name, ldname, ldv)                                                                       \
  X2_REQUIRE(N >= 2 && N <= RT_MAXN, name ": N=%d must be in 2..%d", N, RT_MAXN);                              \
  X2_REQUIRE((ldv) >= N, name ": " ldname "=%d must be at least N=%d", (ldv), N)

extern "C" int x2_itc_soft_fwd(const float* logits, int ld, const long* idx, int N, float* rowstat, float* colstat, float* loss_rows, float* out,
                               void* stream) {
  X2_REQUIRE(logits && idx && rowstat && colstat && loss_rows && out, "x2_itc_soft_fwd: null tensor");
  RT_REQUIRE_N("x2_itc_soft_fwd", "ld", ld);
  X2_REQUIRE(RT_ALIGNED(logits, 4) && RT_ALIGNED(idx, 8) && RT_ALIGNED(rowstat, 4) && RT_ALIGNED(colstat, 4) && RT_ALIGNED(loss_rows, 4) &&
             RT_ALIGNED(out, 4), "x2_itc_soft_fwd: tensors must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(itc_soft_stats_kernel, dim3(N + (N + RT_COLS - 1) / RT_COLS), dim3(RT_THREADS), 0, st, logits, ld, idx, N, rowstat, colstat,
                     loss_rows);
  hipLaunchKernelGGL(itc_soft_mean_kernel, dim3(1), dim3(RT_THREADS), 0, st, loss_rows, N, out);
  return x2_check_launch("x2_itc_soft_fwd");
}

// ---------------------------------------------------------------------------------------------------------------- soft-label ITC, backward
// one launch, a workgroup per row; thread t owns columns t, t + 256, ...
__global__ __launch_bounds__(RT_THREADS) void itc_soft_bwd_kernel(const float* __restrict__ logits, int ld, const long* __restrict__ idx, int N,
                                                                  const float* __restrict__ rowstat, const float* __restrict__ colstat,
                                                                  const float* __restrict__ g, float* __restrict__ dlogits, int ldd) {
  const int i = blockIdx.x;
  const float* row = logits + (size_t)i * ld;
  float* drow = dlogits + (size_t)i * ldd;
  const long gi = idx[i];
  const float m = rowstat[3 * i], ls = rowstat[3 * i + 1], inv_i = 1.f / rowstat[3 * i + 2];
  const float scale = g[0] / (float)(2 * N);
  for (int c = threadIdx.x; c < N; c += RT_THREADS) {
    const float z = row[c];
    const bool pos = idx[c] == gi;
    const float a = expf((z - m) - ls) - (pos ? inv_i : 0.f);
    const float b = expf((z - colstat[3 * c]) - colstat[3 * c + 1]) - (pos ? 1.f / colstat[3 * c + 2] : 0.f);
    drow[c] = scale * (a + b);
  }
}

extern "C" int x2_itc_soft_bwd(const float* logits, int ld, const long* idx, int N, const float* rowstat, const float* colstat, const float* g,
                               float* dlogits, int ldd, void* stream) {
  X2_REQUIRE(logits && idx && rowstat && colstat && g && dlogits, "x2_itc_soft_bwd: null tensor");
  RT_REQUIRE_N("x2_itc_soft_bwd", "ld", ld);
  X2_REQUIRE(ldd >= N, "x2_itc_soft_bwd: ldd=%d must be at least N=%d", ldd, N);
  X2_REQUIRE(RT_ALIGNED(logits, 4) && RT_ALIGNED(idx, 8) && RT_ALIGNED(rowstat, 4) && RT_ALIGNED(colstat, 4) && RT_ALIGNED(g, 4) &&
             RT_ALIGNED(dlogits, 4), "x2_itc_soft_bwd: tensors must be aligned to their element size");
  hipLaunchKernelGGL(itc_soft_bwd_kernel, dim3(N), dim3(RT_THREADS), 0, (hipStream_t)stream, logits, ld, idx, N, rowstat, colstat, g, dlogits, ldd);
  return x2_check_launch("x2_itc_soft_bwd");
}

// ---------------------------------------------------------------------------------------------------------------- hard negatives with a flag
__global__ __launch_bounds__(256) void sample_negatives_checked_kernel(const float* __restrict__ sim, int n, const long* __restrict__ group,
                                                                       const float* __restrict__ u, int* out, int* no_negative) {
  sample_negatives_row(sim, n, group, u, out, no_negative);
}

extern "C" int x2_sample_negatives_checked(const float* sim, int n, const long* group, const float* u, int* out, int* no_negative, void* stream) {
  X2_REQUIRE(sim && u && out && no_negative, "x2_sample_negatives_checked: null tensor");
  X2_REQUIRE(n > 1 && n <= RT_MAXN, "x2_sample_negatives_checked: n=%d not in (1,%d]", n, RT_MAXN);
  hipLaunchKernelGGL(sample_negatives_checked_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, sim, n, group, u, out, no_negative);
  return x2_check_launch("x2_sample_negatives_checked");
}

// ---------------------------------------------------------------------------------------------------------------- recall counts
// launch one: a workgroup per query row; RT_GT ground truths share one pass over the row
__global__ __launch_bounds__(RT_THREADS) void retrieval_ranks_kernel(const float* __restrict__ scores, int ld, int N, const int* __restrict__ gt_offs,
                                                                     const int* __restrict__ gt_ids, int* __restrict__ ranks) {
  __shared__ int red[ROW_WAVES];
  const int r = blockIdx.x;
  const float* row = scores + (size_t)r * ld;
  const int e0 = gt_offs[r], e1 = gt_offs[r + 1];
  int best = INT_MAX;
  for (int e = e0; e < e1; e += RT_GT) {                // e0, e1 and every id are the same in all threads: uniform control flow
    float sj[RT_GT];
    int above[RT_GT];
    bool ok[RT_GT];
#pragma unroll
    for (int k = 0; k < RT_GT; ++k) {
      const int id = e + k < e1 ? gt_ids[e + k] : -1;
      ok[k] = id >= 0 && id < N;
      sj[k] = ok[k] ? row[id] : INFINITY;               // nothing is greater: a skipped slot counts nothing
      above[k] = 0;
    }
    for (int c = threadIdx.x; c < N; c += RT_THREADS) {
      const float v = row[c];
#pragma unroll
      for (int k = 0; k < RT_GT; ++k) above[k] += v > sj[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < RT_GT; ++k)
      if (ok[k]) best = min(best, rt_block_sum_int(above[k], red));
  }
  if (threadIdx.x == 0) ranks[r] = best;
}

// launch two: one workgroup; integer sums.  Launches on one stream are ordered: a plain read-modify-write accumulates.
__global__ __launch_bounds__(RT_THREADS) void retrieval_counts_kernel(const int* __restrict__ ranks, int R, long* __restrict__ counts) {
  __shared__ int red[ROW_WAVES];
  int n1 = 0, n5 = 0, n10 = 0;
  for (int r = threadIdx.x; r < R; r += RT_THREADS) {
    const int k = ranks[r];
    n1 += k < 1 ? 1 : 0;
    n5 += k < 5 ? 1 : 0;
    n10 += k < 10 ? 1 : 0;
  }
  n1 = rt_block_sum_int(n1, red);
  n5 = rt_block_sum_int(n5, red);
  n10 = rt_block_sum_int(n10, red);
  if (threadIdx.x == 0) {
    counts[0] += (long)n1;
    counts[1] += (long)n5;
    counts[2] += (long)n10;
    counts[3] += (long)R;
  }
}

extern "C" int x2_retrieval_ranks(const float* scores, int ld, int R, int N, const int* gt_offs, const int* gt_ids, int* ranks, long* counts,
                                  void* stream) {
  X2_REQUIRE(scores && gt_offs && ranks && counts, "x2_retrieval_ranks: null tensor (gt_ids may be null only when no row has a ground truth)");
  X2_REQUIRE(R >= 1, "x2_retrieval_ranks: R=%d must be at least 1", R);
  X2_REQUIRE(N >= 1 && N <= RT_MAXCOLS, "x2_retrieval_ranks: N=%d must be in 1..%d", N, RT_MAXCOLS);
  X2_REQUIRE(ld >= N, "x2_retrieval_ranks: ld=%d must be at least N=%d", ld, N);
  X2_REQUIRE(RT_ALIGNED(scores, 4) && RT_ALIGNED(gt_offs, 4) && RT_ALIGNED(gt_ids, 4) && RT_ALIGNED(ranks, 4) && RT_ALIGNED(counts, 8),
             "x2_retrieval_ranks: tensors must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(retrieval_ranks_kernel, dim3(R), dim3(RT_THREADS), 0, st, scores, ld, N, gt_offs, gt_ids, ranks);
  hipLaunchKernelGGL(retrieval_counts_kernel, dim3(1), dim3(RT_THREADS), 0, st, ranks, R, counts);
  return x2_check_launch("x2_retrieval_ranks");
}
