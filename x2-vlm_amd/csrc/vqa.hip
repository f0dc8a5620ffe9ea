// VQA inference (XVLMForVQA.rank_answer, models/model_generation.py:562-619): the three kernels around the two decoder passes, and the
// two row kernels of the training step (forward(train=True), model_generation.py:517-550) at the end of the file.
//   x2_answer_topk     log-softmax of the first-step logits, gathered at every candidate answer's first token, k best candidates
//   x2_vqa_candidates  ids, next-token labels, K/V row map and the additive causal x padding mask of the B * k candidate rows
//   x2_vqa_rerank      score = first-token log-probability - sum of the per-token losses, softmax over a question's k scores, sorted
// Order rule of both selections: larger value first, the lower index (candidate / slot) first among equal values - a total order, so
// the result does not depend on how the work is split.  No atomics: every output element has one writer.  The work is tiny (k <= 256
// per question); what these kernels save is launches, the per-question host loop and the [B * k, La, La] 0/1 mask, so they are plain
// VALU code with one workgroup per question (candidates: per row).
#include "x2_rowblock.h"

#define VQ_THREADS ROW_THREADS
#define VQ_MAXK 256
#define VQ_MAXNA 65536
#define VQ_MAXLA 128
#define VQ_CACHE 8192          // candidates whose log-probability is kept in LDS between the selection rounds (the rest are recomputed)
static_assert(VQ_MAXK <= VQ_THREADS, "one thread per selected slot");

__device__ __forceinline__ bool vq_better(float av, int ac, float bv, int bc) { return av > bv || (av == bv && ac < bc); }

// ---------------------------------------------------------------------------------------------------------------- first stage
// One workgroup per question row.  logp[c] = (z[first_tok[c]] - max) - log(sum exp(z - max)) over the V valid columns (x2_logprob_topk's
// arithmetic); a first token outside [0, V) - excluded by the caller - is never dereferenced and scores -inf.  Round r picks the best
// candidate that comes strictly after round r - 1's winner in the order (value descending, index ascending).
__global__ __launch_bounds__(VQ_THREADS) void answer_topk_kernel(const float* __restrict__ logits, int ldv, int V, const int* __restrict__ first_tok,
                                                                 int Na, int K, float* __restrict__ out_vals, int* __restrict__ out_ids) {
  __shared__ float sLp[VQ_CACHE];
  __shared__ float sRedF[VQ_THREADS / 64];
  __shared__ int sRedC[VQ_THREADS / 64];
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* x = logits + (size_t)row * ldv;
  float m = -INFINITY;
  for (int c = tid; c < V; c += VQ_THREADS) m = fmaxf(m, x[c]);
  m = row_block_max(m, sRedF);
  float sum = 0.f;
  for (int c = tid; c < V; c += VQ_THREADS) sum += expf(x[c] - m);
  const float lsum = logf(row_block_sum(sum, sRedF));
  auto logp = [&](int c) -> float {
    const int t = first_tok[c];
    return (unsigned)t < (unsigned)V ? (x[t] - m) - lsum : -INFINITY;
  };
  for (int c = tid; c < Na && c < VQ_CACHE; c += VQ_THREADS) sLp[c] = logp(c);
  __syncthreads();
  float pv = INFINITY;
  int pc = -1;                                                            // the previous winner: everything is after (+inf, -1)
  for (int r = 0; r < K; ++r) {
    float bv = -INFINITY;
    int bc = 0x7fffffff;
    for (int c = tid; c < Na; c += VQ_THREADS) {                          // ascending c: an equal later value never displaces an earlier one
      const float v = c < VQ_CACHE ? sLp[c] : logp(c);
      if (vq_better(pv, pc, v, c) && vq_better(v, c, bv, bc)) { bv = v; bc = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (vq_better(ov, oc, bv, bc)) { bv = ov; bc = oc; }
    }
    if (lane == 0) { sRedF[wave] = bv; sRedC[wave] = bc; }
    __syncthreads();
    bv = sRedF[0]; bc = sRedC[0];
#pragma unroll
    for (int w = 1; w < VQ_THREADS / 64; ++w)
      if (vq_better(sRedF[w], sRedC[w], bv, bc)) { bv = sRedF[w]; bc = sRedC[w]; }
    __syncthreads();
    if (tid == 0) { out_vals[(size_t)row * K + r] = bv; out_ids[(size_t)row * K + r] = bc; }
    pv = bv; pc = bc;
  }
}

extern "C" int x2_answer_topk(const float* logits, int ldv, int V, int B, const int* first_tok, int Na, int K, float* out_vals, int* out_ids,
                              void* stream) {
  X2_REQUIRE(logits && first_tok && out_vals && out_ids, "x2_answer_topk: null tensor");
  X2_REQUIRE(B > 0 && V > 0 && ldv >= V, "x2_answer_topk: B=%d V=%d ldv=%d", B, V, ldv);
  X2_REQUIRE(Na >= 1 && Na <= VQ_MAXNA, "x2_answer_topk: Na=%d must be in 1..%d", Na, VQ_MAXNA);
  X2_REQUIRE(K >= 1 && K <= VQ_MAXK && K <= Na, "x2_answer_topk: k=%d must be in 1..min(Na=%d, %d)", K, Na, VQ_MAXK);
  hipLaunchKernelGGL(answer_topk_kernel, dim3(B), dim3(VQ_THREADS), 0, (hipStream_t)stream, logits, ldv, V, first_tok, Na, K, out_vals, out_ids);
  return x2_check_launch("x2_answer_topk");
}

// ---------------------------------------------------------------------------------------------------------------- candidate rows
// One workgroup per candidate row s = b * k + j, a = ids[s] its answer.  An id outside [0, Na) (the first stage never returns one for
// finite logits) reads no answer: the row becomes all padding (labels -100, every key masked).
__global__ __launch_bounds__(VQ_THREADS) void vqa_candidates_kernel(const long* __restrict__ answer_ids, const long* __restrict__ answer_atts,
                                                                    const int* __restrict__ ids, int Na, int La, int Lp, int K, long pad_id,
                                                                    long* __restrict__ input_ids, long* __restrict__ labels,
                                                                    int* __restrict__ kv_idx, float* __restrict__ mask2d) {
  __shared__ float sAtt[VQ_MAXLA];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int a = ids[s];
  const bool ok = (unsigned)a < (unsigned)Na;
  const long* src = answer_ids + (size_t)(ok ? a : 0) * La;
  const long* att = answer_atts + (size_t)(ok ? a : 0) * La;
  for (int t = tid; t < La; t += VQ_THREADS) {
    input_ids[(size_t)s * La + t] = ok ? src[t] : pad_id;
    sAtt[t] = ok ? (float)att[t] : 0.f;
    if (t + 1 < La) {
      const long nxt = ok ? src[t + 1] : pad_id;
      labels[(size_t)s * (La - 1) + t] = nxt == pad_id ? -100L : nxt;
    }
  }
  if (tid == 0) kv_idx[s] = s / K;
  __syncthreads();
  float* out = mask2d + (size_t)s * La * Lp;
  for (int e = tid; e < La * Lp; e += VQ_THREADS) {
    const int i = e / Lp, j = e - i * Lp;
    out[e] = j < La ? (1.0f - (j <= i ? sAtt[j] : 0.f)) * -10000.0f : 0.f;
  }
}

extern "C" int x2_vqa_candidates(const long* answer_ids, const long* answer_atts, const int* ids, int Na, int La, int B, int K, long pad_token_id,
                                 long* input_ids, long* labels, int* kv_idx, float* mask2d, int mask2d_ld, void* stream) {
  X2_REQUIRE(answer_ids && answer_atts && ids && input_ids && labels && kv_idx && mask2d, "x2_vqa_candidates: null tensor");
  X2_REQUIRE(Na >= 1 && B >= 1 && K >= 1 && (long)B * K < (1L << 31), "x2_vqa_candidates: Na=%d B=%d k=%d", Na, B, K);
  X2_REQUIRE(La >= 2 && La <= VQ_MAXLA, "x2_vqa_candidates: La=%d must be in 2..%d (the 2-D masked attention's limit)", La, VQ_MAXLA);
  X2_REQUIRE(mask2d_ld >= La && mask2d_ld % 64 == 0 && mask2d_ld <= VQ_MAXLA, "x2_vqa_candidates: mask2d_ld=%d must be La=%d rounded up to 64",
             mask2d_ld, La);
  hipLaunchKernelGGL(vqa_candidates_kernel, dim3(B * K), dim3(VQ_THREADS), 0, (hipStream_t)stream, answer_ids, answer_atts, ids, Na, La, mask2d_ld,
                     K, pad_token_id, input_ids, labels, kv_idx, mask2d);
  return x2_check_launch("x2_vqa_candidates");
}

// ---------------------------------------------------------------------------------------------------------------- second stage
// One workgroup per question, thread j = slot j.  The T = La - 1 losses of a row are added in index order in fp32, then subtracted from
// the first-token log-probability.  The sort is by score (the probabilities are a monotone map of the scores, so they come out
// non-increasing), lowest slot first among equal scores: slot j's rank is the number of slots that come before it.
__global__ __launch_bounds__(VQ_THREADS) void vqa_rerank_kernel(const float* __restrict__ loss, int T, const float* __restrict__ vals,
                                                                const int* __restrict__ ids, int K, float* __restrict__ topk_probs,
                                                                int* __restrict__ topk_ids, float* __restrict__ scores) {
  __shared__ float sScore[VQ_MAXK];
  __shared__ float sRed[VQ_THREADS / 64];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool live = j < K;
  float sc = -INFINITY;
  if (live) {
    const float* lr = loss + ((size_t)b * K + j) * T;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += lr[t];
    sc = vals[(size_t)b * K + j] - acc;
    scores[(size_t)b * K + j] = sc;
    sScore[j] = sc;
  }
  const float mx = row_block_max(sc, sRed);                                // the barrier inside also publishes sScore
  const float e = live ? expf(sc - mx) : 0.f;
  const float den = row_block_sum(e, sRed);
  if (live) {
    int rank = 0;
    for (int i = 0; i < K; ++i) rank += vq_better(sScore[i], i, sc, j) ? 1 : 0;
    topk_probs[(size_t)b * K + rank] = e / den;
    topk_ids[(size_t)b * K + rank] = ids[(size_t)b * K + j];
  }
}

extern "C" int x2_vqa_rerank(const float* loss_rows, int T, const float* vals, const int* ids, int B, int K, float* topk_probs, int* topk_ids,
                             float* scores, void* stream) {
  X2_REQUIRE(loss_rows && vals && ids && topk_probs && topk_ids && scores, "x2_vqa_rerank: null tensor");
  X2_REQUIRE(B >= 1 && K >= 1 && K <= VQ_MAXK, "x2_vqa_rerank: B=%d k=%d (k at most %d)", B, K, VQ_MAXK);
  X2_REQUIRE(T >= 1 && T <= VQ_MAXLA - 1, "x2_vqa_rerank: La - 1 = %d must be in 1..%d", T, VQ_MAXLA - 1);
  hipLaunchKernelGGL(vqa_rerank_kernel, dim3(B), dim3(VQ_THREADS), 0, (hipStream_t)stream, loss_rows, T, vals, ids, K, topk_probs, topk_ids, scores);
  return x2_check_launch("x2_vqa_rerank");
}

// ---------------------------------------------------------------------------------------------------------------- training rows
// XVLMForVQA.forward(train=True): the S answer rows of a batch, rows offs[b] .. offs[b + 1] - 1 belonging to question b (offs = the exclusive
// prefix sum of k, on the device: nothing about k is known to the host).  One workgroup per row s.  Rows s >= offs[B] are padding (S is a
// captured shape, sum(k) is not): labels all -100, c = 0, and kv_idx = B - 1, the LAST question - the count below saturates there, and every
// question keeps at least its own rows.  The mask rule is x2_vqa_candidates': (1 - tril[i][j] * atts[s][j]) * -10000, pad columns 0.
__global__ __launch_bounds__(VQ_THREADS) void vqa_train_rows_kernel(const int* __restrict__ offs, const long* __restrict__ answer_ids,
                                                                    const long* __restrict__ answer_atts, const float* __restrict__ weights,
                                                                    int B, int La, int Lp, long pad_id, int* __restrict__ kv_idx,
                                                                    long* __restrict__ labels, float* __restrict__ mask2d, float* __restrict__ c) {
  __shared__ float sAtt[VQ_MAXLA];
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool real = s < offs[B];
  const long* src = answer_ids + (size_t)s * La;
  for (int t = tid; t < La; t += VQ_THREADS) {
    sAtt[t] = (float)answer_atts[(size_t)s * La + t];
    if (t + 1 < La) {
      const long nxt = src[t + 1];
      labels[(size_t)s * (La - 1) + t] = (!real || nxt == pad_id) ? -100L : nxt;
    }
  }
  if (tid == 0) {
    int q = 0;                                                             // questions whose range ends at or before s
    for (int b = 1; b <= B; ++b) q += offs[b] <= s ? 1 : 0;
    kv_idx[s] = min(q, B - 1);
    c[s] = real ? weights[s] / (float)B : 0.f;
  }
  __syncthreads();
  float* out = mask2d + (size_t)s * La * Lp;
  for (int e = tid; e < La * Lp; e += VQ_THREADS) {
    const int i = e / Lp, j = e - i * Lp;
    out[e] = j < La ? (1.0f - (j <= i ? sAtt[j] : 0.f)) * -10000.0f : 0.f;
  }
}

extern "C" int x2_vqa_train_rows(const int* offs, const long* answer_ids, const long* answer_atts, const float* weights, int B, int S, int La,
                                 long pad_token_id, int* kv_idx, long* labels, float* mask2d, int mask2d_ld, float* c, void* stream) {
  X2_REQUIRE(offs && answer_ids && answer_atts && weights && kv_idx && labels && mask2d && c, "x2_vqa_train_rows: null tensor");
  X2_REQUIRE(B >= 1 && S >= 1, "x2_vqa_train_rows: B=%d S=%d", B, S);
  X2_REQUIRE(La >= 2 && La <= VQ_MAXLA, "x2_vqa_train_rows: La=%d must be in 2..%d (the 2-D masked attention's limit)", La, VQ_MAXLA);
  X2_REQUIRE(mask2d_ld >= La && mask2d_ld % 64 == 0 && mask2d_ld <= VQ_MAXLA, "x2_vqa_train_rows: mask2d_ld=%d must be La=%d rounded up to 64",
             mask2d_ld, La);
  hipLaunchKernelGGL(vqa_train_rows_kernel, dim3(S), dim3(VQ_THREADS), 0, (hipStream_t)stream, offs, answer_ids, answer_atts, weights, B, La,
                     mask2d_ld, pad_token_id, kv_idx, labels, mask2d, c);
  return x2_check_launch("x2_vqa_train_rows");
}

// ---------------------------------------------------------------------------------------------------------------- per-sequence loss
// Second stage of x2_mlm_ce_fwd for the answer decoder: rows r = s * T + t, T = La - 1 scored positions per sequence.  One workgroup per
// sequence; wave w folds the (max, sum exp) chunk pairs of rows t = w, w + 4, ... into lse[r] with x2_ce_combine's arithmetic (same bits)
// and leaves lse - z[label] (0 on an ignored row) in LDS; thread 0 then adds the T values in index order.  total (with c): one workgroup,
// thread i adds c[s] * loss_seq[s] for s = i, i + 256, ... in that order, then the row toolkit's fixed tree.
__global__ __launch_bounds__(VQ_THREADS) void seq_loss_combine_kernel(const float* __restrict__ part, int chunks, const float* __restrict__ zlab,
                                                                      const long* __restrict__ labels, int T, float* __restrict__ lse,
                                                                      float* __restrict__ loss_seq) {
  __shared__ float sRow[VQ_MAXLA];
  const int s = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t < T; t += ROW_WAVES) {
    const size_t r = (size_t)s * T + t;
    const float2* pr = reinterpret_cast<const float2*>(part) + r * chunks;
    float mx = -INFINITY;
    for (int ch = lane; ch < chunks; ch += 64) mx = fmaxf(mx, pr[ch].x);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float se = 0.f;
    for (int ch = lane; ch < chunks; ch += 64) { const float2 q = pr[ch]; se += q.y * __expf(q.x - mx); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o, 64);
    if (lane == 0) {
      const float l = mx + logf(se);
      lse[r] = l;
      sRow[t] = labels[r] >= 0 ? l - zlab[r] : 0.f;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += sRow[t];
    loss_seq[s] = acc;
  }
}
__global__ __launch_bounds__(VQ_THREADS) void seq_loss_total_kernel(const float* __restrict__ loss_seq, const float* __restrict__ c, int S,
                                                                    float* __restrict__ total) {
  __shared__ float sRed[ROW_WAVES];
  float acc = 0.f;
  for (int s = threadIdx.x; s < S; s += VQ_THREADS) acc += c[s] * loss_seq[s];
  acc = row_block_sum(acc, sRed);
  if (threadIdx.x == 0) total[0] = acc;
}

extern "C" int x2_seq_loss_combine(const float* part, int chunks, const float* zlab, const long* labels, int S, int T, const float* c, float* lse,
                                   float* loss_seq, float* total, void* stream) {
  X2_REQUIRE(part && zlab && labels && lse && loss_seq, "x2_seq_loss_combine: null tensor");
  X2_REQUIRE(S >= 1 && chunks >= 1 && (long)S * T < (1L << 31), "x2_seq_loss_combine: S=%d chunks=%d", S, chunks);
  X2_REQUIRE(T >= 1 && T <= VQ_MAXLA - 1, "x2_seq_loss_combine: La - 1 = %d must be in 1..%d", T, VQ_MAXLA - 1);
  X2_REQUIRE((c == nullptr) == (total == nullptr), "x2_seq_loss_combine: c and total come together");
  hipLaunchKernelGGL(seq_loss_combine_kernel, dim3(S), dim3(VQ_THREADS), 0, (hipStream_t)stream, part, chunks, zlab, labels, T, lse, loss_seq);
  if (c) hipLaunchKernelGGL(seq_loss_total_kernel, dim3(1), dim3(VQ_THREADS), 0, (hipStream_t)stream, loss_seq, c, S, total);
  return x2_check_launch("x2_seq_loss_combine");
}
