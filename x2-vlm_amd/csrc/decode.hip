// Captioning inference (beam search over cached K/V): the three kernels of a decode step that the training path has no use for.
//   x2_attn_decode    self-attention of the step's n_new tokens over a per-row K/V cache, writing their K/V into it
//   x2_beam_gather    reorder the caches of all layers by the beam back pointers (ping-pong: src -> dst)
//   x2_logprob_topk   log-softmax + repeated-n-gram / EOS penalties + top-K of a row of fp32 logits in one pass
// Head dim 64, bf16 operands, fp32 accumulation.  No atomics: every output element has one writer.  The work per launch is tiny
// (<= 128 keys x 64 per (row, head)); what these kernels save is launches and host round trips, so they are plain VALU code.
#include "x2_common.h"
#include <math.h>

#define DEC_HD 64
#define DEC_MAXL 128          // cache positions a (row, head) workgroup holds in LDS
#define DEC_MAXNEW 16
#define DEC_THREADS 256
#define DEC_KS 33             // dwords per K row in LDS (64 bf16 + 1 dword pad: lanes on consecutive keys hit consecutive banks)

// ---------------------------------------------------------------------------------------------------------------- attention
// One workgroup per (row s, head h).  K/V of positions < hist come from the cache, those of the new tokens from the step's qkv rows
// (the workgroup never reads back what it writes), and the new tokens' K/V go to cache slots hist .. hist + n_new - 1 bit for bit.
// Query j (absolute position hist + j) attends positions 0 .. hist + j.
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_kernel(const bf16_t* __restrict__ qkv, int qkv_ld, bf16_t* __restrict__ cache,
                                                                  bf16_t* __restrict__ out, int out_ld, int H, int n_new, int hist,
                                                                  int Lmax, float scale) {
  __shared__ uint32_t sK[DEC_MAXL * DEC_KS];
  __shared__ uint32_t sV[DEC_MAXL * (DEC_HD / 2)];
  __shared__ float sQ[DEC_MAXNEW * DEC_HD];
  __shared__ float sP[DEC_MAXNEW * (DEC_MAXL + 1)];
  const int s = blockIdx.x / H, h = blockIdx.x % H, tid = threadIdx.x;
  const int Hd = H * DEC_HD, Lk = hist + n_new;
  const size_t crow = (size_t)2 * Hd;                                   // cache elements per position
  bf16_t* cbase = cache + (size_t)s * Lmax * crow + (size_t)h * DEC_HD;
  const bf16_t* qbase = qkv + (size_t)s * n_new * qkv_ld + (size_t)h * DEC_HD;
  // stage K and V: one 16-byte vector (8 bf16) per item; 8 vectors per 64-wide row, K then V
  for (int it = tid; it < Lk * 16; it += DEC_THREADS) {
    const int pos = it >> 4, which = (it >> 3) & 1, v8 = it & 7;
    u32x4 val;
    if (pos < hist) {
      val = *reinterpret_cast<const u32x4*>(cbase + (size_t)pos * crow + (size_t)which * Hd + v8 * 8);
    } else {
      val = *reinterpret_cast<const u32x4*>(qbase + (size_t)(pos - hist) * qkv_ld + (size_t)(1 + which) * Hd + v8 * 8);
      *reinterpret_cast<u32x4*>(cbase + (size_t)pos * crow + (size_t)which * Hd + v8 * 8) = val;
    }
    uint32_t* d = which ? &sV[pos * (DEC_HD / 2) + v8 * 4] : &sK[pos * DEC_KS + v8 * 4];
    d[0] = val.x; d[1] = val.y; d[2] = val.z; d[3] = val.w;
  }
  for (int it = tid; it < n_new * DEC_HD; it += DEC_THREADS)
    sQ[it] = bf2f(qbase[(size_t)(it >> 6) * qkv_ld + (it & 63)]);
  __syncthreads();
  // scores
  for (int it = tid; it < n_new * Lk; it += DEC_THREADS) {
    const int j = it / Lk, k = it - j * Lk;
    float acc = -INFINITY;
    if (k <= hist + j) {
      acc = 0.f;
      const uint32_t* kr = &sK[k * DEC_KS];
      const float* qr = &sQ[j * DEC_HD];
#pragma unroll 8
      for (int d2 = 0; d2 < DEC_HD / 2; ++d2) {
        const uint32_t u = kr[d2];
        acc = fmaf(qr[2 * d2], bf_lo(u), acc);
        acc = fmaf(qr[2 * d2 + 1], bf_hi(u), acc);
      }
      acc *= scale;
    }
    sP[j * (DEC_MAXL + 1) + k] = acc;
  }
  __syncthreads();
  // softmax: a wave per query row
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < n_new; j += DEC_THREADS / 64) {
    float* pr = &sP[j * (DEC_MAXL + 1)];
    const float a = lane < Lk ? pr[lane] : -INFINITY, b = lane + 64 < Lk ? pr[lane + 64] : -INFINITY;
    const float m = wave_max(fmaxf(a, b));                               // finite: key 0 is visible to every query
    const float ea = expf(a - m), eb = expf(b - m);
    const float inv = 1.0f / wave_sum(ea + eb);
    if (lane < Lk) pr[lane] = ea * inv;
    if (lane + 64 < Lk) pr[lane + 64] = eb * inv;
  }
  __syncthreads();
  // P V
  for (int it = tid; it < n_new * DEC_HD; it += DEC_THREADS) {
    const int j = it >> 6, d = it & 63;
    const float* pr = &sP[j * (DEC_MAXL + 1)];
    const bf16_t* vc = reinterpret_cast<const bf16_t*>(sV) + d;
    float acc = 0.f;
    const int last = hist + j;
    for (int k = 0; k <= last; ++k) acc = fmaf(pr[k], bf2f(vc[k * DEC_HD]), acc);
    out[(size_t)(s * n_new + j) * out_ld + h * DEC_HD + d] = f2bf(acc);
  }
}

extern "C" int x2_attn_decode(const void* qkv, int qkv_ld, void* cache, void* out, int out_ld, int S, int H, int n_new, int hist, int Lmax,
                              float scale, void* stream) {
  X2_REQUIRE(qkv && cache && out, "x2_attn_decode: null tensor");
  X2_REQUIRE(S > 0 && H > 0 && (long)S * H < (1L << 31), "x2_attn_decode: S=%d H=%d", S, H);
  X2_REQUIRE(n_new >= 1 && n_new <= DEC_MAXNEW, "x2_attn_decode: n_new=%d must be in 1..%d", n_new, DEC_MAXNEW);
  X2_REQUIRE(Lmax > 0 && Lmax <= DEC_MAXL && Lmax % 8 == 0, "x2_attn_decode: Lmax=%d must be a multiple of 8, at most %d", Lmax, DEC_MAXL);
  X2_REQUIRE(hist >= 0 && hist + n_new <= Lmax, "x2_attn_decode: hist=%d + n_new=%d exceeds Lmax=%d", hist, n_new, Lmax);
  X2_REQUIRE(qkv_ld >= 3 * H * DEC_HD && qkv_ld % 8 == 0 && out_ld >= H * DEC_HD, "x2_attn_decode: qkv_ld=%d out_ld=%d for H=%d (head dim %d)",
             qkv_ld, out_ld, H, DEC_HD);
  X2_REQUIRE(((uintptr_t)qkv | (uintptr_t)cache) % 16 == 0, "x2_attn_decode: qkv and cache must be 16-byte aligned");
  hipLaunchKernelGGL(attn_decode_kernel, dim3(S * H), dim3(DEC_THREADS), 0, (hipStream_t)stream, (const bf16_t*)qkv, qkv_ld, (bf16_t*)cache,
                     (bf16_t*)out, out_ld, H, n_new, hist, Lmax, scale);
  return x2_check_launch("x2_attn_decode");
}

// ---------------------------------------------------------------------------------------------------------------- cache reorder
// dst[l][s][0:hist] = src[l][parent[s]][0:hist]: the kept positions of a row are contiguous, so each (layer, row) is one copy of
// hist * row_elems bf16 in 16-byte vectors, split over blockIdx.y.
__global__ __launch_bounds__(256) void beam_gather_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, const int* __restrict__ parent,
                                                         int S, long row_vecs, long keep_vecs) {
  const int l = blockIdx.x / S, s = blockIdx.x % S;
  const int p = parent[s];
  if ((unsigned)p >= (unsigned)S) return;                                // an index outside the batch copies nothing
  const u32x4* sp = src + ((long)l * S + p) * row_vecs;
  u32x4* dp = dst + ((long)l * S + s) * row_vecs;
  for (long i = (long)blockIdx.y * blockDim.x + threadIdx.x; i < keep_vecs; i += (long)gridDim.y * blockDim.x) dp[i] = sp[i];
}

extern "C" int x2_beam_gather(const void* src, void* dst, const int* parent, int layers, int S, int Lmax, int row_elems, int hist, void* stream) {
  X2_REQUIRE(src && dst && parent, "x2_beam_gather: null tensor");
  X2_REQUIRE(layers > 0 && S > 0 && Lmax > 0 && (long)layers * S < (1L << 31), "x2_beam_gather: layers=%d S=%d Lmax=%d", layers, S, Lmax);
  X2_REQUIRE(row_elems > 0 && row_elems % 8 == 0, "x2_beam_gather: row_elems=%d must keep 16-byte rows", row_elems);
  X2_REQUIRE(hist >= 1 && hist <= Lmax, "x2_beam_gather: hist=%d outside 1..Lmax=%d", hist, Lmax);
  X2_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "x2_beam_gather: src and dst must be 16-byte aligned");
  const long bytes = (long)layers * S * Lmax * row_elems * 2;
  const char *a = (const char*)src, *b = (const char*)dst;
  X2_REQUIRE(a + bytes <= b || b + bytes <= a, "x2_beam_gather: src and dst must be different buffers (src == dst or overlapping is refused)");
  const long row_vecs = (long)Lmax * row_elems / 8, keep_vecs = (long)hist * row_elems / 8;
  const int ny = (int)((keep_vecs + 256 * 4 - 1) / (256 * 4));
  hipLaunchKernelGGL(beam_gather_kernel, dim3(layers * S, ny < 1 ? 1 : (ny > 64 ? 64 : ny)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src,
                     (u32x4*)dst, parent, S, row_vecs, keep_vecs);
  return x2_check_launch("x2_beam_gather");
}

// ---------------------------------------------------------------------------------------------------------------- scoring
#define LP_THREADS 256
#define LP_MAXK 8
#define LP_MAXSEQ 256
static_assert(LP_THREADS == 256 && DEC_THREADS == 256, "the block reductions below combine exactly four waves");

__device__ __forceinline__ bool lp_better(float av, int ac, float bv, int bc) { return av > bv || (av == bv && ac < bc); }

// One workgroup per row: log_softmax over the V valid columns (the padding columns are never read), -10000 ADDED to every token that
// would complete a repeated n-gram of the row's ids so far, column eos_id SET to -10000 when forbid_eos, then the K largest values,
// largest first, lowest column first among equal values.  logs (optional) receives the V penalised log-scores.
__global__ __launch_bounds__(LP_THREADS) void logprob_topk_kernel(const float* __restrict__ logits, int ldv, int V, const int* __restrict__ seq,
                                                                  int Lseq, int seq_len, int ngram, int eos_id, int forbid_eos, int K,
                                                                  float* __restrict__ out_vals, int* __restrict__ out_ids,
                                                                  float* __restrict__ logs) {
  __shared__ int sBan[LP_MAXSEQ];
  __shared__ float sRedF[LP_THREADS / 64];
  __shared__ int sRedC[LP_THREADS / 64];
  __shared__ int sRedT[LP_THREADS / 64];
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* x = logits + (size_t)row * ldv;
  // banned tokens: entry i is seq[i + n - 1] when seq[i .. i + n - 2] equals the last n - 1 ids, else -1
  const int nban = (seq && ngram >= 1 && seq_len >= ngram) ? seq_len - ngram + 1 : 0;
  for (int i = tid; i < nban; i += LP_THREADS) {
    const int* sq = seq + (size_t)row * Lseq;
    bool same = true;
    for (int j = 0; j < ngram - 1; ++j) same = same && sq[i + j] == sq[seq_len - (ngram - 1) + j];
    sBan[i] = same ? sq[i + ngram - 1] : -1;
  }
  // max, then sum of exp
  float m = -INFINITY;
  for (int c = tid; c < V; c += LP_THREADS) m = fmaxf(m, x[c]);
  m = wave_max(m);
  if (lane == 0) sRedF[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sRedF[0], sRedF[1]), fmaxf(sRedF[2], sRedF[3]));
  __syncthreads();
  float sum = 0.f;
  for (int c = tid; c < V; c += LP_THREADS) sum += expf(x[c] - m);
  sum = wave_sum(sum);
  if (lane == 0) sRedF[wave] = sum;
  __syncthreads();
  const float lsum = logf((sRedF[0] + sRedF[1]) + (sRedF[2] + sRedF[3]));
  __syncthreads();
  // per-thread top 8 over its columns (ascending, so a later equal value never displaces an earlier one)
  float tv[LP_MAXK];
  int tc[LP_MAXK];
#pragma unroll
  for (int i = 0; i < LP_MAXK; ++i) { tv[i] = -INFINITY; tc[i] = 0x7fffffff; }
  for (int c = tid; c < V; c += LP_THREADS) {
    float v = (x[c] - m) - lsum;
    bool ban = false;
    for (int i = 0; i < nban; ++i) ban = ban || sBan[i] == c;
    if (ban) v += -10000.0f;
    if (forbid_eos && c == eos_id) v = -10000.0f;
    if (logs) logs[(size_t)row * V + c] = v;
    if (v > tv[LP_MAXK - 1]) {
      tv[LP_MAXK - 1] = v; tc[LP_MAXK - 1] = c;
#pragma unroll
      for (int i = LP_MAXK - 1; i > 0; --i) {
        if (tv[i] > tv[i - 1]) {
          const float fv = tv[i]; tv[i] = tv[i - 1]; tv[i - 1] = fv;
          const int fc = tc[i]; tc[i] = tc[i - 1]; tc[i - 1] = fc;
        }
      }
    }
  }
  // K rounds: the best head of all threads wins, its owner moves to its next entry
  for (int r = 0; r < K; ++r) {
    float bv = tv[0];
    int bc = tc[0], bt = tid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64), ot = __shfl_xor(bt, o, 64);
      if (lp_better(ov, oc, bv, bc)) { bv = ov; bc = oc; bt = ot; }
    }
    if (lane == 0) { sRedF[wave] = bv; sRedC[wave] = bc; sRedT[wave] = bt; }
    __syncthreads();
    bv = sRedF[0]; bc = sRedC[0]; bt = sRedT[0];
#pragma unroll
    for (int w = 1; w < LP_THREADS / 64; ++w)
      if (lp_better(sRedF[w], sRedC[w], bv, bc)) { bv = sRedF[w]; bc = sRedC[w]; bt = sRedT[w]; }
    __syncthreads();
    if (tid == 0) { out_vals[(size_t)row * K + r] = bv; out_ids[(size_t)row * K + r] = bc; }
    if (tid == bt) {
#pragma unroll
      for (int i = 0; i < LP_MAXK - 1; ++i) { tv[i] = tv[i + 1]; tc[i] = tc[i + 1]; }
      tv[LP_MAXK - 1] = -INFINITY; tc[LP_MAXK - 1] = 0x7fffffff;
    }
  }
}

extern "C" int x2_logprob_topk(const float* logits, int ldv, int V, int S, const int* seq, int Lseq, int seq_len, int ngram, int eos_id,
                               int forbid_eos, int K, float* out_vals, int* out_ids, float* logs, void* stream) {
  X2_REQUIRE(logits && out_vals && out_ids, "x2_logprob_topk: null tensor");
  X2_REQUIRE(S > 0 && V > 0 && ldv >= V, "x2_logprob_topk: S=%d V=%d ldv=%d", S, V, ldv);
  X2_REQUIRE(K >= 1 && K <= LP_MAXK && K <= V, "x2_logprob_topk: K=%d must be in 1..%d and at most V=%d", K, LP_MAXK, V);
  X2_REQUIRE(eos_id >= 0 && eos_id < V, "x2_logprob_topk: eos_id=%d outside the vocabulary %d", eos_id, V);
  X2_REQUIRE(ngram >= 0 && seq_len >= 0, "x2_logprob_topk: ngram=%d seq_len=%d", ngram, seq_len);
  X2_REQUIRE(!seq || (seq_len <= Lseq && seq_len <= LP_MAXSEQ), "x2_logprob_topk: seq_len=%d exceeds Lseq=%d or %d", seq_len, Lseq, LP_MAXSEQ);
  hipLaunchKernelGGL(logprob_topk_kernel, dim3(S), dim3(LP_THREADS), 0, (hipStream_t)stream, logits, ldv, V, seq, Lseq, seq_len, ngram, eos_id,
                     forbid_eos, K, out_vals, out_ids, logs);
  return x2_check_launch("x2_logprob_topk");
}
