// The hard-negative draw of a row (xvlm.py:828-857), shared by x2_sample_negatives (heads.hip) and x2_sample_negatives_checked (retrieval.hip):
// one device function, so both entry points give the same bits.  block_reduce is heads.hip's workgroup reduction (the waves added left to right
// behind a leading barrier); the cross-entropy kernels of heads.hip use it as well.
#pragma once
#include "x2_common.h"
#include <math.h>

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
  return r;
}

// Row b = blockIdx.x: w[j] = softmax_j(sim[b][j]) + 1e-5, w[b] = 0 (or w[j] = 0 where group[j] == group[b]); draw one j
// with the uniform u[b] in [0,1) by inverse CDF.  One workgroup of 256 threads (<= 1024 columns) per row; no host sync.
// no_negative (or NULL): no_negative[b] = 1 where every candidate of the row is masked, else 0.
__device__ __forceinline__ void sample_negatives_row(const float* __restrict__ sim, int n, const long* __restrict__ group,
                                                     const float* __restrict__ u, int* out, int* no_negative) {
  __shared__ float sh[8];
  __shared__ float w[1024];
  const int b = blockIdx.x;
  const float* z = sim + (long)b * n;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < n; c += 256) mx = fmaxf(mx, z[c]);
  mx = block_reduce(mx, sh, true);
  float s = 0.f;
  for (int c = threadIdx.x; c < n; c += 256) s += __expf(z[c] - mx);
  s = block_reduce(s, sh, false);
  for (int c = threadIdx.x; c < n; c += 256) {
    const bool same = group ? group[c] == group[b] : c == b;
    w[c] = same ? 0.f : __expf(z[c] - mx) / s + 1e-5f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int c = 0; c < n; ++c) tot += w[c];
    const float t = u[b] * tot;
    float cum = 0.f; int pick = -1;
    for (int c = 0; c < n; ++c) { cum += w[c]; if (w[c] > 0.f && cum > t) { pick = c; break; } }
    if (pick < 0) for (int c = n - 1; c >= 0; --c) if (w[c] > 0.f) { pick = c; break; }
    // every candidate masked (all rows in one group): torch.multinomial raises in the reference (xvlm.py:845-855).  Called eagerly,
    // XVLMBase.get_hard_negatives rejects that batch on the host; inside a stream capture nothing is read back, the row is flagged in
    // no_negative and trains on the pair (b, b).  Never hand an out-of-range row index downstream.
    out[b] = pick < 0 ? b : pick;
    if (no_negative) no_negative[b] = pick < 0 ? 1 : 0;
  }
}
