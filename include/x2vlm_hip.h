/* x2vlm_hip.h — C ABI of libx2vlm_hip.so: the MI355X (gfx950) kernels of the X^2-VLM pre-training step.
 *
 * The reference (zengyan-97/X2-VLM) is 100 % Python and has no FFI layer: every entry point below replaces
 * an implicit ATen / cuBLAS / cuDNN call made by the cited reference line (forward AND its autograd
 * backward).  A maintainer binds them with ctypes (INTEGRATION.md shows the stub); x2-vlm_amd/_lib.py is
 * that binding, x2-vlm_amd/kernels.py the tensor-level wrappers.
 *
 * Conventions
 *   - extern "C", POD arguments only: device pointers as void* / typed pointers, sizes as int / long,
 *     the HIP stream as void* (hipStream_t).  No torch types.
 *   - returns 0 on success, < 0 on error (-1 bad argument, -2 launch failure); x2_last_error() gives the
 *     message (thread-local).  Nothing is launched when an argument check fails.
 *   - the caller owns all memory; kernels never allocate, never synchronise the host; every call is
 *     asynchronous and ordered on the stream passed in; distinct streams may be used concurrently.
 *   - bf16 tensors are raw uint16 bit patterns; "ld*" are leading dimensions in ELEMENTS.
 *   - gradients documented as "+=" are added onto caller-initialised memory; since ABI v12 no entry point the training step uses adds
 *     with atomics (every sum has a fixed order: two runs give the same bits); the two that still can - x2_gemm_nt(colsum != NULL) and
 *     x2_gemm_tn_grouped on its 128x128 kernel with split > 1 and no workspace - say so below.
 */
#ifndef X2VLM_HIP_H
#define X2VLM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* x2_last_error(void);
int x2_abi_version(void);          /* == 14 */
int x2_device_cus(void);           /* compute units of the current HIP device, 0 if none */
int x2_tune(int key, int value);   /* kernel-variant knobs for probes/ and tests (0 = automatic); keys 0 1 2 3 5 10 12 13 14 15, listed in csrc/gemm.hip,
                                    * any other key is refused.
                                    * key 12 = compute units every tile plan leaves to RCCL's channel kernels (world > 1);
                                    * key 14 = 1: attention backward as two kernels even where a one-pass kernel applies (3: only the long form 3 off);
                                    * key 15 = NT ping-pong kernel (32x32x16 MFMAs): 0 automatic, 1 never, 3 .. 6 always, at 32 x value rows;
                                    * key 2 (work-skipping ablation bits) is refused unless the library was built with -DX2_PROBE */
int x2_tune_get(int key);          /* current value of a knob, -1 for an unknown key (bench.py reports the non-default ones) */

/* ---- dense contractions (csrc/gemm.hip) -------------------------------------------------------------
 * F.linear of beit2.py:131 (fused qkv), :160 (proj), :62/:66 (MLP); xbert.py:338-350 (Q/K/V, cross K/V from
 * image tokens), :428 (attention output), :497 (intermediate), :512 (output), :798 (MLM transform),
 * :822 (tied decoder); nn.Conv2d patch embedding beit2.py:225,231 (as a GEMM over patch rows).
 *
 * C[M,N] = epilogue(A[M,K] . B[N,K]^T), bf16 operands, fp32 MFMA accumulation.  K % 64 == 0, N % 8 == 0.
 *   v = acc + bias[n]
 *   act == 1: aux[m,n] = bf16(v); v = gelu(v)        (erf form)   -> fc1 / intermediate forward
 *   act == 2: v *= gelu'(aux[m,n])                                 -> dgrad through the GELU
 *   act == 0 and aux != NULL: aux[m,n] = bf16(v)                   -> value before layer scale (for dgamma)
 *   v *= dropout(v)   (drop_thr16 != 0: hidden dropout, xbert.py:429, 513; counter-based, see below)
 *   v *= gamma[n]; v *= rowscale[m]; v += resid[m,n]               -> x + drop_path(gamma_1 * proj(...)) (beit2.py:206-207),
 *                                                                     dropout(dense(x)) + residual (xbert.py:430,514)
 * Dropout everywhere in this ABI: element e of a site is dropped iff u16(hash(e >> 1 ^ seed), e & 1) < thr16
 * (thr16 = round(p * 65536), 0 = off); survivors are multiplied by `scale`.  The backward regenerates the mask
 * from the same (thr16, seed, scale); kernels.dropout_keep() is the host mirror.
 * drop_epoch (every dropout-capable entry point): NULL, or a device word holding a step counter that is mixed into the
 * seed (seed' = hash(seed + 0x9E3779B1 * *drop_epoch)): a hipGraph-captured step, whose kernel arguments are frozen,
 * increments the word once per replay and so draws new masks on every step.
 *   C = out_f32 ? float : bf16.  Forward linears pass B = W (N x K); input gradients pass B = W^T. */
int x2_gemm_nt(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
               const float* bias, const float* gamma, const float* resid, int ldr, void* aux, int ldaux,
               int act, int out_f32, unsigned drop_thr16, unsigned drop_seed, float drop_scale, const unsigned* drop_epoch,
               const float* rowscale, float* colsum, void* stream);      /* colsum[n] += sum_m C[m,n] (fused bias gradient), NULL = off */

/* C = (A . B^T) x GELU'(aux) -> bf16 plus the column sums of C as partial rows colparts[r][N], r < *nrows_out (2 per row tile
 * of the launch; colparts must hold 2 * ceil(M / 64) rows); the caller adds them with x2_reduce_partials(_multi)(colparts,
 * *nrows_out, 1, N, out).  Input gradient through the MLP's GELU + bias gradient of its first linear in one kernel
 * (autograd of beit2.py:62-66, xbert.py:497: GeluBackward + the bias reduction of AddmmBackward). */
int x2_gemm_nt_dgelu_colparts(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                              const void* aux, int ldaux, float* colparts, int* nrows_out, void* stream);
/* The same product with a split contraction, for few output tiles and a long K: C[M,N] (fp32, no epilogue) =
 * A[M,K] . B[N,K]^T.  The input gradient of the tied MLM decoder (reference: autograd of the F.linear behind
 * xbert.py:822, dt[R,768] = dlogits[R,30528] . E) is 36-72 output tiles of 477 contraction steps - a serial chain on a
 * seventh of the chip.  Slice s of the contraction writes its partial product to ws[s*M*N ...]; a second kernel adds the
 * slices in a fixed order (deterministic, no atomics).  slices: 0 = chosen to put two workgroups on every CU with at
 * least 8 contraction steps each; clamped to ws_floats / (M*N); ws = NULL or one slice: a single launch straight into C. */
int x2_gemm_nt_splitk(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                      int slices, float* ws, long ws_floats, void* stream);

/* Weight gradients of one layer in one launch: for each problem  dW[N,K] (+)= dY[Mc,N]^T . X[Mc,K]  (fp32 out).
 * problems: count (<= 8) rows of 11 int64 {dY, X, dW, Mc, N, K, ld_dY, ld_X, ld_dW, n_ld, k_ld}; n_ld / k_ld are
 * the readable widths of dY / X rows (>= N / K, multiples of 8).  accumulate: dW += instead of dW =.
 * Contraction lengths that are all multiples of 64 run on 256x256 tiles (one workgroup per CU); split = slices of the
 * contraction per tile (0 = chosen to fill the CUs), whose partial tiles pass through ws (split * tiles256 * 65536
 * floats; ws = NULL: never split) and are added in a fixed order; an explicit split > 1 with a workspace takes this path whatever the tile
 * count.  Otherwise 128x128 tiles, where split > 1 (without a workspace) adds with fp32 atomics and requires accumulate. */
int x2_gemm_tn_grouped(const int64_t* problems, int count, int accumulate, int split, float* ws, long ws_floats,
                       void* stream);
/* A queue of such problems (every layer whose operands are ready) as whole rounds of the compute units: additive to ABI v14, no existing
 * signature changes.  The 256x256 tiles of all problems are walked in the order given.  The largest multiple of `cus` tiles (main part) runs
 * unsplit and stores directly, cut into launches only where a launch's 32 windows run out (then at the last whole round they reach); a window is (problem, first tile, tile count) of a
 * problem's own tile grid, so a launch may end or begin in the middle of a problem.  The tiles left over (fewer than cus) are one more launch
 * under the split rule of x2_gemm_tn_grouped (fullest last round, slices of at least 16 contraction steps, workspace permitting): partial
 * tiles and the fixed-order reduction apply to those tiles only.  A queue of at most one round is all remainder: x2_gemm_tn_grouped(split = 0).
 *   x2_tn_plan : the plan, pure host arithmetic (no device call).  shapes: count rows of 3 int64 {Mc, N, K}; cus <= 0: the count the library
 *       plans with (the device's, less x2_tune(12)); ws_floats: room for partial tiles.  windows: rows of 4 int32 {launch, problem, first tile,
 *       tile count} in launch order; launches: rows of 2 int32 {split, 1 = remainder}.  *n_windows / *n_launches: the plan's sizes; with
 *       max_windows == max_launches == 0 only they are written, more rows than the room given returns -1.
 *   x2_gemm_tn_queue : runs launches [first_launch, first_launch + n_launches) of that plan (n_launches == 0: all from first_launch on) for
 *       problems as x2_gemm_tn_grouped takes them, any count.  Work that must follow the launch completing a problem runs the plan a launch
 *       at a time.  Fewer than 24 tiles in all: x2_gemm_tn_grouped in groups of 8 (one launch, first_launch must be 0). */
int x2_tn_plan(const int64_t* shapes, int count, int cus, long ws_floats, int* windows, int max_windows, int* launches, int max_launches,
               int* n_windows, int* n_launches);
int x2_gemm_tn_queue(const int64_t* problems, int count, int accumulate, float* ws, long ws_floats, int first_launch, int n_launches,
                     void* stream);

/* ---- fused attention, head dim 64 (csrc/attention.hip) ----------------------------------------------
 * beit2.py:135-159 (q*scale, QK^T, + relative_position_bias, softmax, PV); xbert.py:364-409 (QK^T/sqrt(d),
 * + additive mask, softmax, PV) for self-attention and for cross-attention to image tokens (xbert.py:345-348).
 * Scores/probabilities never reach HBM.  kv_idx lets several query batches share one K/V batch.
 * Field order is the ABI (mirrored by ctypes.Structure in x2-vlm_amd/_lib.py). */
typedef struct X2AttnArgs {
  const void *Q, *K, *V, *O, *dO;            /* bf16; O/dO: backward inputs                               */
  void *Out, *dQ, *dK, *dV, *dS;             /* bf16 outputs; dS [B][H][Lq][ds_ld] optional (bias grad)   */
  float *LSE, *Delta;                        /* [B][H][Lq] fp32: log2-domain logsumexp; rowsum(dO*O)      */
  long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;            /* batch / row strides, elements        */
  long dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs, do_bs, do_rs;
  int B, Bkv, H, Lq, Lk;
  float scale;
  const float* bias;  int bias_ld;           /* [H][Lq][bias_ld]  additive, bias_ld % 64 == 0             */
  const float* biasT; int biasT_ld;          /* [H][Lk][biasT_ld] transposed copy (backward)              */
  const float* mask;  int mask_ld;           /* [B][mask_ld] additive per key, mask_ld % 64 == 0          */
  const int* kv_idx;                         /* [B] query batch -> K/V batch, NULL = identity             */
  const int* seq_off; const int* seq_ids;    /* CSR inverse of kv_idx (backward dK/dV), NULL = identity   */
  int ds_ld;
  unsigned drop_thr16, drop_seed; float drop_scale;   /* dropout on the probabilities (xbert.py:399);
                                                          element = ((b*H + h)*Lq + q) * round_up(Lk,64) + key */
  int dbg;                                           /* 0; ablation switches for probes/bench_attn.py */
  int head_dim;                                      /* hidden / heads of the caller: must be 64, checked */
  const unsigned* drop_epoch;                        /* device step counter mixed into drop_seed, or NULL */
  int grid_nx, grid_ny, grid_nz, grid_map;           /* written by the library (XCD-aware workgroup order of the bias kernels): pass 0 */
  int phase;                                         /* x2_attn_bwd: 0 = dQ (+dS, Delta) then dK/dV; 1 = the dQ half only; 2 = the dK/dV half only
                                                        (reads the Delta a phase-1 call wrote): the K/V-side gradients on another stream */
  float* ws; long ws_floats;                         /* x2_attn_bwd (ABI v13): fp32 scratch of B * H * ceil(Lq / 128) * 8192 floats for the long one-pass
                                                        backward (form 3 below), or NULL / smaller: such a geometry runs the two kernels */
  float* colsum_ws;                                  /* x2_attn_bwd (ABI v14), honoured by forms 1 and 3 only (ask x2_attn_bwd_one_pass), or NULL: [B][2][H*64] fp32,
                                                        per sequence the column sums of the stored dQ (k = 0) and dV (k = 1) rows - summed over B
                                                        (x2_reduce_partials, nblk = B, nk = 2) they are the q / v bias gradient of the fused qkv
                                                        projection (beit2.py:129-131: qkv_bias = cat(q_bias, 0, v_bias)) without a pass over [M, 3D] */
} X2AttnArgs;
int x2_attn_fwd(const X2AttnArgs* args, void* stream);
int x2_attn_bwd(const X2AttnArgs* args, void* stream);   /* dQ (+dS, Delta) then dK/dV; no atomics */
/* Which backward a phase-0 x2_attn_bwd call with these arguments runs: 0 = two kernels (dQ, then dK/dV), 1 = one pass, one workgroup per
 * (sequence, head) (64 < Lq, Lk <= 208, no K/V sharing, no probability dropout: the BEiT-2 blocks, beit2.py:135-159), 2 = one pass, one
 * workgroup per (shared K/V batch, head) (Lq <= 128, Lk <= 208, no bias: the cross-attention of xbert.py:322-415), 3 = one pass, one workgroup
 * per (sequence, head) that walks 256-key parts x 128-query chunks (208 < Lq <= 640, 208 < Lk <= 768, no K/V sharing, no probability
 * dropout, `ws` given, biasT_ld >= 128 ceil(Lq / 128): the BEiT-2 blocks of X2VLM-large at 384 px, N = 577).  A caller that
 * would put the dK/dV half (phase 2) on another stream asks first: in one pass there is no such half. */
int x2_attn_bwd_one_pass(const X2AttnArgs* args);

/* ---- row-wise kernels (csrc/rowwise.hip) ------------------------------------------------------------
 * nn.LayerNorm: beit2.py:175,181,411 (eps 1e-6); xbert.py:214,422,506,796 (1e-12); xvlm.py:166 (1e-5).
 * period > 0: rows are the non-cls tokens of a (B, period+1, D) tensor (row r -> r + r/period + 1), used for
 * fc_norm over patches (beit2.py:409-411). */
int x2_layernorm_fwd(const float* x, const float* w, const float* b, void* y_bf16, float* y_f32, float* mean,
                     float* rstd, int rows, int D, float eps, int period, unsigned drop_thr16, unsigned drop_seed,
                     float drop_scale, const unsigned* drop_epoch, void* stream);   /* drop: dropout on the LN output (xbert.py:215) */
/* g = LN'(mask_in(dy)); dx = dres + g (fp32); dx_bf16 = mask_out(g); dw += , db += ; dcol += column sums of mask_out(g)
 * (= gradient and bias gradient of the linear whose dropped output was added to the residual before this LN).
 * post != 0 (dy bf16, period 0, no output mask): the by-products describe the FINAL output instead - dx_bf16 =
 * post_rowscale[row] * dx (post_rowscale NULL = 1), dcol += its column sums: what the layer scale below this LayerNorm needs
 * of its incoming gradient (x2_layerscale_finish) */
int x2_layernorm_bwd(const void* dy /* fp32, or bf16 when dy_is_bf16 */, int dy_is_bf16, const float* x, const float* mean, const float* rstd, const float* w,
                     const float* dres, float* dx, void* dx_bf16, float* dw, float* db, float* dcol, int rows, int D,
                     int period, unsigned in_thr16, unsigned in_seed, float in_scale, unsigned out_thr16,
                     unsigned out_seed, float out_scale, const unsigned* drop_epoch, float* ws /* [ceil(rows/16)][3][D] */,
                     int defer, int post, const float* post_rowscale, void* stream);
/* Column reductions are two-stage (per-workgroup partial rows in the caller's workspace `ws`, then a deterministic
 * add): fp32 atomics measured ~43 G adds/s on MI355X, slower than the HBM traffic of these kernels. */
int x2_colsum_bf16(const void* y, float* out, int M, int N, int ld, float* ws /* [ceil(M/64)][N] */, int defer, void* stream);
/* defer != 0: only stage 1 (partials into ws); the caller finishes with x2_reduce_partials, possibly on another stream:
 * out_k[c] += sum_blk ws[blk][k][c], k < nk <= 3 */
int x2_reduce_partials(const float* part, int nblk, int nk, int width, float* o0, float* o1, float* o2, void* stream);
/* `count` such reductions in one launch (all parameter-gradient sums of one layer's backward), nk <= 4 here;
 * desc: count rows of 8 int64 {part, nblk, nk, width, o0, o1, o2, o3} (a null output skips that partial row) */
int x2_reduce_partials_multi(const int64_t* desc, int count, void* stream);
/* backward of x + r[m] * gamma * u, u = A . W^T + b (beit2.py:206-207; r = DropPath factor or 1) without a pass over u: with
 * dX' = r * dX the input gradient is dX' . (diag(gamma) W) (x2_cast_transpose_multi folds gamma into the W^T copy), the weight-
 * gradient GEMM computes G = dX'^T . A, and x2_layerscale_finish turns G and cs = colsum(dX') into
 *   dgamma += rowdot(G, W) + b * cs,  dbias += gamma * cs,  G <- diag(gamma) G  (= dW).
 * desc: count rows of 9 int64 {G [N][K] fp32, W [N][K] fp32 master weight, b or 0, gamma, cs, dgamma, dbias or 0, N, K}.
 * dX' (bf16) and cs come from x2_layernorm_bwd (post = 1) or from x2_rowscale_cast_colsum. */
int x2_layerscale_finish(const int64_t* desc, int count, void* stream);
int x2_rowscale_cast_colsum(const float* dx, const float* rowscale, void* dx_bf16, float* colsum, int M, int D,
                            float* ws /* [ceil(M/32)][D] */, int defer, void* stream);
int x2_cast_bf16(const float* src, void* dst, long n, void* stream);
/* src [R][C] fp32 -> dst [R][C] bf16 (or NULL) and dstT [C][ldt] bf16 = src^T, ldt >= R: columns R..ldt-1 of dstT are left untouched (a caller that
 * reads them as padding zeroes them once) */
int x2_cast_transpose_bf16(const float* src, void* dst, void* dstT, int R, int C, int ldt, void* stream);
/* bf16 (W, W^T) copies of many fp32 weights in one launch (what apex O1's per-call weight casts amount to, done once per
 * optimizer step): desc = count rows of 8 int64 {src, dst, dstT, R, C, ldt, roff, tscale}: src [R][C] fp32 -> rows roff.. of
 * dst [*][C] and columns roff.. of dstT [C][ldt]; R, C, ldt, roff multiples of 4; tscale (fp32 [R]) or 0: the transposed
 * copy holds tscale[r] * src[r][c] (a layer scale folded into the weight of the input-gradient GEMM) */
int x2_cast_transpose_multi(const int64_t* desc, int count, void* stream);
/* many small fp32 vectors packed in one launch (stacked q/k/v biases): desc = count rows {src or 0 = zeros, dst, n} */
int x2_copy_f32_multi(const int64_t* desc, int count, void* stream);
/* PatchEmbed input rows (beit2.py:225-232): image (B,3,R,R) -> bf16 [B*(R/ps)^2][3*ps*ps] */
int x2_patchify(const float* image, void* cols, int B, int R, int ps, void* stream);
/* torch.cat((cls_tokens, x), 1) (beit2.py:385-387) and its backward */
int x2_assemble_tokens(const float* patch, const float* cls, float* x, int B, int P, int D, void* stream);
int x2_assemble_tokens_bwd(const float* dx, void* dpatch_bf16, float* dcls, int B, int P, int D, void* stream);
/* token 0 <- (weighted) mean of patch tokens: avgpool beit2.py:413-416, region pooling beit2.py:430-436 */
int x2_pool_tokens(float* x, const float* w, int B, int P, int D, int bwd, void* stream);
/* relative_position_bias_table[relative_position_index] x scale -> [H][N][ld] (+ transposed), beit2.py:138-144; the pad columns N..ld-1 /
 * N..ldT-1 are written as zeros.  scale = 1, or
 * log2(e) for a bias in the unit the attention kernels' softmax works in: set bit 4 (16) of X2AttnArgs.dbg with such a bias
 * (no mask) and a score costs one fma instead of four VALU operations */
int x2_relpos_bias(const float* table, const long* index, const long* indexT /* index^T or NULL */, float* bias, float* biasT, int N, int H, int ld, int ldT,
                   float scale, void* stream);
/* dtable[index[i][j]][h] += sum_b dS[b][h][i][j] (dS bf16 [B][H][N][ld]); the index arrives as its CSR inverse
 * (inv_off [T+1], inv_pos = i*ld + j); ws: slices*H*N*ld floats (batch-slice sums, then a gather: no atomics).
 * Reads columns j < 8 ceil(N / 8) of dS only: the one-pass attention backward leaves columns >= 16 ceil(N / 16) of its dS stream unwritten. */
int x2_relpos_bias_bwd(const void* dS, const int* inv_off, const int* inv_pos, float* dtable, int B, int N, int H, int ld,
                       int T, float* ws, int slices, void* stream);

/* ---- embeddings, heads, losses (csrc/heads.hip) -----------------------------------------------------
 * BertEmbeddings xbert.py:205-213 (word + position + token-type 0); backward scatter-adds. */
int x2_embed_fwd(const long* ids, const float* word, const float* pos, const float* type0, float* out, int R, int L,
                 int D, void* stream);
/* dword[ids[r]] += g[r], dpos[r % L] += g[r], dtype0 += sum_r g[r]: every sum in a fixed order (no atomics: rows with the same token id are added in
 * ascending r by one workgroup; position totals pass through `scratch`, min(L, R) * D floats).  D <= 4096. */
int x2_embed_bwd(const long* ids, const float* g, float* dword, float* dpos, float* dtype0, int R, int L, int D,
                 float* scratch, void* stream);
/* torch.gather of sequences / masked positions (xbert.py:1588-1589, xvlm.py:866-884) and its backward */
int x2_gather_rows(const float* src, const int* idx, float* dst, void* dst_bf16, int R, long len, void* stream);
/* dst[d][:] = sum of src[r][:] over idx[r] == d, all D rows of dst written (zeros where nothing points); no atomics; R <= 8192 */
int x2_scatter_rows(const float* src, const int* idx, float* dst, int R, int D, long len, void* stream);
/* small fp32 linear with arbitrary strides: vision_proj / text_proj (xvlm.py:785-792), similarity matrices
 * (xvlm.py:807, 831-832), last layers of itm_head / bbox_head (xvlm.py:163-169) and their backward */
int x2_linear_f32(const float* A, const float* B, float* C, const float* bias, const float* alpha_ptr, float alpha,
                  int M, int N, int K, long sam, long sak, long sbn, long sbk, long ldc, int accumulate,
                  int ksplit /* K slices; > 1: partial tiles through ws, added in slice order */,
                  float* ws /* ksplit * M * N floats when ksplit > 1 */, void* stream);
int x2_l2norm(const float* x, const float* dy, float* out, int R, int D, int bwd, void* stream);   /* F.normalize */
/* F.cross_entropy / CrossEntropyLoss(ignore_index=-100): xvlm.py:812-813, 899; xbert.py:1660-1661.
 * out2 = {mean loss, number of counted rows}; backward writes (softmax - onehot) * gscale * g / count. */
int x2_ce_fwd(const float* logits, long ld, const long* labels, int R, int C, float* lse, float* loss_row, float* out2,
              void* stream);
int x2_ce_bwd(const float* logits, long ld, const long* labels, const float* lse, const float* g, const float* stat,
              float gscale, int R, int C, float* dl_f32, void* dl_bf16, long ldd, void* stream);
/* The MLM head's cross-entropy over the tied decoder with the logits kept in the GEMM accumulators (reference:
 * BertLMPredictionHead.decoder = nn.Linear(hidden, vocab) followed by CrossEntropyLoss, xbert.py:822, 1653-1661; there
 * the [R, V] logits are materialised in fp16 and up-cast for the loss).  X [R, Hd] bf16 = transformed masked rows,
 * E [Vp, Hd] bf16 = word embeddings padded to Vp % 64 == 0 rows, bias [Vp], labels [R] (< 0: ignored), V = vocabulary.
 *   x2_mlm_ce_fwd : part[R][Vp/64][2] = (max, sum exp(z - max)) of every 64-column chunk of z = X.E^T + bias (columns
 *                   < V only), zlab[r] = z[r][label[r]]
 *   x2_ce_combine : lse[r] from the chunks of row r, loss_row[r] = lse - zlab (0 for ignored rows),
 *                   out2 = {mean loss, counted rows}
 *   x2_mlm_ce_bwd : dl[R][ldd] bf16 = (exp(z - lse[r]) - [c == label]) * gscale * g[0] / stat[1], z recomputed by the same
 *                   GEMM; ignored rows and columns >= V are written as 0 */
int x2_mlm_ce_fwd(const void* X, const void* E, const float* bias, const long* labels, int R, int Vp, int V, int Hd,
                  int ldx, int lde, float* part, float* zlab, void* stream);
int x2_ce_combine(const float* part, int chunks, const float* zlab, const long* labels, int R, float* lse, float* loss_row,
                  float* out2, void* stream);
int x2_mlm_ce_bwd(const void* X, const void* E, const float* bias, const long* labels, const float* lse, const float* g,
                  const float* stat, float gscale, int R, int Vp, int V, int Hd, int ldx, int lde, void* dl_bf16, long ldd,
                  void* stream);
/* MLM text masking of a padded batch on the device (csrc/masking.hip): dataset/pretrain_dataset.py:59-130 (TextMaskingGenerator.__call__) and
 * :242-275 (ImageTextJsonDataset.preprocess: masked_ids, padding) - host work of the reference's data-loader workers.
 *   text_ids, text_atts [B, L] int64 (captions left-aligned, atts = 1 on the caption, first token = cls_id); is_subword [vocab] bytes, 1 where the
 *   token text starts with '##' (WordPiece continuation); outputs int64: text_ids_masked [B, L] (pad_id beyond the caption), masked_pos [B, max_masks]
 *   (pad 0), masked_ids [B, max_masks] (original ids, pad pad_mask = -100).  2 <= L <= 512.
 *   Random draws come from a stream of 32-bit words per caption, consumed in the reference's draw order (rand() < p: word < ceil(p 2^32);
 *   randint(a, b): a + ((word (b - a + 1)) >> 32); shuffle: random.shuffle's loop with j = (word (i + 1)) >> 32): words != NULL: caption b reads
 *   words[b * words_ld + k] (injected, parity tests: at most 4 L + 64 are consumed); words == NULL: word k = hash(seed', b, k) with
 *   seed' = epoch ? hash(seed + 0x9E3779B1 * *epoch) : seed (a hipGraph-captured step increments *epoch per replay: new masks every step).
 *   The order of the reported positions is the iteration order of the CPython set the reference collects them in (restated in the kernel). */
int x2_mask_tokens(const long* text_ids, const long* text_atts, int B, int L, const unsigned char* is_subword, int vocab,
                   const unsigned* words, int words_ld, unsigned seed, const unsigned* epoch, double mask_prob, int max_masks,
                   double skipgram_prb, int skipgram_size, int mask_whole_word, long cls_id, long mask_id, long pad_id, long pad_mask,
                   long* text_ids_masked, long* masked_pos, long* masked_ids, void* stream);
/* hard negatives, xvlm.py:828-857: softmax(sim)+1e-5 with the diagonal (or same-group entries) zeroed, one
 * inverse-CDF draw per row from u[b] in [0,1); replaces 2*B torch.multinomial(...).item() host syncs */
int x2_sample_negatives(const float* sim, int n, const long* group, const float* u, int* out, void* stream);
/* additive key mask of BertModel (get_extended_attention_mask: neg = -10000; invert_attention_mask: -1e9; xbert.py:1105-1160):
 * out[s][l] = (1 - atts[s][l]) * neg, l < L; 0 in the pad columns L..Lp-1 (the attention kernels read [S][Lp], Lp % 64 == 0) */
int x2_additive_mask(const long* atts, float* out, int S, int L, int Lp, float neg, void* stream);

/* ---- captioning fine-tune (XVLMForMLMCaptioning): additive to ABI v14 - no existing signature or struct changes, x2_abi_version() stays 14 ----
 *   x2_attn_fwd_mask2d / x2_attn_bwd_mask2d : x2_attn_fwd / x2_attn_bwd for BERT self-attention with a per-sequence additive mask
 *       mask2d[B][Lq][mask2d_ld] fp32 read per (query, key) (x2_additive_mask2d builds it); Lq == Lk <= 128, B == Bkv, head_dim 64, H any;
 *       args->bias / biasT / mask / kv_idx / seq_off / dS must be NULL and dbg 0 (key padding is what the 2-D mask expresses); dropout and
 *       LSE / Delta as x2_attn_fwd / x2_attn_bwd; the backward takes phase 0 only and has no atomics
 *   x2_additive_mask2d : out[s][i][j] = (1 - m[s][i][j]) * neg (j < L), 0 for L <= j < Lp; m [S][L][L] int64
 *   x2_embed_fwd_pid / x2_embed_bwd_pid : x2_embed_fwd / _bwd with explicit position ids pids[R] (int64) instead of r % L:
 *       out[r] = word[ids[r]] + pos[pids[r]] + type0;  dword[ids[r]] += g[r], dpos[pids[r]] += g[r], dtype0 += g[r] (fixed order, no atomics;
 *       L = row period of the scratch totals, scratch of min(L, R) * D floats)
 *   x2_mlm_ls_fwd : x2_mlm_ce_fwd plus sumz[R][Vp/64] (sum of z over each chunk's valid columns) and zign[R] = z[r][ignore]
 *   x2_ls_combine : label-smoothed KL (q[label] = 1 - ls, q[c] = ls / (V - 2), q[ignore] = 0, q = 0 on rows whose label is ignore):
 *       lse[r], kl_row[r], out2 = {sum_r kl_row[r] * w[r] / (sum w + 1e-5), sum w}
 *   x2_mlm_ls_bwd : dl[R][ldd] bf16 = (sum(q) * softmax(z) - q) * gscale * g[0] * w[r] / (stat[1] + 1e-5), 0 on ignored rows and pad columns */
int x2_attn_fwd_mask2d(const X2AttnArgs* args, const float* mask2d, int mask2d_ld, void* stream);
int x2_attn_bwd_mask2d(const X2AttnArgs* args, const float* mask2d, int mask2d_ld, void* stream);
int x2_additive_mask2d(const long* m, float* out, int S, int L, int Lp, float neg, void* stream);
int x2_embed_fwd_pid(const long* ids, const long* pids, const float* word, const float* pos, const float* type0, float* out, int R, int D,
                     void* stream);
int x2_embed_bwd_pid(const long* ids, const long* pids, const float* g, float* dword, float* dpos, float* dtype0, int R, int L, int D,
                     float* scratch, void* stream);
int x2_mlm_ls_fwd(const void* X, const void* E, const float* bias, const long* labels, long ignore, int R, int Vp, int V, int Hd, int ldx,
                  int lde, float* part, float* sumz, float* zlab, float* zign, void* stream);
int x2_ls_combine(const float* part, const float* sumz, int chunks, const float* zlab, const float* zign, const long* labels, const float* w,
                  int R, int V, long ignore, float ls, float* lse, float* kl_row, float* out2, void* stream);
int x2_mlm_ls_bwd(const void* X, const void* E, const float* bias, const long* labels, const float* w, const float* lse, const float* g,
                  const float* stat, float gscale, float ls, long ignore, int R, int Vp, int V, int Hd, int ldx, int lde, void* dl_bf16,
                  long ldd, void* stream);
/* CSR "K/V batch -> query sequences using it" from kv[S] (values in [0, Bi)): off[Bi+1], order[S] (stable counting sort);
 * the seq_off / seq_ids tables of X2AttnArgs for rows that share an image's K/V (the 4-pass fusion batch) */
int x2_kv_csr(const int* kv, int S, int Bi, int* off, int* order, void* stream);
/* row tables of the 4B-row fusion batch the step runs instead of the reference's four fusion passes (models/model_pretrain.py:44-62,
 * xvlm.py:859-899): row q * B + b = (text b, image b) | (text b, image ineg[b]) | (text tneg[b], image b) | (masked text b, image b);
 * t_idx[r] = row of the 2B-row [clean ; masked] text batch, kv[r] = image, atts_out[r] = text mask, enc_out[r] = image mask.
 * with_match == 0: the masked rows only (ret_match_loss=False).  Replaces torch.arange / cat / index launches. */
int x2_tail_index(const int* ineg, const int* tneg, const long* text_atts /* [B][L] */, const long* image_atts /* [Bi][T] */, int B, int L,
                  int T, int with_match, int* t_idx, int* kv, long* atts_out /* [R][L] */, long* enc_out /* [R][T] */, void* stream);
/* timm drop_path of the BEiT blocks (beit2.py:205-207, rates linspace(0, 0.1, depth) beit2.py:314): per-row keep / (1 - rate[l])
 * factors out[depth][2 branches][B * T], one Bernoulli per (block, branch, sample) hashed from (seed [, *epoch]) */
int x2_droppath_rows(const float* rates, unsigned seed, const unsigned* epoch, int depth, int B, int T, float* out, void* stream);
/* video path, xvlm.py:627-645 ('avgpool'): forward out[Bc][T][D] = mean_f (x[Bc * F][T][D] + pos[F][D]) (pos may be NULL);
 * backward (bwd != 0): out = dx[Bc * F][T][D] = dy / F per frame, dpos[F][D] = column sums of dy / F (NULL: not wanted) */
int x2_frame_mean(const float* x, const float* pos, const float* dy, float* out, float* dpos, int Bc, int F, int T, int D, int bwd,
                  void* stream);
int x2_gelu_f32(const float* x, const float* dy, float* out, long n, void* stream);               /* nn.GELU, xvlm.py:167 */
int x2_colsum_f32(const float* x, float* out, int M, int N, void* stream);

/* ---- captioning inference (csrc/decode.hip), additive to ABI v14: one decode step of models/model_generation.py:139-328 ----
 * Self-attention of a step's n_new tokens per row over a per-row K/V cache.  qkv [S * n_new][qkv_ld >= 3 * Hd] bf16 (Hd = 64 * H), the
 * fused projection rows; cache [S][Lmax][2 * Hd] bf16 of this layer (K then V), indexed by ABSOLUTE position; hist = positions already
 * cached, the same for every row.  Writes the new tokens' K/V to cache slots hist .. hist + n_new - 1 and out [S * n_new][out_ld] bf16,
 * query j attending positions 0 .. hist + j (the tril mask sliced as attention_mask[:, start_pos:next_pos+1, :next_pos+1]).
 * n_new <= 16, hist + n_new <= Lmax <= 128, Lmax % 8 == 0.  One workgroup owns a (row, head): no query reads another's fresh K/V. */
int x2_attn_decode(const void* qkv, int qkv_ld, void* cache, void* out, int out_ld, int S, int H, int n_new, int hist, int Lmax, float scale,
                   void* stream);
/* dst[l][s][0:hist] = src[l][parent[s]][0:hist] over caches [layers][S][Lmax][row_elems] bf16, one launch for all layers (select_beam_items
 * and, with parent[s] = s / K, first_expand).  dst beyond hist is left alone; src and dst must not overlap (src == dst is refused). */
int x2_beam_gather(const void* src, void* dst, const int* parent, int layers, int S, int Lmax, int row_elems, int hist, void* stream);
/* per row of fp32 logits [S][ldv] (V valid columns, the rest never read): log_softmax; -10000 ADDED to every token seq[i + n - 1] with
 * seq[i .. i+n-2] equal to the row's last n - 1 ids (seq [S][Lseq] int32, seq_len ids so far, n = ngram; none when seq_len < n, seq NULL or
 * n == 0: get_dup_ngram_candidates with an empty forbid_ignore_set); column eos_id SET to -10000 when forbid_eos; then the K <= 8 largest
 * values and their columns, largest first, lowest column first among equal values.  logs (or NULL): the [S][V] penalised log-scores. */
int x2_logprob_topk(const float* logits, int ldv, int V, int S, const int* seq, int Lseq, int seq_len, int ngram, int eos_id, int forbid_eos,
                    int K, float* out_vals, int* out_ids, float* logs, void* stream);

/* ---- VQA inference: additive to ABI v14 (csrc/vqa.hip) - XVLMForVQA.rank_answer, models/model_generation.py:562-619.  No existing signature or
 * struct changes, x2_abi_version() stays 14.  Both selections order by value descending, the LOWER index first among equal values.
 *   x2_answer_topk : per question row of fp32 first-step logits [B][ldv] (V valid columns, the rest never read):
 *       logp[c] = z[first_tok[c]] - logsumexp(z) for the Na candidate answers (first_tok int32 [Na], values in [0, V) - a precondition; a value
 *       outside is not dereferenced and scores -inf), the k largest as vals [B][k] (LOG-probabilities) and their candidate indices ids [B][k].
 *       Refused without a launch: k outside 1..min(Na, 256), Na outside 1..65536.
 *   x2_vqa_candidates : rows s = b * k + j of the second decoder pass from answer_ids / answer_atts int64 [Na][La] and ids [B][k]:
 *       input_ids [S][La]; labels [S][La-1] = the next token, -100 where it is pad_token_id; kv_idx [S] = s / k;
 *       mask2d [S][La][mask2d_ld] = (1 - tril[i][j] * atts[s][j]) * -10000 for j < La, 0 for La <= j < mask2d_ld (= La rounded up to 64): the
 *       layout x2_attn_fwd_mask2d reads.  2 <= La <= 128.  An id outside [0, Na) yields an all-padding row.
 *   x2_vqa_rerank : loss_rows [S][T] (T = La - 1 <= 127, x2_ce_combine's loss_row: 0 on ignored rows), vals / ids of the first stage:
 *       scores[b][j] = vals[b][j] - (sum of loss_rows[b * k + j][0..T-1], added in index order); softmax over the k <= 256 scores of a question;
 *       topk_probs [B][k] and topk_ids [B][k] (ids gathered) sorted by score, scores [B][k] unsorted. */
int x2_answer_topk(const float* logits, int ldv, int V, int B, const int* first_tok, int Na, int K, float* out_vals, int* out_ids, void* stream);
int x2_vqa_candidates(const long* answer_ids, const long* answer_atts, const int* ids, int Na, int La, int B, int K, long pad_token_id,
                      long* input_ids, long* labels, int* kv_idx, float* mask2d, int mask2d_ld, void* stream);
int x2_vqa_rerank(const float* loss_rows, int T, const float* vals, const int* ids, int B, int K, float* topk_probs, int* topk_ids, float* scores,
                  void* stream);

/* ---- VQA fine-tune: additive to ABI v14 (csrc/vqa.hip, csrc/gemm.hip) - XVLMForVQA.forward(train=True), models/model_generation.py:517-550:
 * loss = sum_s weights[s] * (sum_t CE(logits[s][t], answer_ids[s][t+1])) / B.  No existing signature or struct changes, x2_abi_version() stays 14.
 *   x2_vqa_train_rows : the S answer rows of a batch of B questions; rows offs[b] .. offs[b+1]-1 belong to question b (offs int32 [B+1], the
 *       exclusive prefix sum of k, read on the device).  kv_idx [S] = that b; labels [S][La-1] = the next token, -100 where it is pad_token_id;
 *       mask2d as x2_vqa_candidates; c [S] = weights[s] / B.  Rows s >= offs[B] are padding: labels all -100, c = 0, kv_idx = B - 1 (the last
 *       question); their mask follows their answer_atts like any row's.  2 <= La <= 128.  One writer per element, no atomics.
 *   x2_seq_loss_combine : second stage of x2_mlm_ce_fwd over rows r = s * T + t (T = La - 1 <= 127): lse [S*T] (x2_ce_combine's bits),
 *       loss_seq [S] = sum_t (lse - zlab), 0 where labels[r] < 0, added in index order; with c [S] (c and total come together) total [1] =
 *       sum_s c[s] * loss_seq[s], added in a fixed order by one workgroup.
 *   x2_mlm_seq_bwd : dl [R][ldd] bf16 = (softmax(z[r]) - onehot(labels[r])) * (c[r / T] * g[0]), z recomputed as x2_mlm_ce_bwd does; exact
 *       zeros on rows with a negative label, on every row of a sequence whose c[s] * g[0] is 0, and in columns V .. Vp-1.  R % T == 0. */
int x2_vqa_train_rows(const int* offs, const long* answer_ids, const long* answer_atts, const float* weights, int B, int S, int La,
                      long pad_token_id, int* kv_idx, long* labels, float* mask2d, int mask2d_ld, float* c, void* stream);
int x2_seq_loss_combine(const float* part, int chunks, const float* zlab, const long* labels, int S, int T, const float* c, float* lse,
                        float* loss_seq, float* total, void* stream);
int x2_mlm_seq_bwd(const void* X, const void* E, const float* bias, const long* labels, const float* c, const float* lse, const float* g, int T,
                   int R, int Vp, int V, int Hd, int ldx, int lde, void* dl_bf16, long ldd, void* stream);

/* ---- visual grounding: additive to ABI v14 (csrc/grounding.hip) - XVLMForGrounding (models/model_grounding.py), the box tail of
 * XVLMBase.get_bbox_loss + box_ops.py (xvlm.py:927-957) and grounding_eval_bbox / computeIoU (dataset/utils.py:363-453).  No existing signature
 * or struct changes, x2_abi_version() stays 14.  All tensors fp32 (hit: int32), rows of four floats 16-byte aligned (size: 8-byte).
 *   x2_bbox_loss_fwd : coord[B][4] = sigmoid(logits); per row the L1 sum over the four coordinates and 1 - GIoU of the matched pair, both boxes
 *       through cx +- w / 2; degenerate flag = some row of either box set has x2 < x1 or y2 < y1 (rows with keep == 0 count): then every row's
 *       GIoU term is 0 (xvlm.py:943-946, decided on the device).  stat[4] = {sum keep * l1 / num, sum keep * giou / num, flag (0 / 1), num},
 *       num = sum keep, or B when keep == NULL (num == 0 divides by zero, as the reference does).  One workgroup, fixed summation order, no
 *       atomics: two runs give the same bits.  1 <= B <= 1048576.
 *   x2_bbox_loss_bwd : dlogits[B][4] = (g_coord + g_bbox * keep / num * sign(coord - target) + g_giou * keep / num * d(1 - GIoU)/dcoord)
 *       * coord * (1 - coord); g_bbox / g_giou device scalars (NULL = 0), g_coord [B][4] or NULL; coord and stat are the forward's.  Under the
 *       flag no GIoU expression is evaluated (no 0 / 0 of an unselected branch).  Ties: sign(0) = 0; max / min of equal edges send the gradient to
 *       the target's edge (the prediction gets 0); the clamp at exactly 0 passes 0.  1 <= B <= 1048576.
 *   x2_grounding_iou : per sample, in fp32 and the reference's order: x, w of coord (normalised cxcywh) times size[i][0] (width), y, h times
 *       size[i][1] (height), centre moved to the corner; then computeIoU against ref_box (pixel xywh): inclusive -1 / +1 pixel edges, strict <
 *       for "overlaps", union from w * h; hit = iou >= 0.5.  1 <= N <= 16777216.
 * A B or N outside its range returns -1 and names the entry point in x2_last_error() without launching. */
int x2_bbox_loss_fwd(const float* logits, const float* target, const float* keep, int B, float* coord, float* stat, void* stream);
int x2_bbox_loss_bwd(const float* coord, const float* target, const float* keep, const float* stat, const float* g_bbox, const float* g_giou,
                     const float* g_coord, int B, float* dlogits, void* stream);
int x2_grounding_iou(const float* coord, const float* ref_box, const float* size, int N, float* iou, int* hit, void* stream);

/* ---- classification fine-tunes: additive to ABI v14 (csrc/classify.hip) - XVLMForNLVR (models/model_classification.py, NLVR.py): the tail of a
 * build_mlp head behind its first Linear, LayerNorm -> erf-GELU -> Linear(H -> C) -> F.cross_entropy(ignore_index=-100), and the accuracy of the
 * evaluation loop.  No existing signature or struct changes, x2_abi_version() stays 14.  All tensors fp32 except labels (int64), pred (int32) and
 * counts (int64).  1 <= R <= 65536; 4 <= H <= 16384, H % 4 == 0; leading dimensions >= H and % 4 == 0; h, gamma, beta, w, dh 16-byte aligned (rows
 * are read as float4); 2 <= C <= 16.  No atomics, fixed summation orders: two runs give the same bits.
 *   x2_cls_tail_fwd : h [R][ldh] (pre-LayerNorm), w [C][H], labels [R] in [0, C) or -100 (any value outside [0, C) is treated as ignored), or
 *       NULL.  Launch one, a workgroup per row: mean and biased variance in two passes, rstd = 1 / sqrt(var + eps), y = xhat * gamma + beta,
 *       gelu(y), logits [R][C] = gelu(y) @ w^T + bias, rowstat [R][2] = {mean, rstd}, with labels nll [R] = logsumexp - logit[label] (0 on an
 *       ignored row).  Launch two (labels only), one workgroup: stat [2] = {sum nll / n_valid, n_valid}; n_valid == 0 gives NaN, as torch does.
 *       Without labels nll and stat are not touched.
 *   x2_cls_tail_bwd : dlogits = g_logits + g_loss / n_valid * (softmax(logits) - onehot) on valid rows, g_logits alone on ignored ones; g_loss a
 *       device scalar (NULL = 0), g_logits [R][C] (NULL = 0); rowstat, logits and stat are the forward's.  Launch one, a workgroup per row:
 *       dh [R][lddh] through dlogits @ w, gelu'(y) = Phi(y) + y phi(y) and LayerNorm's backward.  Launch two, one thread per column walking rows
 *       0..R-1 in order: dgamma [H], dbeta [H], dw [C][H] and dbias [C], recomputing xhat, y and gelu(y) from h and rowstat.
 *   x2_cls_accuracy : one workgroup; pred [R] = the lowest index of the row's maximum (strict >: torch's max(1) tie rule), counts [2] += {rows with
 *       pred == label, R}: the caller zeroes counts once, launches on one stream accumulate.  NaN logits are outside the contract.
 * An argument outside its range returns -1 and names the entry point in x2_last_error() without launching. */
int x2_cls_tail_fwd(const float* h, int ldh, const float* gamma, const float* beta, const float* w, const float* bias, const long* labels, int R,
                    int H, int C, float eps, float* logits, float* rowstat, float* nll, float* stat, void* stream);
int x2_cls_tail_bwd(const float* h, int ldh, const float* gamma, const float* beta, const float* w, const float* rowstat, const float* logits,
                    const long* labels, const float* stat, const float* g_loss, const float* g_logits, int R, int H, int C, float* dh, int lddh,
                    float* dgamma, float* dbeta, float* dw, float* dbias, void* stream);
int x2_cls_accuracy(const float* logits, const long* labels, int R, int C, int* pred, long* counts, void* stream);

/* ---- wide-label classification head: additive to ABI v14 (csrc/classify_wide.hip) - XVLMForClassification and XVLMForVQAClassification
 * (models/model_classification.py): the row work around the logits GEMM of a build_mlp head with more than 16 labels.  The logits themselves are
 * x2_gemm_nt(act, Wp, bias_p) -> fp32 [R][Cp], Cp = C rounded up to 64 with zero weight rows and zero bias: the pad columns hold 0, and every
 * entry point here reads columns [0, C) only.  No existing signature changes, x2_abi_version() stays 14.  fp32 tensors except act and dl (bf16,
 * round to nearest even), offs (int32), targets / labels / counts (int64), pred / hit (int32).  1 <= R <= 65536; 4 <= H <= 16384, H % 4 == 0;
 * 2 <= C <= 2^20; ldh, lda, ldd, lddh >= H and % 4 == 0 with h, gamma, beta, dact, dh 16-byte and act 8-byte aligned; ldl, ldt, ldg >= C (any value:
 * rows are read as float4 when the base is 16-byte aligned and the leading dimension % 4 == 0, as scalars otherwise, with the same arithmetic);
 * Cp >= C, Cp % 4 == 0, lddl >= Cp and % 4 == 0, dl 8-byte aligned.  No atomics; summation orders are fixed (file header): two runs give the same
 * bits.
 *   x2_lngelu_fwd : one launch, a workgroup per row.  mean, biased variance as the mean of (x - mean)^2 in a second pass, rstd = 1 / sqrt(var + eps),
 *       act [R][lda] = bf16(erf-GELU(xhat * gamma + beta)), rowstat [R][2] = {mean, rstd}.  Columns [H, lda) of act are not written.
 *   x2_lngelu_bwd : launch one, a workgroup per row: dy = dact * gelu'(y), LayerNorm's backward -> dh [R][lddh].  Launch two, one thread per column
 *       walking rows 0..R-1 in order: dgamma [H], dbeta [H].  xhat and y are recomputed from h and rowstat.
 *   x2_soft_ce_fwd : row r owns the entries offs[r] .. offs[r+1]-1 of targets [T] and weights [T] (NULL = 1); offs [R+1] is required.  Launch one, a
 *       workgroup per row: lse [R] over columns [0, C) (max, then sum of exp(z - max)), rowloss [R] = sum_j w_j (lse - z[t_j]) in index order; an
 *       entry with t_j outside [0, C) (ignore_index's -100) is skipped, a row without entries gives 0.  Launch two, one workgroup: stat [2] =
 *       {sum_r rowloss / denom, denom}; denom_mode 0: denom = R (the loss.sum() / image.size(0) of XVLMForVQAClassification), 1: the number of
 *       non-skipped entries (with offs = 0..R and NULL weights F.cross_entropy(ignore_index=-100); no such entry gives 0 / 0 = NaN, as torch does).
 *       targets == NULL: no loss is asked for, only lse is written and rowloss / stat are not touched.
 *   x2_kl_ce_fwd : lse, lse_t [R] of the logits and the teacher [R][ldt], rowloss [R] = sum_c p_c ((t_c - lse_t) - (z_c - lse)) with
 *       p_c = exp(t_c - lse_t) (p_c == 0 contributes 0), stat = {sum_r rowloss / R, R}: nn.KLDivLoss('none')(log_softmax(z), softmax(t)).sum() / R.
 *   x2_soft_ce_bwd : one launch, a workgroup per row: dl [R][lddl] = bf16(g_logits[r][c] + g_loss / denom * (Wr softmax(z)[c] - sum_{j: t_j = c} w_j))
 *       for c < C and 0 for C <= c < Cp; Wr = the sum of the row's non-skipped weights, denom = the forward's stat[1]; duplicates of a column add in
 *       index order (the entries are staged in LDS 256 at a time: no maximum k).  g_loss: device scalar; g_logits [R][ldg]; either may be NULL
 *       (= 0); with g_loss NULL the loss's tensors are not read and may be NULL.
 *   x2_kl_ce_bwd : the same for the KL loss: dl = bf16(g_logits + g_loss / R * (softmax(z) - p)).
 *   x2_cls_accuracy_rows : launch one, a workgroup per row: pred [R] = the lowest index of the maximum over columns [0, C) (prediction.max(1)'s
 *       tie rule), hit [R] = (pred == label); a label of -100 is a miss.  Launch two, one workgroup: counts [2] += {sum hit, R} by a plain
 *       read-modify-write (the caller zeroes counts once; launches on one stream accumulate).  NaN logits are outside the contract.
 * An argument outside its range returns -1 and names the entry point in x2_last_error() without launching. */
int x2_lngelu_fwd(const float* h, int ldh, const float* gamma, const float* beta, int R, int H, float eps, void* act, int lda, float* rowstat,
                  void* stream);
int x2_lngelu_bwd(const float* dact, int ldd, const float* h, int ldh, const float* gamma, const float* beta, const float* rowstat, int R, int H,
                  float* dh, int lddh, float* dgamma, float* dbeta, void* stream);
int x2_soft_ce_fwd(const float* logits, int ldl, int R, int C, const int* offs, const long* targets, const float* weights, int denom_mode, float* lse,
                   float* rowloss, float* stat, void* stream);
int x2_kl_ce_fwd(const float* logits, int ldl, const float* teacher, int ldt, int R, int C, float* lse, float* lse_t, float* rowloss, float* stat,
                 void* stream);
int x2_soft_ce_bwd(const float* logits, int ldl, int R, int C, const int* offs, const long* targets, const float* weights, const float* lse,
                   const float* stat, const float* g_loss, const float* g_logits, int ldg, void* dl, int lddl, int Cp, void* stream);
int x2_kl_ce_bwd(const float* logits, int ldl, const float* teacher, int ldt, int R, int C, const float* lse, const float* lse_t, const float* g_loss,
                 const float* g_logits, int ldg, void* dl, int lddl, int Cp, void* stream);
int x2_cls_accuracy_rows(const float* logits, int ldl, const long* labels, int R, int C, int* pred, int* hit, long* counts, void* stream);

/* ---- image-text retrieval fine-tune and evaluation: additive to ABI v14 (csrc/retrieval.hip) - XVLMForRetrieval (models/model_retrieval.py), the
 * soft-label branch of XVLMBase.get_contrastive_loss (xvlm.py:805-826), get_hard_negatives with `idx` (xvlm.py:828-857) and itm_eval
 * (Retrieval.py:171-215).  No existing signature or struct changes, x2_abi_version() stays 14.  fp32 tensors except idx / group / counts (int64) and
 * out / no_negative / gt_offs / gt_ids / ranks (int32).  Plain fp32 arithmetic with libm expf / logf, no atomics, one writer per output element,
 * fixed summation orders (file header): two runs give the same bits.
 *   x2_itc_soft_fwd : logits [N][ld] = the similarities already divided by temp, idx [N] the (all-gathered) group ids, pos_ij = (idx[i] == idx[j]).
 *       2 <= N <= 1024 (x2_sample_negatives' bound), ld >= N; columns [N, ld) are never read.  Launch one, N + ceil(N / 64) workgroups: per row i
 *       cnt_i = sum_j pos_ij, lse_i = max + log sum exp(z_ij - max), li_i = lse_i - (sum_j pos_ij z_ij) / cnt_i; per column j the same over z_.j
 *       (lt_j), the matrix read row-major by workgroups of 64 adjacent columns - no transpose, no strided walk.  rowstat / colstat [N][3] =
 *       {max, log sum exp(z - max), cnt} (lse = the sum of the first two, kept apart: one fp32 lse near 1000, at temp = 0.001, is too coarse for
 *       the backward's exp(z - lse)), loss_rows [2N] = {li, lt}.  Launch two, one workgroup: out[0] = (sum_i li_i / N + sum_j lt_j / N) / 2.
 *   x2_itc_soft_bwd : one launch, a workgroup per row: dlogits[i][j] = g[0] / (2N) * ((exp(z_ij - lse_i) - pos_ij / cnt_i) + (exp(z_ij - lse^col_j)
 *       - pos_ij / cnt_j)) for j < N; g a device scalar; rowstat / colstat are the forward's; ldd >= N, columns [N, ldd) are not written.
 *   x2_sample_negatives_checked : x2_sample_negatives - the same device function, the same arithmetic and tie handling, bit for bit - plus
 *       no_negative [n] = 1 where every candidate of row b is masked (all rows share its group) or none has a positive weight (a row of NaN
 *       similarities), else 0; out[b] = b on such a row.
 *   x2_retrieval_ranks : scores [R][ld], N columns (1 <= N <= 65536, ld >= N, R >= 1); the ground-truth columns of query r are
 *       gt_ids[gt_offs[r] .. gt_offs[r+1]) (CSR; the caller guarantees 0 <= gt_offs[r] <= gt_offs[r+1] <= the length of gt_ids); an id outside
 *       [0, N) is skipped and never dereferenced.  Launch one, a workgroup per row: ranks[r] = min over its ground truths j of
 *       #{c < N : s[c] > s[j]} - STRICTLY greater: the tie rule.  np.argsort(...)[::-1] has no defined order among equal scores, so this is the
 *       reference's rank whenever the ground truth's score is not tied; with rerank_scores' -100 fill a ground truth outside the top k_test gets
 *       rank k_test here and some rank >= k_test there, so R@1 / R@5 / R@10 agree for k_test >= 10.  A row without a ground truth gets INT_MAX
 *       (the reference's 1e20): in no recall, but in the denominator.  Launch two, one workgroup: counts [4] += {#ranks < 1, #ranks < 5,
 *       #ranks < 10, R} by a plain read-modify-write (the caller zeroes counts once; launches on one stream accumulate).  NaN scores are outside
 *       the contract.
 * An argument outside its range returns -1 and names the entry point in x2_last_error() without launching. */
int x2_itc_soft_fwd(const float* logits, int ld, const long* idx, int N, float* rowstat, float* colstat, float* loss_rows, float* out, void* stream);
int x2_itc_soft_bwd(const float* logits, int ld, const long* idx, int N, const float* rowstat, const float* colstat, const float* g, float* dlogits,
                    int ldd, void* stream);
int x2_sample_negatives_checked(const float* sim, int n, const long* group, const float* u, int* out, int* no_negative, void* stream);
int x2_retrieval_ranks(const float* scores, int ld, int R, int N, const int* gt_offs, const int* gt_ids, int* ranks, long* counts, void* stream);

/* ---- optimizer (csrc/optim.hip) -- "next" row of the scope table ------------------------------------------
 * optim.py:26-104 (transformers==4.12.5 AdamW, eps 1e-8, betas (0.9,0.98), correct_bias) and the global-norm clip of
 * accelerators/apex_ddp_accelerator.py:99-102, as two multi-tensor launches.  table: ntensors records
 * {float* p; const float* g (NULL = no gradient); float* m; float* v; long n; int group; int blk0; float stepscale; int pad}
 * in device memory, blk0 = prefix sum of ceil(n / 16384); nblocks = total; stepscale = sqrt(1 - b2^t) / (1 - b1^t) with t the
 * tensor's own step count (HF AdamW keeps state["step"] per parameter).  out2 = {total norm, min(1, max_norm / (norm + 1e-6))}. */
int x2_grad_norm(const void* table, int ntensors, int nblocks, float max_norm, float* partial, float* out2, void* stream);
int x2_adamw_multi(const void* table, int ntensors, int nblocks, const float* lr, const float* wd, int ngroups, float b1,
                   float b2, float eps, const float* clip2 /* out2 of x2_grad_norm or NULL */, void* stream);

/* ---- data-parallel communication (csrc/comm.hip) -----------------------------------------------------------
 * RCCL over xGMI behind the C ABI, for hosts that are not PyTorch (the Python host may use either these or
 * torch.distributed's "nccl" backend, which is the same RCCL).  Replaces accelerators/apex_ddp_accelerator.py:57-66
 * (NCCL init), :70-77 (per-tensor broadcast), :80-97 (apex DDP: flat all-reduce + average) and models/xvlm.py:140-160
 * (ITC all_gather; its backward keeps the local slice and needs no collective).  One communicator per process, one
 * process per GPU.  librccl.so.1 is loaded on first use (the library itself has no link-time RCCL dependency).
 * Every collective is enqueued on `stream` (the caller's communication stream) and, if done_event (a hipEvent_t) is
 * non-NULL, records it behind the collective.  dtype: 0 = fp32, 1 = bf16. */
int x2_comm_unique_id(void* out128);                                     /* rank 0; share the 128 bytes out of band */
int x2_comm_init(const void* id128, int rank, int world, void** comm_out);  /* collective; current HIP device = this rank's GPU */
int x2_comm_info(void* comm, int* rank, int* world);
int x2_comm_allreduce_bucket(void* comm, void* buf, long count, int dtype, int average, void* done_event, void* stream);
int x2_comm_allgather(void* comm, const void* send, void* recv, long count_per_rank, int dtype, void* done_event, void* stream);
int x2_comm_broadcast(void* comm, void* buf, long count, int dtype, int root, void* done_event, void* stream);
int x2_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif
