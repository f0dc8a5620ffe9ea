// Visual grounding (XVLMForGrounding, models/model_grounding.py; Grounding_bbox.py): the box tail of the step and the evaluation.
//   x2_bbox_loss_fwd   sigmoid + L1 + (1 - GIoU) of matched pairs + the reference's degenerate-box early-out + both means, one launch
//   x2_bbox_loss_bwd   d(logits) of both losses and of a cotangent on the coordinates, one launch
//   x2_grounding_iou   grounding_eval_bbox / computeIoU (dataset/utils.py:363-453) of a whole evaluation set, one launch
// Replaces XVLMBase.get_bbox_loss + box_ops.py (xvlm.py:927-957): about forty elementwise ATen launches forward and as many in autograd's
// backward.  The work is a few flops per row, so this is plain VALU code; what it saves is launches and the host sync of the early-out.
// No atomics: the forward is ONE workgroup (the flag and the means need every row; thread t adds rows t, t + 256, ... in index order, then
// x2_rowblock.h's block sum), so two runs give the same bits.
//
// Sub-gradient choices of the backward (the reference's autograd splits a tie of max / min in half; tests stay away from ties):
//   |coord - target| at 0 -> 0 (as torch);  max(a, b) / min(a, b) at a == b -> the gradient goes to the TARGET's edge, the prediction gets 0;
//   clamp(x, min=0) at x == 0 -> 0 (torch passes 1; x == 0 means touching boxes, where the clamped value is 0 on both sides).
// Degenerate flag: some row of either box set has x2 < x1 or y2 < y1 after cx +- 0.5 * w (rows with keep == 0 count, as in the reference):
// every row's GIoU term is 0 and the backward does not evaluate a single GIoU expression, so no 0 / 0 of an unselected branch can reach
// dlogits.  Without the flag the arithmetic is the reference's: a pair of zero-area boxes (union 0) is NaN there and here.
#include "x2_rowblock.h"

#define GR_THREADS ROW_THREADS
#define GR_MAXB (1 << 20)          // forward: one workgroup walks every row (4096 rows per thread at the limit)
#define GR_MAXN (1 << 24)

#define GR_ALIGNED(p) ((((uintptr_t)(p)) & 15) == 0)          // rows of four floats are read and written as float4

struct GrBox { float x1, y1, x2, y2; };
__device__ __forceinline__ GrBox gr_xyxy(float cx, float cy, float w, float h) {          // box_ops.box_cxcywh_to_xyxy
  GrBox b;
  b.x1 = cx - 0.5f * w; b.y1 = cy - 0.5f * h; b.x2 = cx + 0.5f * w; b.y2 = cy + 0.5f * h;
  return b;
}
__device__ __forceinline__ bool gr_degenerate(const GrBox& b) { return b.x2 < b.x1 || b.y2 < b.y1; }

// 1 - generalized_box_iou of one pair (box_ops.py:24-57, the diagonal only)
__device__ __forceinline__ float gr_giou_loss(const GrBox& a, const GrBox& b) {
  const float area1 = (a.x2 - a.x1) * (a.y2 - a.y1), area2 = (b.x2 - b.x1) * (b.y2 - b.y1);
  const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.f), ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.f);
  const float inter = iw * ih, uni = area1 + area2 - inter;
  const float cw = fmaxf(fmaxf(a.x2, b.x2) - fminf(a.x1, b.x1), 0.f), ch = fmaxf(fmaxf(a.y2, b.y2) - fminf(a.y1, b.y1), 0.f);
  const float area = cw * ch;
  return 1.f - (inter / uni - (area - uni) / area);
}

__global__ __launch_bounds__(GR_THREADS) void bbox_loss_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                   const float* __restrict__ keep, int B, float* __restrict__ coord,
                                                                   float* __restrict__ stat) {
  __shared__ float red[GR_THREADS / 64];
  float l1 = 0.f, gi = 0.f, num = 0.f, bad = 0.f;
  for (int r = threadIdx.x; r < B; r += GR_THREADS) {
    const float4 z = reinterpret_cast<const float4*>(logits)[r], t = reinterpret_cast<const float4*>(target)[r];
    float4 c;
    c.x = 1.f / (1.f + expf(-z.x)); c.y = 1.f / (1.f + expf(-z.y)); c.z = 1.f / (1.f + expf(-z.z)); c.w = 1.f / (1.f + expf(-z.w));
    reinterpret_cast<float4*>(coord)[r] = c;
    const float k = keep ? keep[r] : 1.f;
    const GrBox a = gr_xyxy(c.x, c.y, c.z, c.w), b = gr_xyxy(t.x, t.y, t.z, t.w);
    const bool deg = gr_degenerate(a) || gr_degenerate(b);
    bad += deg ? 1.f : 0.f;
    l1 += ((fabsf(c.x - t.x) + fabsf(c.y - t.y)) + (fabsf(c.z - t.z) + fabsf(c.w - t.w))) * k;
    if (!deg) gi += gr_giou_loss(a, b) * k;          // a degenerate row sets the flag: its own term is never needed
    num += k;
  }
  l1 = row_block_sum(l1, red);
  gi = row_block_sum(gi, red);
  bad = row_block_sum(bad, red);
  num = keep ? row_block_sum(num, red) : (float)B;
  if (threadIdx.x == 0) {
    const bool flag = bad > 0.f;
    stat[0] = l1 / num;
    stat[1] = flag ? 0.f : gi / num;                  // a select, not a product: the unselected sum may hold anything
    stat[2] = flag ? 1.f : 0.f;
    stat[3] = num;
  }
}

extern "C" int x2_bbox_loss_fwd(const float* logits, const float* target, const float* keep, int B, float* coord, float* stat, void* stream) {
  X2_REQUIRE(logits && target && coord && stat, "x2_bbox_loss_fwd: null tensor");
  X2_REQUIRE(B >= 1 && B <= GR_MAXB, "x2_bbox_loss_fwd: B=%d must be in 1..%d", B, GR_MAXB);
  X2_REQUIRE(GR_ALIGNED(logits) && GR_ALIGNED(target) && GR_ALIGNED(coord), "x2_bbox_loss_fwd: [B][4] tensors must be 16-byte aligned");
  hipLaunchKernelGGL(bbox_loss_fwd_kernel, dim3(1), dim3(GR_THREADS), 0, (hipStream_t)stream, logits, target, keep, B, coord, stat);
  return x2_check_launch("x2_bbox_loss_fwd");
}

// One thread per row.  With L = 1 - GIoU = 2 - I / U - U / C (I intersection, U union, C enclosing area):
//   dL/dI = -1 / U - gU,  dL/dA1 = gU = I / U^2 - 1 / C,  dL/dC = U / C^2;  A1 = pw * ph, I = iw * ih, C = cw * ch.
__global__ __launch_bounds__(GR_THREADS) void bbox_loss_bwd_kernel(const float* __restrict__ coord, const float* __restrict__ target,
                                                                   const float* __restrict__ keep, const float* __restrict__ stat,
                                                                   const float* __restrict__ g_bbox, const float* __restrict__ g_giou,
                                                                   const float* __restrict__ g_coord, int B, float* __restrict__ dlogits) {
  const int r = blockIdx.x * GR_THREADS + threadIdx.x;
  if (r >= B) return;
  const float4 c = reinterpret_cast<const float4*>(coord)[r], t = reinterpret_cast<const float4*>(target)[r];
  const float scale = (keep ? keep[r] : 1.f) / stat[3];
  const float gb = g_bbox ? g_bbox[0] * scale : 0.f;
  float4 d = g_coord ? reinterpret_cast<const float4*>(g_coord)[r] : make_float4(0.f, 0.f, 0.f, 0.f);
  auto sgn = [](float v) -> float { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
  d.x += gb * sgn(c.x - t.x); d.y += gb * sgn(c.y - t.y); d.z += gb * sgn(c.z - t.z); d.w += gb * sgn(c.w - t.w);
  if (g_giou && stat[2] == 0.f) {                     // under the flag nothing below is evaluated
    const float gg = g_giou[0] * scale;
    const GrBox a = gr_xyxy(c.x, c.y, c.z, c.w), b = gr_xyxy(t.x, t.y, t.z, t.w);
    const float pw = a.x2 - a.x1, ph = a.y2 - a.y1;
    const float iwr = fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), ihr = fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1);
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float I = iw * ih, U = pw * ph + (b.x2 - b.x1) * (b.y2 - b.y1) - I;
    const float cwr = fmaxf(a.x2, b.x2) - fminf(a.x1, b.x1), chr = fmaxf(a.y2, b.y2) - fminf(a.y1, b.y1);
    const float cw = fmaxf(cwr, 0.f), ch = fmaxf(chr, 0.f);
    const float C = cw * ch;
    const float gU = I / (U * U) - 1.f / C, gI = -1.f / U - gU, gC = U / (C * C);
    const float g_iw = iwr > 0.f ? gI * ih : 0.f, g_ih = ihr > 0.f ? gI * iw : 0.f;
    const float g_cw = cwr > 0.f ? gC * ch : 0.f, g_ch = chr > 0.f ? gC * cw : 0.f;
    // edges of the prediction: x2 through min (intersection) and max (enclosure), x1 through max and min
    const float dx2 = gU * ph + (a.x2 < b.x2 ? g_iw : 0.f) + (a.x2 > b.x2 ? g_cw : 0.f);
    const float dx1 = -gU * ph - (a.x1 > b.x1 ? g_iw : 0.f) - (a.x1 < b.x1 ? g_cw : 0.f);
    const float dy2 = gU * pw + (a.y2 < b.y2 ? g_ih : 0.f) + (a.y2 > b.y2 ? g_ch : 0.f);
    const float dy1 = -gU * pw - (a.y1 > b.y1 ? g_ih : 0.f) - (a.y1 < b.y1 ? g_ch : 0.f);
    d.x += gg * (dx1 + dx2); d.y += gg * (dy1 + dy2); d.z += gg * 0.5f * (dx2 - dx1); d.w += gg * 0.5f * (dy2 - dy1);
  }
  d.x *= c.x * (1.f - c.x); d.y *= c.y * (1.f - c.y); d.z *= c.z * (1.f - c.z); d.w *= c.w * (1.f - c.w);
  reinterpret_cast<float4*>(dlogits)[r] = d;
}

extern "C" int x2_bbox_loss_bwd(const float* coord, const float* target, const float* keep, const float* stat, const float* g_bbox,
                                const float* g_giou, const float* g_coord, int B, float* dlogits, void* stream) {
  X2_REQUIRE(coord && target && stat && dlogits, "x2_bbox_loss_bwd: null tensor");
  X2_REQUIRE(B >= 1 && B <= GR_MAXB, "x2_bbox_loss_bwd: B=%d must be in 1..%d", B, GR_MAXB);
  X2_REQUIRE(GR_ALIGNED(coord) && GR_ALIGNED(target) && GR_ALIGNED(g_coord) && GR_ALIGNED(dlogits),
             "x2_bbox_loss_bwd: [B][4] tensors must be 16-byte aligned");
  hipLaunchKernelGGL(bbox_loss_bwd_kernel, dim3((B + GR_THREADS - 1) / GR_THREADS), dim3(GR_THREADS), 0, (hipStream_t)stream, coord, target, keep,
                     stat, g_bbox, g_giou, g_coord, B, dlogits);
  return x2_check_launch("x2_bbox_loss_bwd");
}

// One thread per sample, fp32 in the reference's order: x and w times the width, y and h times the height, centre to corner
// (coord[0] -= coord[2] / 2), then computeIoU(ref_box, coord) with its inclusive pixel edges.
__global__ __launch_bounds__(GR_THREADS) void grounding_iou_kernel(const float* __restrict__ coord, const float* __restrict__ ref_box,
                                                                   const float* __restrict__ size, int N, float* __restrict__ iou,
                                                                   int* __restrict__ hit) {
  const int i = blockIdx.x * GR_THREADS + threadIdx.x;
  if (i >= N) return;
  const float4 c = reinterpret_cast<const float4*>(coord)[i], rb = reinterpret_cast<const float4*>(ref_box)[i];
  const float2 wh = reinterpret_cast<const float2*>(size)[i];
  const float pw = c.z * wh.x, ph = c.w * wh.y;
  const float px = c.x * wh.x - pw / 2.f, py = c.y * wh.y - ph / 2.f;
  const float x1 = fmaxf(rb.x, px), y1 = fmaxf(rb.y, py);
  const float x2 = fminf(rb.x + rb.z - 1.f, px + pw - 1.f), y2 = fminf(rb.y + rb.w - 1.f, py + ph - 1.f);
  const float inter = (x1 < x2 && y1 < y2) ? (x2 - x1 + 1.f) * (y2 - y1 + 1.f) : 0.f;
  const float v = inter / (rb.z * rb.w + pw * ph - inter);
  iou[i] = v;
  hit[i] = v >= 0.5f ? 1 : 0;
}

extern "C" int x2_grounding_iou(const float* coord, const float* ref_box, const float* size, int N, float* iou, int* hit, void* stream) {
  X2_REQUIRE(coord && ref_box && size && iou && hit, "x2_grounding_iou: null tensor");
  X2_REQUIRE(N >= 1 && N <= GR_MAXN, "x2_grounding_iou: N=%d must be in 1..%d", N, GR_MAXN);
  X2_REQUIRE(GR_ALIGNED(coord) && GR_ALIGNED(ref_box) && (((uintptr_t)size) & 7) == 0, "x2_grounding_iou: coord / ref_box must be 16-byte, size 8-byte aligned");
  hipLaunchKernelGGL(grounding_iou_kernel, dim3((N + GR_THREADS - 1) / GR_THREADS), dim3(GR_THREADS), 0, (hipStream_t)stream, coord, ref_box, size,
                     N, iou, hit);
  return x2_check_launch("x2_grounding_iou");
}
