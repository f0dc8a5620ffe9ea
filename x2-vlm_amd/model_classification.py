"""NLVR2 fine-tune and evaluation on the MI355X stages (models/model_classification.py: XVLMForNLVR; NLVR.py).

  XVLMForNLVR    forward(image, text_ids, text_atts, targets, train=True): image holds image0 stacked over image1 ([2B, ...], as NLVR.py builds
                 it).  One vision pass over the 2B images, one fusion pass over 2B text rows, the fusion CLS rows b and B + b side by side as
                 [B, 2W], cls_head's first Linear as ops.mlp_head runs it, and the rest of the head with the cross-entropy as ops.cls_tail (two
                 launches forward, two backward, no host round trip: the step replays as a hipGraph, graph.GraphedStep).
                 train=True -> the loss, train=False -> the logits [B, 2].
  NLVRAccuracy   the evaluation loop's accuracy without its per-batch .item(): update(prediction, targets) is one launch, result() one read-back.

The text rows.  The reference calls get_cross_embeds(text_ids=...) once per image, i.e. runs the text-only layers twice on the same ids.
  self.training: one 2B-row pass with ids and masks repeated - every row then draws its own dropout and DropPath masks, as the two calls do.
  otherwise:     the two calls repeat the text-only layers on identical inputs, so they run once on B rows (get_text_embeds) and the 2B fusion rows
                 read them through _fusion_cls with t_idx = [0..B, 0..B] and kv = [0..2B): row r attends to image r.
Per row both routes are the reference's arithmetic.  Tokenizer, data loader and the NLVR.py script stay with the caller.
"""
import torch

from . import ops
from . import kernels as K
from .model_generation import _HOST_PATH
from .xvlm import XVLMBase, build_mlp


class XVLMForNLVR(XVLMBase):
    """Follows VLMo: one classifier over the concatenated CLS rows of the two (image, text) pairs."""

    def __init__(self, config):
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=False, use_matching_loss=False,
                         use_mlm_loss=False, use_bbox_loss=False, config_text=None)
        self.cls_head = build_mlp(input_dim=self.text_width * 2, output_dim=2)
        self.init_params = ["cls_head." + n for n, _ in self.cls_head.named_parameters()]

    def _pair_cls(self, image, text_ids, text_atts):
        """[B, 2W]: the fusion CLS row of (image0[b], text[b]) beside that of (image1[b], text[b])"""
        B = text_ids.shape[0]
        assert image.shape[0] == 2 * B, "image must hold image0 stacked over image1: %d rows for %d texts" % (image.shape[0], B)
        image_embeds, image_atts = self.get_vision_embeds(image)
        if self.training:
            cls = self.get_cross_embeds(image_embeds, image_atts, text_ids=text_ids.repeat(2, 1), text_atts=text_atts.repeat(2, 1))[:, 0, :]
        else:
            text_embeds = self.get_text_embeds(text_ids, text_atts)
            ar = torch.arange(B, device=image.device, dtype=torch.int32)
            cls = self._fusion_cls(image_embeds, image_atts, text_embeds, text_atts, torch.cat([ar, ar]),
                                   torch.arange(2 * B, device=image.device, dtype=torch.int32))
        out = torch.cat((cls[:B], cls[B:]), dim=-1)
        assert out.shape[-1] == self.text_width * 2
        return out

    def forward(self, image, text_ids, text_atts, targets, train=True):
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise NotImplementedError(_HOST_PATH % "XVLMForNLVR.forward")
        x = self._pair_cls(image, text_ids, text_atts)
        head = self.cls_head
        w0 = head[0].weight
        if w0.shape[1] % 64 == 0 and w0.shape[0] % 8 == 0 and x.numel() % 4 == 0:          # ops.mlp_head's rule for its first Linear
            h = ops.LinearBf16Fn.apply(x, w0, head[0].bias)
        else:
            h = ops.linear(x, w0, head[0].bias)
        prediction, loss = ops.cls_tail(head, h, targets if train else None)
        return loss if train else prediction


class NLVRAccuracy:
    """NLVR.py:88-96 without the per-batch host round trip: update() is one launch (kernels.cls_accuracy: the row argmax under max(1)'s tie rule,
    then counts += {correct, rows} on the device), result() reads the two counters back once.  correct / counted equals the reference's
    metric_logger global average sum(acc_b * n_b) / sum(n_b), and is formatted as NLVR.py:96 does."""

    def __init__(self):
        self.counts = None

    def update(self, prediction, targets):
        """prediction fp32 [B, C] (a HIP tensor: the model's train=False output), targets [B] -> pred_class int32 [B] (left on the device)"""
        if not isinstance(prediction, torch.Tensor) or not prediction.is_cuda:
            raise NotImplementedError(_HOST_PATH % "NLVRAccuracy.update")
        if self.counts is None:
            self.counts = torch.zeros(2, dtype=torch.int64, device=prediction.device)
        targets = torch.as_tensor(targets, device=prediction.device).to(torch.int64).contiguous()
        return K.cls_accuracy(prediction.detach().to(torch.float32).contiguous(), targets, self.counts)

    def result(self):
        """{'acc': correct / counted} (the one read-back); printed as the reference prints its averaged stats"""
        correct, counted = self.counts.tolist()
        acc = correct / counted
        print("Averaged stats:", "acc: {:.4f}".format(acc))
        return {"acc": acc}

    def formatted(self):
        """the dict NLVR.py:96 returns: every value as '{:.4f}'"""
        return {k: "{:.4f}".format(v) for k, v in self.result().items()}
