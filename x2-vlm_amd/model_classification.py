"""Classification fine-tunes and their evaluation on the MI355X stages (models/model_classification.py: XVLMForNLVR, XVLMForClassification,
XVLMForVQAClassification; NLVR.py, VQA_msrvtt.py, VQA_msvd.py).

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

  XVLMForClassification      forward(image, text_ids, text_atts, targets=None, train=True): the CLS row of the 12-layer text pass (image is None), of
                             the vision pass (text_ids is None; 5-D video batches go through the frame mean) or of the fusion pass, then cls_head.
                             Up to 16 labels the tail is ops.cls_tail, above that ops.cls_wide with one target per row and the mean over the
                             non-ignored rows (F.cross_entropy(ignore_index=-100)).  num_labels == 1 (the MSE regression) is not built.
  XVLMForVQAClassification   forward(image, text_ids, text_atts, targets=None, k=None, weights=None, train=True, answer_pred=None,
                             return_logits=False): row b owns k[b] of the T targets and weights, loss = sum_b sum_j w_j CE(prediction[b], t_j) / B
                             without the reference's repeat of the prediction rows; with answer_pred the KL divergence to softmax(answer_pred).
  ClassificationAccuracy     NLVRAccuracy for any number of labels (kernels.cls_accuracy_rows: a workgroup per row).
"""
import torch

from . import ops
from . import kernels as K
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
        ops.require_hip(image, "XVLMForNLVR.forward")
        x = self._pair_cls(image, text_ids, text_atts)
        prediction, loss = ops.cls_tail(self.cls_head, ops.head_first_linear(self.cls_head, x), targets if train else None)
        return loss if train else prediction


class XVLMForClassification(XVLMBase):
    """VQA_msrvtt.py / VQA_msvd.py (video QA as 1500- / 1000-way classification) and the single-tower classifiers."""

    def __init__(self, config):
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=False, use_matching_loss=False,
                         use_mlm_loss=False, use_bbox_loss=False)
        feature_dim = self.vision_width if config.get("task_name") == "imagenet" else self.text_width
        self.num_labels = config["num_labels"]
        self.cls_head = build_mlp(input_dim=feature_dim, output_dim=self.num_labels)

    def forward(self, image, text_ids, text_atts, targets=None, train=True):
        probe = text_ids if image is None else image
        ops.require_hip(probe, "XVLMForClassification.forward")
        if self.num_labels == 1:
            raise NotImplementedError("XVLMForClassification: the MSE regression head (num_labels == 1) is not built on the HIP path")
        if image is None:
            output_cls = self.get_text_embeds_12L(text_ids, text_atts)[:, 0, :]
        elif text_ids is None:
            image_embeds, _ = self.get_vision_embeds(image)
            output_cls = image_embeds[:, 0, :]
        else:
            image_embeds, image_atts = self.get_vision_embeds(image)
            output_cls = self.get_cross_embeds(image_embeds, image_atts, text_ids=text_ids, text_atts=text_atts)[:, 0, :]
        h = ops.head_first_linear(self.cls_head, output_cls)
        if self.num_labels <= 16:
            prediction, loss = ops.cls_tail(self.cls_head, h, targets if train else None)
        elif train:
            offs = torch.arange(h.shape[0] + 1, device=h.device, dtype=torch.int32)          # one target per row
            prediction, loss = ops.cls_wide(self.cls_head, h, targets=targets, offs=offs, denom_mode=1)
        else:
            prediction, loss = ops.cls_wide(self.cls_head, h)
        return loss if train else prediction


class XVLMForVQAClassification(XVLMBase):
    """VQA v2 over a closed answer set (3129 labels by convention): k-expanded weighted cross-entropy, KL distillation, return_logits."""

    def __init__(self, config):
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=False, use_matching_loss=False,
                         use_mlm_loss=False, use_bbox_loss=False)
        self.num_labels = config["num_labels"]
        self.cls_head = build_mlp(input_dim=self.text_width, output_dim=self.num_labels)
        self.init_params = ["cls_head." + n for n, _ in self.cls_head.named_parameters()]

    @staticmethod
    def _offsets(k, B, T, device):
        """int32 [B + 1]: the exclusive prefix sum of k.  A device tensor stays on the device (no synchronisation: the caller guarantees
        sum(k) <= T); a list or a host tensor is checked here."""
        if isinstance(k, torch.Tensor) and k.is_cuda:
            assert k.numel() == B, "k must hold one count per row"
            offs = torch.zeros(B + 1, device=device, dtype=torch.int32)
            offs[1:] = torch.cumsum(k.reshape(-1), 0)
            return offs
        ks = [int(n) for n in (k.tolist() if isinstance(k, torch.Tensor) else k)]
        if len(ks) != B or min(ks) < 0 or sum(ks) != T:
            raise ValueError("k must hold %d non-negative counts that sum to the %d targets (got %s)" % (B, T, ks))
        offs = [0]
        for n in ks:
            offs.append(offs[-1] + n)
        return torch.tensor(offs, dtype=torch.int32).to(device)

    def forward(self, image, text_ids, text_atts, targets=None, k=None, weights=None, train=True, answer_pred=None, return_logits=False):
        ops.require_hip(image, "XVLMForVQAClassification.forward")
        if self.num_labels <= 16:
            raise ValueError("XVLMForVQAClassification: num_labels=%d; the wide head serves more than 16 labels" % self.num_labels)
        image_embeds, image_atts = self.get_vision_embeds(image)
        output_cls = self.get_cross_embeds(image_embeds, image_atts, text_ids=text_ids, text_atts=text_atts)[:, 0, :]
        h = ops.head_first_linear(self.cls_head, output_cls)
        if not train:
            return ops.cls_wide(self.cls_head, h)[0]
        if answer_pred is not None:
            return ops.cls_wide(self.cls_head, h, teacher=answer_pred)[1]
        B = h.shape[0]
        assert image.size(0) == B
        targets = targets.to(h.device).view(-1)
        weights = torch.as_tensor(weights, dtype=torch.float32).to(h.device).view(-1)
        prediction, loss = ops.cls_wide(self.cls_head, h, targets=targets, offs=self._offsets(k, B, targets.shape[0], h.device), weights=weights,
                                        denom_mode=0)
        return (loss, prediction) if return_logits else loss


class NLVRAccuracy:
    """NLVR.py:88-96 without the per-batch host round trip: update() is one launch (kernels.cls_accuracy: the row argmax under max(1)'s tie rule,
    then counts += {correct, rows} on the device), result() reads the two counters back once.  correct / counted equals the reference's
    metric_logger global average sum(acc_b * n_b) / sum(n_b), and is formatted as NLVR.py:96 does."""

    who = "NLVRAccuracy.update"          # the name a refused host tensor is reported under
    strided_ok = False          # whether the kernel reads a column view of wider rows in place

    def __init__(self):
        self.counts = None

    def _launch(self, prediction, targets):
        return K.cls_accuracy(prediction, targets, self.counts)

    def update(self, prediction, targets):
        """prediction fp32 [B, C] (a HIP tensor: the model's train=False output), targets [B] -> pred_class int32 [B] (left on the device)"""
        ops.require_hip(prediction, self.who)
        if self.counts is None:
            self.counts = torch.zeros(2, dtype=torch.int64, device=prediction.device)
        targets = torch.as_tensor(targets, device=prediction.device).to(torch.int64).contiguous()
        prediction = prediction.detach().to(torch.float32)
        return self._launch(prediction if self.strided_ok and prediction.stride(1) == 1 else prediction.contiguous(), targets)

    def result(self):
        """{'acc': correct / counted} (the one read-back); printed as the reference prints its averaged stats"""
        correct, counted = self.counts.tolist()
        acc = correct / counted
        print("Averaged stats:", "acc: {:.4f}".format(acc))
        return {"acc": acc}

    def formatted(self):
        """the dict NLVR.py:96 returns: every value as '{:.4f}'"""
        return {k: "{:.4f}".format(v) for k, v in self.result().items()}


class ClassificationAccuracy(NLVRAccuracy):
    """NLVRAccuracy for any number of labels (VQA_msrvtt.py:88-96): update() is kernels.cls_accuracy_rows - a workgroup per row takes the lowest
    index of the row's maximum, a second launch adds {correct, rows} to the device counters; a target of -100 counts as a miss, as
    (targets == pred_class).sum() / targets.size(0) does.  result() / formatted() are NLVRAccuracy's."""

    who = "ClassificationAccuracy.update"
    strided_ok = True

    def _launch(self, prediction, targets):
        return K.cls_accuracy_rows(prediction, targets, self.counts)[0]
