"""Visual grounding fine-tune and evaluation on the MI355X stages (models/model_grounding.py, Grounding_bbox.py, dataset/utils.py:363-453).

  XVLMForGrounding      forward(image, text_ids, text_atts, target_bbox=None): the predicted box (normalised cxcywh), with a target also the
                        L1 and GIoU losses of XVLMBase.get_bbox_loss - here the box tail is two launches (ops.bbox_loss over
                        kernels.bbox_loss_fwd / _bwd) and the reference's degenerate-box early-out is a device flag, so the step has no host
                        round trip and replays as a hipGraph (graph.GraphedStep)
  grounding_iou         the pixel-space IoU of a whole evaluation set against its reference boxes in one launch (kernels.grounding_iou)
  grounding_eval_bbox   the reference's accuracies from it: per RefCOCO split, or the single VLUE score

Looking reference boxes and image sizes up (the REFER toolkit, a VLUE JSON file) stays with the caller: these functions take tensors.
"""
import torch

from . import checkpoint, ops
from . import kernels as K
from .xvlm import XVLMBase

SPLITS = ("val", "testA", "testB")


class XVLMForGrounding(XVLMBase):
    def __init__(self, config):
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=False, use_matching_loss=False,
                         use_mlm_loss=False, use_bbox_loss=True)
        self.init_params = []

    def load_pretrained(self, ckpt_rpath, config, load_bbox_pretrain=False, is_eval=False):
        """The checkpoint through checkpoint.load_pretrained with the text keys' `bert.` infix removed (this model's text encoder is the
        bare BertModel), loaded non-strictly; missing vision_encoder keys (the index buffers) are not printed.  load_bbox_pretrain is only
        reported, as in the reference.  Returns the load_state_dict result."""
        print("### load_bbox_pretrain, ", load_bbox_pretrain)
        state_dict = checkpoint.load_pretrained(self, ckpt_rpath, config, is_eval=is_eval, load_text=True)
        msg = self.load_state_dict(state_dict, strict=False)
        print("load checkpoint from %s" % ckpt_rpath)
        print("missing_keys: ", [p for p in msg.missing_keys if "vision_encoder" not in p])
        print("unexpected_keys: ", msg.unexpected_keys)
        return msg

    def forward(self, image, text_ids, text_atts, target_bbox=None):
        ops.require_hip(image, "XVLMForGrounding.forward")
        image_embeds, _ = self.get_vision_embeds(image)
        text_embeds = self.get_text_embeds(text_ids, text_atts)
        if target_bbox is None:
            return self.predict_bbox(image_embeds, text_embeds, text_atts)
        # predict_bbox up to the head's logits (all-ones image mask, the fusion CLS row); the sigmoid is the loss kernel's first step
        ones = torch.ones(image_embeds.shape[:2], device=image_embeds.device)
        cls = self.get_cross_embeds(image_embeds, ones, text_embeds=text_embeds, text_atts=text_atts)[:, 0, :]
        return ops.bbox_loss(ops.mlp_head(self.bbox_head, cls), target_bbox)


def _as_f32_rows(t, cols, device=None):
    t = torch.as_tensor(t, dtype=torch.float32, device=device).reshape(-1, cols)
    return t.contiguous()


def grounding_iou(pred, ref_box, size):
    """pred [N, 4] normalised cxcywh (a HIP tensor: the model's output_coord rows), ref_box [N, 4] pixel xywh, size [N, 2] (width, height)
    -> (iou fp32 [N], hit bool [N] = iou >= 0.5), grounding_eval_bbox's arithmetic and computeIoU's convention, on the device."""
    ops.require_hip(pred, "grounding_iou")
    pred = _as_f32_rows(pred.detach(), 4)
    iou, hit = K.grounding_iou(pred, _as_f32_rows(ref_box, 4, pred.device), _as_f32_rows(size, 2, pred.device))
    return iou, hit.bool()


def grounding_eval_bbox(pred, ref_box, size, split=None):
    """The reference's evaluation from tensors.  split: a list of N labels 'val' | 'testA' | 'testB' -> {'val_d', 'testA_d', 'testB_d'}
    (grounding_eval_bbox; a sample with another label is counted nowhere, an empty split divides by zero, both as in the reference);
    None -> {'score'} (grounding_eval_bbox_vlue).  One launch and one read-back for the whole set."""
    _, hit = grounding_iou(pred, ref_box, size)
    hit = hit.cpu()
    if split is None:
        result = {"score": int(hit.sum()) / hit.numel()}
    else:
        assert len(split) == hit.numel()
        result = {}
        for name in SPLITS:
            rows = torch.tensor([s == name for s in split], dtype=torch.bool)
            result[name + "_d"] = int((hit & rows).sum()) / int(rows.sum())
    for metric, acc in result.items():
        print(f"{metric}: {acc:.3f}")
    return result
