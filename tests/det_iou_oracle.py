"""The detection head's IoU loss family, IoU match cost and QualityFocalLoss as plain torch formulas (mmdet's, written out):
dtype-generic, gradients by autograd.  The reference of tests/test_det_iou_cpu.py and tests/test_det_iou_gpu.py (run in fp64
there), and the stand-ins that the CPU tests patch in for the three HIP-backed ops of the feature.

Notation: boxes p (prediction) and t (target) are xyxy; ov the clamped-at-0 intersection area, ap / at the areas, cw / ch the
clamped-at-0 extents of the enclosing box, rho2 = ((t.x1+t.x2)-(p.x1+p.x2))^2/4 + ((t.y1+t.y2)-(p.y1+p.y2))^2/4."""
import math

import torch
import torch.nn.functional as F


def xyxy(b):
    """cxcywh -> xyxy"""
    return torch.cat([b[..., :2] - 0.5 * b[..., 2:], b[..., :2] + 0.5 * b[..., 2:]], -1)


def _parts(p, t):
    ap = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
    at = (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])
    wh = (torch.min(p[..., 2:], t[..., 2:]) - torch.max(p[..., :2], t[..., :2])).clamp(min=0)
    ov = wh[..., 0] * wh[..., 1]
    ewh = (torch.max(p[..., 2:], t[..., 2:]) - torch.min(p[..., :2], t[..., :2])).clamp(min=0)
    return ov, ap, at, ewh[..., 0], ewh[..., 1]


def _rho2(p, t):
    return ((t[..., 0] + t[..., 2]) - (p[..., 0] + p[..., 2])) ** 2 / 4 + ((t[..., 1] + t[..., 3]) - (p[..., 1] + p[..., 3])) ** 2 / 4


def iou(p, t):
    """ov / max(union, 1e-6): IoUCost(iou_mode='iou'), IoULoss before its eps floor, QualityFocalLoss's score"""
    ov, ap, at, _, _ = _parts(p, t)
    return ov / (ap + at - ov).clamp(min=1e-6)


def giou(p, t, eps=1e-6):
    ov, ap, at, cw, ch = _parts(p, t)
    un = (ap + at - ov).clamp(min=eps)
    ea = (cw * ch).clamp(min=eps)
    return ov / un - (ea - un) / ea


def iou_loss(p, t, eps=1e-6, mode='log'):
    i = iou(p, t).clamp(min=eps)
    return {'linear': 1 - i, 'square': 1 - i ** 2, 'log': -i.log()}[mode]


def giou_loss(p, t, eps=1e-6):
    return 1 - giou(p, t, eps)


def diou(p, t, eps=1e-6):
    ov, ap, at, cw, ch = _parts(p, t)
    i = ov / (ap + at - ov + eps)
    c2 = cw ** 2 + ch ** 2 + eps
    return i - _rho2(p, t) / c2


def diou_loss(p, t, eps=1e-6):
    return 1 - diou(p, t, eps)


def ciou(p, t, eps=1e-6):
    ov, ap, at, cw, ch = _parts(p, t)
    i = ov / (ap + at - ov + eps)
    c2 = cw ** 2 + ch ** 2 + eps
    w1, h1 = p[..., 2] - p[..., 0], p[..., 3] - p[..., 1] + eps
    w2, h2 = t[..., 2] - t[..., 0], t[..., 3] - t[..., 1] + eps
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    with torch.no_grad():
        alpha = (i > 0.5).to(v.dtype) * v / (1 - i + v)
    return (i - (_rho2(p, t) / c2 + alpha * v)).clamp(min=-1.0, max=1.0)


def ciou_loss(p, t, eps=1e-6):
    return 1 - ciou(p, t, eps)


def box_loss(kind, p, t, eps=1e-6, mode='log'):
    """the per-pair loss of `kind` on xyxy boxes"""
    if kind == 'iou':
        return iou_loss(p, t, eps, mode)
    return {'giou': giou_loss, 'diou': diou_loss, 'ciou': ciou_loss}[kind](p, t, eps)


def box_loss_sums_kind(pred, target, weight, factors, kind='giou', eps=1e-6, mode='log'):
    """ops.box_loss_sums_kind: pred / target / weight (S,B,Q,4) cxcywh normalised, factors (B,4) -> (l1 (S,), iou loss (S,));
    the loss on the pixel boxes, weighted by the mean of the four box weights; a zero-weight row adds an exact 0."""
    f = factors.view(1, -1, 1, 4)
    l1 = ((pred - target).abs() * weight).flatten(1).sum(1)
    wm = weight.mean(-1)
    per = box_loss(kind, xyxy(pred) * f, xyxy(target) * f, eps, mode)
    per = torch.where(wm == 0, torch.zeros_like(per), per * wm)
    return l1, per.flatten(1).sum(1)


def match_cost_batched_kind(cls_score, bbox_pred, gt_bboxes, gt_labels, factors, w_cls, w_l1, w_iou, alpha, gamma, eps,
                            iou_mode='giou'):
    """ops.match_cost_batched_kind: cls (S,B,Q,C), box (S,B,Q,4), gt (B,G,4) xyxy pixels, labels (B,G), factors (B,4) -> (S,B,Q,G)"""
    S, B, Q, C = cls_score.shape
    G = gt_bboxes.shape[1]
    p = cls_score.sigmoid()
    neg = -(1 - p + eps).log() * (1 - alpha) * p.pow(gamma)
    pos = -(p + eps).log() * alpha * (1 - p).pow(gamma)
    c_cls = torch.gather(pos - neg, 3, gt_labels[None, :, None, :].expand(S, B, Q, G)) * w_cls
    gn = gt_bboxes / factors[:, None, :]
    gc = torch.cat([(gn[..., :2] + gn[..., 2:]) / 2, gn[..., 2:] - gn[..., :2]], -1)
    c_l1 = (bbox_pred[:, :, :, None, :] - gc[None, :, None, :, :]).abs().sum(-1) * w_l1
    boxes = (xyxy(bbox_pred) * factors[None, :, None, :])[:, :, :, None, :]
    gts = gt_bboxes[None, :, None, :, :]
    c_iou = -{'giou': giou, 'iou': iou}[iou_mode](boxes, gts) * w_iou
    return c_cls + c_l1 + c_iou


def quality_focal_loss_sum(pred, target, box_pred, box_target, beta=2.0, weight=None):
    """ops.quality_focal_loss_sum: pred (S,N,C) logits, target (S,N) in [0,C] (C = background), boxes (S,N,4) cxcywh normalised,
    weight (S,N) or None -> (S,)."""
    S, N, C = pred.shape
    s = iou(xyxy(box_pred.detach()), xyxy(box_target)).to(pred.dtype)  # (S,N): the quality of a foreground row
    sig = pred.sigmoid()
    onehot = F.one_hot(target, C + 1)[..., :C].to(pred.dtype)
    score = onehot * s.unsqueeze(-1)                                     # 0 off the target class and on background rows
    off = F.binary_cross_entropy_with_logits(pred, torch.zeros_like(pred), reduction='none') * sig.pow(beta)
    at = F.binary_cross_entropy_with_logits(pred, score, reduction='none') * (score - sig).abs().pow(beta)
    loss = torch.where(onehot > 0, at, off).sum(-1)
    if weight is not None:
        loss = loss * weight
    return loss.sum(1)
