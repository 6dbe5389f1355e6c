"""Detection / segmentation loss pieces: box utilities, matching cost (giou / iou), the assignment solvers, focal / quality focal /
box loss sums (GIoU, and the IoU / DIoU / CIoU kinds), the
fused upsample + cross-entropy (plain, and with class weights / avg_non_ignore / OHEM), the fused upsample + Dice / Tversky /
sigmoid focal / Lovasz-softmax."""
import math

import torch
from torch.autograd import Function

from .core import _WS, _Prof, _chk, _f32c, _ptr, _stream, lib

def bbox_cxcywh_to_xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def bbox_xyxy_to_cxcywh(b):
    x1, y1, x2, y2 = b.unbind(-1)
    return torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], dim=-1)


def _giou(b1, b2, aligned, eps=1e-6):
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    if aligned:
        lt, rb = torch.max(b1[..., :2], b2[..., :2]), torch.min(b1[..., 2:], b2[..., 2:])
        elt, erb = torch.min(b1[..., :2], b2[..., :2]), torch.max(b1[..., 2:], b2[..., 2:])
        a1, a2 = area1, area2
    else:
        lt = torch.max(b1[..., :, None, :2], b2[..., None, :, :2])
        rb = torch.min(b1[..., :, None, 2:], b2[..., None, :, 2:])
        elt = torch.min(b1[..., :, None, :2], b2[..., None, :, :2])
        erb = torch.max(b1[..., :, None, 2:], b2[..., None, :, 2:])
        a1, a2 = area1[..., None], area2[..., None, :]
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = (a1 + a2 - overlap).clamp(min=eps)
    ious = overlap / union
    ewh = (erb - elt).clamp(min=0)
    earea = (ewh[..., 0] * ewh[..., 1]).clamp(min=eps)
    return ious - (earea - union) / earea


def _iou(b1, b2, eps=1e-6):
    """mmdet bbox_overlaps(mode='iou') of every box of b1 (..., N, 4) against every box of b2 (..., M, 4), xyxy."""
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    wh = (torch.min(b1[..., :, None, 2:], b2[..., None, :, 2:]) - torch.max(b1[..., :, None, :2], b2[..., None, :, :2])).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    return overlap / (area1[..., None] + area2[..., None, :] - overlap).clamp(min=eps)


IOU_MODES = {'giou': 0, 'iou': 1}                     # IoUCost's iou_mode -> rscotr_match_cost_kind
BOX_KINDS = {'giou': 0, 'iou': 1, 'diou': 2, 'ciou': 3}  # loss_iou holder -> rscotr_box_loss_kind
IOU_LOSS_MODES = {'linear': 0, 'square': 1, 'log': 2}  # IoULoss's mode


def match_cost(cls_score, bbox_pred, gt_bboxes, gt_labels, img_w, img_h, w_cls, w_l1, w_iou, alpha, gamma, eps, iou_mode='giou'):
    """mmdet FocalLossCost + BBoxL1Cost(xywh) + IoUCost(iou_mode: 'giou' | 'iou') for S prediction sets of one image:
    cls_score (S,Q,C), bbox_pred (S,Q,4) cxcywh normalised, gt (G,4) xyxy pixels -> (S,Q,G)."""
    if iou_mode not in IOU_MODES:
        raise ValueError(f'match_cost: iou_mode must be one of {sorted(IOU_MODES)}, got {iou_mode!r}')
    factor = gt_bboxes.new_tensor([img_w, img_h, img_w, img_h])
    p = cls_score.sigmoid()
    neg = -(1 - p + eps).log() * (1 - alpha) * p.pow(gamma)
    pos = -(p + eps).log() * alpha * (1 - p).pow(gamma)
    c_cls = (pos[..., gt_labels] - neg[..., gt_labels]) * w_cls
    gt_c = bbox_xyxy_to_cxcywh(gt_bboxes / factor)
    c_l1 = (bbox_pred[..., :, None, :] - gt_c[None, None, :, :]).abs().sum(-1) * w_l1
    boxes = bbox_cxcywh_to_xyxy(bbox_pred) * factor
    gts = gt_bboxes.unsqueeze(0).expand(boxes.shape[0], -1, -1)
    c_iou = -(_giou(boxes, gts, aligned=False) if iou_mode == 'giou' else _iou(boxes, gts)) * w_iou
    return c_cls + c_l1 + c_iou


def match_cost_batched(cls_score, bbox_pred, gt_bboxes, gt_labels, factors, w_cls, w_l1, w_iou, alpha, gamma, eps):
    """mmdet FocalLossCost + BBoxL1Cost(xywh) + IoUCost(giou) for all images at once on padded ground truth, one
    kernel (rscotr_match_cost): cls_score (S,B,Q,C), bbox_pred (S,B,Q,4), gt_bboxes (B,G,4) xyxy pixels, gt_labels
    (B,G), factors (B,4) = (w,h,w,h) -> (S,B,Q,G).  Columns of padding ground truths hold finite garbage; the
    assignment ignores them."""
    cls_score, bbox_pred, gt_bboxes, factors = _f32c(cls_score), _f32c(bbox_pred), _f32c(gt_bboxes), _f32c(factors)
    gt_labels = gt_labels.contiguous()
    _chk(cls_score, bbox_pred, gt_bboxes, gt_labels, factors)
    S, B, Q, C = cls_score.shape
    G = gt_bboxes.shape[1]
    cost = torch.empty((S, B, Q, G), dtype=torch.float32, device=cls_score.device)
    lib.call('rscotr_match_cost', cls_score.data_ptr(), bbox_pred.data_ptr(), gt_bboxes.data_ptr(), gt_labels.data_ptr(),
             factors.data_ptr(), cost.data_ptr(), S, B, Q, C, G, float(w_cls), float(w_l1), float(w_iou), float(alpha),
             float(gamma), float(eps), _stream())
    return cost


def match_cost_batched_kind(cls_score, bbox_pred, gt_bboxes, gt_labels, factors, w_cls, w_l1, w_iou, alpha, gamma, eps,
                            iou_mode='giou'):
    """match_cost_batched with IoUCost's iou_mode chosen ('giou' | 'iou': cost = -IoU * w_iou, union clamped at 1e-6), one
    kernel (rscotr_match_cost_kind); 'giou' launches match_cost_batched's kernel."""
    if iou_mode not in IOU_MODES:
        raise ValueError(f'match_cost_batched_kind: iou_mode must be one of {sorted(IOU_MODES)}, got {iou_mode!r}')
    cls_score, bbox_pred, gt_bboxes, factors = _f32c(cls_score), _f32c(bbox_pred), _f32c(gt_bboxes), _f32c(factors)
    gt_labels = gt_labels.contiguous()
    _chk(cls_score, bbox_pred, gt_bboxes, gt_labels, factors)
    S, B, Q, C = cls_score.shape
    G = gt_bboxes.shape[1]
    cost = torch.empty((S, B, Q, G), dtype=torch.float32, device=cls_score.device)
    lib.call('rscotr_match_cost_kind', cls_score.data_ptr(), bbox_pred.data_ptr(), gt_bboxes.data_ptr(), gt_labels.data_ptr(),
             factors.data_ptr(), cost.data_ptr(), S, B, Q, C, G, float(w_cls), float(w_l1), float(w_iou), float(alpha),
             float(gamma), float(eps), IOU_MODES[iou_mode], _stream())
    return cost


def lsap_batch(flat_cost, rows, cols):
    """Solve len(rows) assignment problems whose fp32 costs are concatenated in `flat_cost`
    (device or host).  ONE device->host copy, then the C-ABI solver (rscotr_lsap_batch_f32).
    Returns (row_inds, col_inds): lists of int64 numpy arrays (row_inds ascending, as SciPy)."""
    import numpy as np
    host = flat_cost.detach().to('cpu', torch.float32).contiguous().numpy()  # the step's one sync
    n = len(rows)
    sizes = np.asarray(rows, dtype=np.int64) * np.asarray(cols, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    outs = np.minimum(rows, cols).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(outs)[:-1]]).astype(np.int64)
    total = int(outs.sum())
    r = np.zeros(max(total, 1), dtype=np.int64)
    c = np.zeros(max(total, 1), dtype=np.int64)
    rows_a = np.asarray(rows, dtype=np.int32)
    cols_a = np.asarray(cols, dtype=np.int32)
    assert host.size == int(sizes.sum())
    lib.call('rscotr_lsap_batch_f32', host.ctypes.data, offsets.ctypes.data, rows_a.ctypes.data,
             cols_a.ctypes.data, n, out_off.ctypes.data, r.ctypes.data, c.ctypes.data)
    return ([r[out_off[k]:out_off[k] + outs[k]] for k in range(n)],
            [c[out_off[k]:out_off[k] + outs[k]] for k in range(n)])


def lsap_device(cost, gcount):
    """The matcher's assignment problems solved ON THE DEVICE (rscotr_lsap_dev_f32: SciPy's algorithm and
    tie-breaks in fp64, one wavefront per problem, no host round trip).  cost (P, Q, ld) fp32 with the
    first gcount[p] columns of problem p real; gcount (P,) int32 device.  Returns q_for_gt (P, ld) int32:
    the query assigned to each ground truth, -1 for padding columns."""
    cost = _f32c(cost)
    _chk(cost, gcount)
    assert gcount.dtype == torch.int32 and gcount.is_contiguous()
    P, Q, ld = cost.shape
    out = torch.empty((P, ld), dtype=torch.int32, device=cost.device)
    lib.call('rscotr_lsap_dev_f32', cost.data_ptr(), gcount.data_ptr(), P, Q, ld, out.data_ptr(), _stream())
    return out


class _RefineBox(Function):
    @staticmethod
    def forward(ctx, delta, ref, eps):
        delta, ref = _f32c(delta), _f32c(ref)
        _chk(delta, ref)
        out = torch.empty_like(delta)
        lib.call('rscotr_refine_box_fwd', delta.data_ptr(), ref.data_ptr(), out.data_ptr(), delta.numel(), float(eps), _stream())
        ctx.save_for_backward(out, ref)
        ctx.eps = float(eps)
        return out

    @staticmethod
    def backward(ctx, g):
        out, ref = ctx.saved_tensors
        g = _f32c(g)
        dd = torch.empty_like(out) if ctx.needs_input_grad[0] else None
        dr = torch.empty_like(out) if ctx.needs_input_grad[1] else None
        lib.call('rscotr_refine_box_bwd', g.data_ptr(), out.data_ptr(), ref.data_ptr(), _ptr(dd), _ptr(dr), out.numel(),
                 ctx.eps, _stream())
        return dd, dr, None


def refine_box(delta, ref, eps=1e-3):
    """sigmoid(delta + inverse_sigmoid(ref, eps)): one kernel per direction (rscotr_refine_box_*)."""
    return _RefineBox.apply(delta, ref, eps)


class _FocalSum(Function):
    @staticmethod
    def forward(ctx, pred, target, gamma, alpha, weight):
        pred = _f32c(pred)
        target = target.contiguous()
        weight = None if weight is None else _f32c(weight)
        _chk(pred, target, weight)
        S, N, C = pred.shape
        sums = torch.empty(S, dtype=torch.float32, device=pred.device)
        dpred = torch.empty_like(pred)
        lib.call('rscotr_focal_sum', pred.data_ptr(), target.data_ptr(), _ptr(weight), sums.data_ptr(), dpred.data_ptr(),
                 S, N, C, float(gamma), float(alpha), _stream())
        ctx.save_for_backward(dpred)
        return sums

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g.view(-1, 1, 1), None, None, None, None


def sigmoid_focal_loss_sum(pred, target, gamma, alpha, weight=None):
    """mmcv sigmoid_focal_loss (CUDA op semantics) summed per set, one kernel that also leaves the gradient
    (rscotr_focal_sum): pred (S,N,C) logits, target (S,N) int64 in [0,C] with C = background, optional per-sample
    weight (S,N) -> (S,)."""
    return _FocalSum.apply(pred, target, gamma, alpha, weight)


class _BoxLoss(Function):
    @staticmethod
    def forward(ctx, pred, target, weight, factors, eps):
        pred, target, weight, factors = _f32c(pred), _f32c(target), _f32c(weight), _f32c(factors)
        _chk(pred, target, weight, factors)
        S, B, Q, _ = pred.shape
        sums = torch.empty((2, S), dtype=torch.float32, device=pred.device)
        d_l1, d_gi = torch.empty_like(pred), torch.empty_like(pred)
        lib.call('rscotr_box_loss', pred.data_ptr(), target.data_ptr(), weight.data_ptr(), factors.data_ptr(),
                 sums.data_ptr(), d_l1.data_ptr(), d_gi.data_ptr(), S, B, Q, float(eps), _stream())
        ctx.save_for_backward(d_l1, d_gi)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g1, g2):
        d_l1, d_gi = ctx.saved_tensors
        return d_l1 * g1.view(-1, 1, 1, 1) + d_gi * g2.view(-1, 1, 1, 1), None, None, None, None


def box_loss_sums(pred, target, weight, factors, eps=1e-6):
    """L1 (cxcywh, normalised) and GIoU (xyxy in pixels: * factors (B,4)) loss sums per prediction set
    (detr_head.py:392-415), one kernel that also leaves both gradients (rscotr_box_loss):
    pred / target / weight (S,B,Q,4) -> (l1 (S,), giou (S,)); the GIoU weight is the mean of the 4 box weights."""
    return _BoxLoss.apply(pred, target, weight, factors, eps)


class _BoxLossKind(Function):
    @staticmethod
    def forward(ctx, pred, target, weight, factors, eps, kind, mode):
        pred, target, weight, factors = _f32c(pred), _f32c(target), _f32c(weight), _f32c(factors)
        _chk(pred, target, weight, factors)
        S, B, Q, _ = pred.shape
        sums = torch.empty((2, S), dtype=torch.float32, device=pred.device)
        d_l1, d_iou = torch.empty_like(pred), torch.empty_like(pred)
        lib.call('rscotr_box_loss_kind', pred.data_ptr(), target.data_ptr(), weight.data_ptr(), factors.data_ptr(),
                 sums.data_ptr(), d_l1.data_ptr(), d_iou.data_ptr(), S, B, Q, float(eps), kind, mode, _stream())
        ctx.save_for_backward(d_l1, d_iou)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g1, g2):
        d_l1, d_iou = ctx.saved_tensors
        return d_l1 * g1.view(-1, 1, 1, 1) + d_iou * g2.view(-1, 1, 1, 1), None, None, None, None, None, None


def box_loss_sums_kind(pred, target, weight, factors, kind='giou', eps=1e-6, mode='log'):
    """box_loss_sums with the IoU loss chosen: kind 'giou' | 'iou' | 'diou' | 'ciou' = mmdet GIoULoss / IoULoss / DIoULoss /
    CIoULoss on the pixel boxes; `mode` ('linear' | 'square' | 'log') is IoULoss's and read by kind 'iou' only.  One kernel
    that also leaves both gradients (rscotr_box_loss_kind; 'giou' launches box_loss_sums' kernel) -> (l1 (S,), iou loss (S,)).
    A row whose four weights are 0 adds an exact 0 and gets a zero gradient."""
    if kind not in BOX_KINDS:
        raise ValueError(f'box_loss_sums_kind: kind must be one of {sorted(BOX_KINDS)}, got {kind!r}')
    if mode not in IOU_LOSS_MODES:
        raise ValueError(f'box_loss_sums_kind: mode must be one of {sorted(IOU_LOSS_MODES)}, got {mode!r}')
    return _BoxLossKind.apply(pred, target, weight, factors, eps, BOX_KINDS[kind], IOU_LOSS_MODES[mode])


class _QFLSum(Function):
    @staticmethod
    def forward(ctx, pred, target, box_pred, box_target, beta, weight):
        pred, box_pred, box_target = _f32c(pred), _f32c(box_pred.detach()), _f32c(box_target)
        target = target.contiguous()
        weight = None if weight is None else _f32c(weight)
        _chk(pred, target, box_pred, box_target, weight)
        S, N, C = pred.shape
        if tuple(box_pred.shape) != (S, N, 4) or tuple(box_target.shape) != (S, N, 4) or tuple(target.shape) != (S, N):
            raise ValueError(f'quality_focal_loss_sum: pred {tuple(pred.shape)} needs target (S,N) and boxes (S,N,4), got '
                             f'{tuple(target.shape)}, {tuple(box_pred.shape)}, {tuple(box_target.shape)}')
        sums = torch.empty(S, dtype=torch.float32, device=pred.device)
        dpred = torch.empty_like(pred)
        lib.call('rscotr_qfl_sum', pred.data_ptr(), target.data_ptr(), _ptr(weight), box_pred.data_ptr(), box_target.data_ptr(),
                 sums.data_ptr(), dpred.data_ptr(), S, N, C, float(beta), _stream())
        ctx.save_for_backward(dpred)
        return sums

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g.view(-1, 1, 1), None, None, None, None, None


def quality_focal_loss_sum(pred, target, box_pred, box_target, beta=2.0, weight=None):
    """mmdet QualityFocalLoss (as the DETR / DINO heads of mmdet 3.x use it) summed per set, one kernel that also leaves the
    gradient (rscotr_qfl_sum): pred (S,N,C) logits, target (S,N) int64 in [0,C] with C = background, box_pred / box_target
    (S,N,4) cxcywh normalised, optional per-sample weight (S,N) -> (S,).  The quality score of a foreground row is the IoU of
    its two boxes, a constant: box_pred gets no gradient."""
    if not float(beta) >= 0:
        raise ValueError(f'quality_focal_loss_sum: beta must be >= 0, got {beta}')
    return _QFLSum.apply(pred, target, box_pred, box_target, beta, weight)


def _upsample_args(logit, label, class_weight=None):
    """The opening of the three fused upsample losses: fp32-contiguous logits and class weights, contiguous labels, all on
    one device, as many class weights as channels -> (logit, label, cw | None, B, C, h, w, H, W, lse (B,H,W) to be written)."""
    logit = _f32c(logit)
    label = label.contiguous()
    cw = None if class_weight is None else _f32c(class_weight)
    _chk(logit, label, cw)
    B, C, h, w = logit.shape
    H, W = label.shape[-2:]
    if cw is not None and cw.numel() != C:
        raise ValueError(f'class_weight has {cw.numel()} entries, the logits have {C} channels')
    lse = torch.empty((B, H, W), dtype=torch.float32, device=logit.device)
    return logit, label, cw, B, C, h, w, H, W, lse


class _UpsampleCE(Function):
    @staticmethod
    def forward(ctx, logit, label, ignore_index):
        logit, label, _, B, C, h, w, H, W, lse = _upsample_args(logit, label)
        sums = torch.empty(3, dtype=torch.float32, device=logit.device)
        with _Prof('upsample_ce_fwd', 4 * B * C * h * w + 12 * B * H * W):
            nws = lib.rscotr_upsample_ce_workspace()
            lib.call('rscotr_upsample_ce_fwd', logit.data_ptr(), label.data_ptr(), lse.data_ptr(), sums.data_ptr(),
                     B, C, h, w, H, W, int(ignore_index), _WS.get(nws, logit.device).data_ptr(), nws, _stream())
        ctx.save_for_backward(logit, label, lse)
        ctx.ignore = int(ignore_index)
        ctx.mark_non_differentiable(sums)
        npix = float(B * H * W)
        return sums[0] / npix, sums

    @staticmethod
    def backward(ctx, g_loss, g_sums):
        logit, label, lse = ctx.saved_tensors
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        gscale = (g_loss / float(B * H * W)).reshape(1).float().contiguous()
        dlogit = torch.empty_like(logit)
        with _Prof('upsample_ce_bwd', 8 * B * C * h * w + 12 * B * H * W):
            lib.call('rscotr_upsample_ce_bwd', logit.data_ptr(), label.data_ptr(), lse.data_ptr(), gscale.data_ptr(),
                     dlogit.data_ptr(), B, C, h, w, H, W, ctx.ignore, _stream())
        return dlogit, None, None


def upsample_ce(seg_logit, label, ignore_index=255):
    """mmseg BaseDecodeHead.losses: bilinear resize (align_corners=False) to the label size, CE with
    ignore_index averaged over ALL pixels, and top-1 accuracy over non-ignored pixels — fused: the
    upsampled logits are never materialised (rscotr_upsample_ce_*).
    seg_logit (B,C,h,w), label (B,H,W) int64 -> (loss_ce 0-d, acc (1,))."""
    loss, sums = _UpsampleCE.apply(seg_logit, label, ignore_index)
    acc = (sums[1] * 100.0 / (sums[2] + torch.finfo(torch.float32).eps)).reshape(1)
    return loss, acc


class _UpsampleCEWeighted(Function):
    """The fused seg loss with class weights, the avg_non_ignore normaliser and OHEM pixel sampling (rscotr_upsample_ce_w_* /
    rscotr_upsample_ce_ohem).  norm: 'all' (/ B*H*W), 'valid' (/ (#non-ignored + eps)) or 'sum'; ohem: None or
    (kept, nll_thresh).  Everything stays on the device: the normaliser and the upstream gradient meet in the device scalar
    grad_scale."""

    @staticmethod
    def forward(ctx, logit, label, ignore_index, class_weight, norm, ohem):
        logit, label, cw, B, C, h, w, H, W, lse = _upsample_args(logit, label, class_weight)
        dev = logit.device
        nll, pixw = torch.empty_like(lse), torch.empty_like(lse)
        sums = torch.empty(4, dtype=torch.float32, device=dev)
        nws = lib.rscotr_upsample_ce_w_workspace()
        ws = _WS.get(nws, dev).data_ptr()
        with _Prof('upsample_ce_w_fwd', 4 * B * C * h * w + 20 * B * H * W):
            lib.call('rscotr_upsample_ce_w_fwd', logit.data_ptr(), label.data_ptr(), _ptr(cw), lse.data_ptr(), nll.data_ptr(),
                     pixw.data_ptr(), sums.data_ptr(), B, C, h, w, H, W, int(ignore_index), ws, nws, _stream())
        num = sums[0]
        if ohem is not None:
            kept, nll_thresh = ohem
            with _Prof('upsample_ce_ohem', 6 * 12 * B * H * W):
                lib.call('rscotr_upsample_ce_ohem', label.data_ptr(), _ptr(cw), nll.data_ptr(), pixw.data_ptr(),
                         sums.data_ptr() + 12, B * H * W, C, int(ignore_index), int(kept), float(nll_thresh), ws, nws, _stream())
            num = sums[3]
        denom = None
        if norm == 'all':
            loss = num / float(B * H * W)
        elif norm == 'valid':
            denom = sums[2] + torch.finfo(torch.float32).eps
            loss = num / denom
        else:
            loss = num.clone()
        ctx.save_for_backward(logit, label, lse, pixw, denom)
        ctx.ignore, ctx.norm = int(ignore_index), norm
        ctx.mark_non_differentiable(sums, pixw)
        return loss, sums, pixw

    @staticmethod
    def backward(ctx, g_loss, g_sums, g_pixw):
        logit, label, lse, pixw, denom = ctx.saved_tensors
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        if ctx.norm == 'all':
            g_loss = g_loss / float(B * H * W)
        elif ctx.norm == 'valid':
            g_loss = g_loss / denom
        gscale = g_loss.reshape(1).float().contiguous()
        dlogit = torch.empty_like(logit)
        with _Prof('upsample_ce_w_bwd', 8 * B * C * h * w + 16 * B * H * W):
            lib.call('rscotr_upsample_ce_w_bwd', logit.data_ptr(), label.data_ptr(), lse.data_ptr(), pixw.data_ptr(),
                     gscale.data_ptr(), dlogit.data_ptr(), B, C, h, w, H, W, ctx.ignore, _stream())
        return dlogit, None, None, None, None, None


def upsample_ce_weighted(seg_logit, label, ignore_index=255, class_weight=None, avg_non_ignore=False, reduction='mean',
                         ohem=None):
    """`upsample_ce` with mmseg's CrossEntropyLoss options and OHEMPixelSampler, still one fused pass over the logits:
        l_p = s_p * class_weight[y_p] * nll_p over the non-ignored pixels,
        reduction='mean': sum l / (B*H*W), or / (#non-ignored + eps) with avg_non_ignore;  'sum': sum l;
        ohem = (thresh, min_kept) or a dict with those keys: s_p = [prob_p < max(kth, thresh)], kth the
        min(min_kept * B, #non-ignored - 1)-th smallest probability of the label over the non-ignored pixels (found on the
        device); None: s_p = 1.
    class_weight: a float tensor of C entries on the logits' device, or None.
    -> (loss 0-d, acc (1,) as upsample_ce: unweighted and unsampled, pix_weight (B,H,W) = s_p * class_weight[y_p], no gradient)."""
    if reduction not in ('mean', 'sum'):
        raise NotImplementedError(f"upsample_ce_weighted: reduction={reduction!r} (only 'mean' and 'sum')")
    norm = 'sum' if reduction == 'sum' else ('valid' if avg_non_ignore else 'all')
    sel = None
    if ohem is not None:
        thresh, min_kept = (ohem['thresh'], ohem['min_kept']) if isinstance(ohem, dict) else ohem
        if thresh is None:
            raise NotImplementedError('upsample_ce_weighted: the loss-ranked OHEM (thresh=None) is not implemented')
        if min_kept < 0:
            raise ValueError(f'min_kept must be >= 0, got {min_kept}')
        sel = (int(min_kept) * seg_logit.shape[0], -math.log(thresh) if thresh > 0 else math.inf)
    if class_weight is not None and not torch.is_tensor(class_weight):
        class_weight = torch.as_tensor(class_weight, dtype=torch.float32, device=seg_logit.device)
    loss, sums, pix_weight = _UpsampleCEWeighted.apply(seg_logit, label, ignore_index, class_weight, norm, sel)
    acc = (sums[1] * 100.0 / (sums[2] + torch.finfo(torch.float32).eps)).reshape(1)
    return loss, acc, pix_weight


class _UpsampleDice(Function):
    """The fused bilinear upsample + softmax + Dice loss (rscotr_upsample_dice_*).  Forward leaves the per-pixel log-sum-exp and
    the two backward coefficients of every (image, class); the upstream gradient meets them on the device (grad_scale)."""

    @staticmethod
    def forward(ctx, logit, label, ignore_index, smooth, class_weight, loss_weight):
        logit, label, cw, B, C, h, w, H, W, lse = _upsample_args(logit, label, class_weight)
        dev = logit.device
        coef = torch.empty((B, C, 2), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = lib.rscotr_upsample_dice_workspace(B, C)
        # the logits twice (log-sum-exp, then the sums), labels, lse written and re-read
        with _Prof('upsample_dice_fwd', 8 * B * C * h * w + 16 * B * H * W):
            lib.call('rscotr_upsample_dice_fwd', logit.data_ptr(), label.data_ptr(), _ptr(cw), lse.data_ptr(), coef.data_ptr(),
                     loss.data_ptr(), B, C, h, w, H, W, int(ignore_index), float(smooth), float(loss_weight),
                     _WS.get(nws, dev).data_ptr(), nws, _stream())
        ctx.save_for_backward(logit, label, lse, coef)
        ctx.ignore = int(ignore_index)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        logit, label, lse, coef = ctx.saved_tensors
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        gscale = g_loss.reshape(1).float().contiguous()
        pix_s = torch.empty_like(lse)
        dlogit = torch.empty_like(logit)
        # pre-pass: logits, labels, lse read, S written; gather: logits read, gradient written, labels, lse, S read
        with _Prof('upsample_dice_bwd', 12 * B * C * h * w + 32 * B * H * W):
            lib.call('rscotr_upsample_dice_bwd', logit.data_ptr(), label.data_ptr(), lse.data_ptr(), coef.data_ptr(),
                     gscale.data_ptr(), pix_s.data_ptr(), dlogit.data_ptr(), B, C, h, w, H, W, ctx.ignore, _stream())
        return dlogit, None, None, None, None, None


def upsample_dice(seg_logit, label, ignore_index=255, smooth=1.0, class_weight=None, loss_weight=1.0):
    """mmseg 0.28 DiceLoss (exponent 2) as BaseDecodeHead.losses reaches it, fused: bilinear resize (align_corners=False) to the
    label size, softmax, and per (image, class)
        num = 2 * sum p t v + smooth,  den = sum (p^2 + t) + smooth,
    t the one-hot of clamp(label, 0, C-1), v = [label != ignore_index] (den is not masked: mmseg's quirk);
        loss = loss_weight / C * sum_{c != ignore_index} class_weight[c] * mean_b (1 - num / den).
    Neither the up-sampled logits nor the probabilities are materialised (rscotr_upsample_dice_*); bit-reproducible.
    seg_logit (B,C,h,w), label (B,H,W) int64, class_weight a float tensor / list of C entries or None -> loss 0-d."""
    if class_weight is not None and not torch.is_tensor(class_weight):
        class_weight = torch.as_tensor(class_weight, dtype=torch.float32, device=seg_logit.device)
    return _UpsampleDice.apply(seg_logit, label, ignore_index, smooth, class_weight, loss_weight)


class _UpsampleTversky(Function):
    """The fused bilinear upsample + softmax + Tversky loss (rscotr_upsample_tversky_*): the Dice Function's buffers and
    launches on the second instantiation of its kernels."""

    @staticmethod
    def forward(ctx, logit, label, ignore_index, alpha, beta, smooth, class_weight, loss_weight):
        logit, label, cw, B, C, h, w, H, W, lse = _upsample_args(logit, label, class_weight)
        dev = logit.device
        coef = torch.empty((B, C, 2), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = lib.rscotr_upsample_tversky_workspace(B, C)
        # the logits twice (log-sum-exp, then the sums), labels, lse written and re-read
        with _Prof('upsample_tversky_fwd', 8 * B * C * h * w + 16 * B * H * W):
            lib.call('rscotr_upsample_tversky_fwd', logit.data_ptr(), label.data_ptr(), _ptr(cw), lse.data_ptr(), coef.data_ptr(),
                     loss.data_ptr(), B, C, h, w, H, W, int(ignore_index), float(alpha), float(beta), float(smooth),
                     float(loss_weight), _WS.get(nws, dev).data_ptr(), nws, _stream())
        ctx.save_for_backward(logit, label, lse, coef)
        ctx.ignore = int(ignore_index)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        logit, label, lse, coef = ctx.saved_tensors
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        gscale = g_loss.reshape(1).float().contiguous()
        pix_s = torch.empty_like(lse)
        dlogit = torch.empty_like(logit)
        # pre-pass: logits, labels, lse read, S written; gather: logits read, gradient written, labels, lse, S read
        with _Prof('upsample_tversky_bwd', 12 * B * C * h * w + 32 * B * H * W):
            lib.call('rscotr_upsample_tversky_bwd', logit.data_ptr(), label.data_ptr(), lse.data_ptr(), coef.data_ptr(),
                     gscale.data_ptr(), pix_s.data_ptr(), dlogit.data_ptr(), B, C, h, w, H, W, ctx.ignore, _stream())
        return dlogit, None, None, None, None, None, None, None


def upsample_tversky(seg_logit, label, ignore_index=255, alpha=0.3, beta=0.7, smooth=1.0, class_weight=None, loss_weight=1.0):
    """mmseg 0.28 TverskyLoss as BaseDecodeHead.losses reaches it, fused: bilinear resize (align_corners=False) to the label
    size, softmax, and per (image, class)
        TP = sum p t v,  FP = sum p (1 - t) v,  FN = sum (1 - p) t v,
    t the one-hot of clamp(label, 0, C-1), v = [label != ignore_index] (all three sums masked, unlike Dice's denominator);
        loss = loss_weight / C * sum_{c != ignore_index} class_weight[c] * mean_b (1 - (TP + smooth) / (TP + alpha FP + beta FN + smooth)).
    alpha + beta == 1 and smooth > 0 (an all-ignored image would be 0 / 0), else ValueError.  Neither the up-sampled logits nor
    the probabilities are materialised (rscotr_upsample_tversky_*); bit-reproducible.
    seg_logit (B,C,h,w), label (B,H,W) int64, class_weight a float tensor / list of C entries or None -> loss 0-d."""
    if float(alpha) + float(beta) != 1.0:
        raise ValueError(f'upsample_tversky: alpha + beta must be 1.0, got {alpha} + {beta}')
    if not float(smooth) > 0:
        raise ValueError(f'upsample_tversky: smooth must be > 0, got {smooth}')
    if class_weight is not None and not torch.is_tensor(class_weight):
        class_weight = torch.as_tensor(class_weight, dtype=torch.float32, device=seg_logit.device)
    return _UpsampleTversky.apply(seg_logit, label, ignore_index, alpha, beta, smooth, class_weight, loss_weight)


class _UpsampleFocal(Function):
    """The fused bilinear upsample + sigmoid focal loss (rscotr_upsample_focal_*).  Nothing per pixel is saved: backward walks the
    logits again.  scale (loss_weight, over B*H*W*C for the mean) and the upstream gradient meet in the device scalar grad_scale."""

    @staticmethod
    def forward(ctx, logit, label, ignore_index, gamma, alpha, alpha_c, class_weight, scale):
        logit = _f32c(logit)
        label = label.contiguous()
        cw = None if class_weight is None else _f32c(class_weight)
        ac = None if alpha_c is None else _f32c(alpha_c)
        _chk(logit, label, cw, ac)
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        for name, t in (('class_weight', cw), ('alpha', ac)):
            if t is not None and t.numel() != C:
                raise ValueError(f'{name} has {t.numel()} entries, the logits have {C} channels')
        loss = torch.empty(1, dtype=torch.float32, device=logit.device)
        nws = lib.rscotr_upsample_focal_workspace()
        # the logits and the labels once
        with _Prof('upsample_focal_fwd', 4 * B * C * h * w + 8 * B * H * W):
            lib.call('rscotr_upsample_focal_fwd', logit.data_ptr(), label.data_ptr(), _ptr(ac), _ptr(cw), loss.data_ptr(), B, C, h,
                     w, H, W, int(ignore_index), float(gamma), float(alpha), float(scale), _WS.get(nws, logit.device).data_ptr(),
                     nws, _stream())
        ctx.save_for_backward(logit, label, ac, cw)
        ctx.opts = (int(ignore_index), float(gamma), float(alpha), float(scale))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        logit, label, ac, cw = ctx.saved_tensors
        ignore, gamma, alpha, scale = ctx.opts
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        gscale = (g_loss * scale).reshape(1).float().contiguous()
        dlogit = torch.empty_like(logit)
        # logits read, gradient written, labels read
        with _Prof('upsample_focal_bwd', 8 * B * C * h * w + 8 * B * H * W):
            lib.call('rscotr_upsample_focal_bwd', logit.data_ptr(), label.data_ptr(), _ptr(ac), _ptr(cw), gscale.data_ptr(),
                     dlogit.data_ptr(), B, C, h, w, H, W, ignore, gamma, alpha, _stream())
        return dlogit, None, None, None, None, None, None, None


def upsample_focal(seg_logit, label, ignore_index=255, gamma=2.0, alpha=0.5, class_weight=None, reduction='mean', loss_weight=1.0):
    """mmseg 0.28 FocalLoss (the sigmoid form, py_sigmoid_focal_loss) as BaseDecodeHead.losses reaches it, fused: bilinear resize
    (align_corners=False) to the label size, then per pixel and class
        t = [label == c],  v = [label != ignore_index],  s = sigmoid(u),  q = (1 - s) t + s (1 - t),
        e = BCE_with_logits(u, t) * (alpha_c t + (1 - alpha_c) (1 - t)) * q^gamma * class_weight[c] * v;
        reduction='mean': loss_weight * sum e / (B*H*W*C) (ignored pixels count in the divisor);  'sum': loss_weight * sum e.
    A label outside [0, C) that is not ignore_index has no positive class: the pixel is all-negative (mmseg's F.one_hot would
    raise there).  gamma >= 0 (0 gives q^0 = 1 everywhere, with a finite gradient); alpha a float, or a tensor / list of C
    floats; class_weight a float tensor / list of C entries or None.  The up-sampled logits are not materialised
    (rscotr_upsample_focal_*); stable at any logit magnitude; bit-reproducible.
    seg_logit (B,C,h,w), label (B,H,W) int64 -> loss 0-d."""
    if reduction not in ('mean', 'sum'):
        raise NotImplementedError(f"upsample_focal: reduction={reduction!r} (only 'mean' and 'sum')")
    alpha_c = None
    if torch.is_tensor(alpha) or isinstance(alpha, (list, tuple)):
        alpha_c, alpha = torch.as_tensor(alpha, dtype=torch.float32, device=seg_logit.device), 0.0
    if not float(gamma) >= 0:
        raise ValueError(f'upsample_focal: gamma must be >= 0, got {gamma}')
    if class_weight is not None and not torch.is_tensor(class_weight):
        class_weight = torch.as_tensor(class_weight, dtype=torch.float32, device=seg_logit.device)
    B, C = seg_logit.shape[:2]
    H, W = label.shape[-2:]
    scale = float(loss_weight) / float(max(B * H * W * C, 1)) if reduction == 'mean' else float(loss_weight)
    return _UpsampleFocal.apply(seg_logit, label, ignore_index, gamma, alpha, alpha_c, class_weight, scale)


class _UpsampleLovasz(Function):
    """The fused bilinear upsample + softmax + Lovasz-softmax loss (rscotr_upsample_lovasz_*).  Forward leaves the per-pixel
    log-sum-exp, the plane D (slots, B*H*W) = d loss / d p_c and the summed-segment flags; the upstream gradient meets them on the
    device (grad_scale).  slots: an int32 device tensor of the summed classes or None (every class)."""

    @staticmethod
    def forward(ctx, logit, label, ignore_index, slots, present, per_image, image_mean, class_weight, loss_weight):
        logit, label, cw, B, C, h, w, H, W, lse = _upsample_args(logit, label, class_weight)
        _chk(slots)
        dev = logit.device
        nslots = C if slots is None else slots.numel()
        nseg = B * nslots if per_image else nslots
        dplane = torch.empty((nslots, B * H * W), dtype=torch.float32, device=dev)
        meta = torch.empty(nseg + C, dtype=torch.int32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = lib.rscotr_upsample_lovasz_workspace(B, C, nslots, H, W, int(per_image))
        # the logits and lse, then per slot: {key, payload} written, 4 sort passes reading them twice and writing once, the scan
        with _Prof('upsample_lovasz_fwd', 4 * B * C * h * w + 12 * B * H * W + (8 + 4 * 24 + 16) * nslots * B * H * W):
            lib.call('rscotr_upsample_lovasz_fwd', logit.data_ptr(), label.data_ptr(), _ptr(slots), _ptr(cw), lse.data_ptr(),
                     dplane.data_ptr(), meta.data_ptr(), loss.data_ptr(), B, C, nslots, h, w, H, W, int(ignore_index),
                     int(present), int(per_image), int(image_mean), float(loss_weight), _WS.get(nws, dev).data_ptr(), nws,
                     _stream())
        ctx.save_for_backward(logit, label, lse, dplane, meta, slots)
        ctx.opts = (int(ignore_index), nslots, int(per_image))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        logit, label, lse, dplane, meta, slots = ctx.saved_tensors
        ignore, nslots, per_image = ctx.opts
        B, C, h, w = logit.shape
        H, W = label.shape[-2:]
        gscale = g_loss.reshape(1).float().contiguous()
        pix_s = torch.empty_like(lse)
        dlogit = torch.empty_like(logit)
        # pre-pass: logits, labels, lse and the slots' planes read, S written; gather: logits read, gradient written, labels, lse,
        # S and the planes read
        with _Prof('upsample_lovasz_bwd', 12 * B * C * h * w + (32 + 8 * nslots) * B * H * W):
            lib.call('rscotr_upsample_lovasz_bwd', logit.data_ptr(), label.data_ptr(), _ptr(slots), lse.data_ptr(),
                     dplane.data_ptr(), meta.data_ptr(), gscale.data_ptr(), pix_s.data_ptr(), dlogit.data_ptr(), B, C, nslots,
                     h, w, H, W, ignore, per_image, _stream())
        return dlogit, None, None, None, None, None, None, None, None


# the elements one wavefront / one workgroup of a sort pass of csrc/seg_lovasz.hip ranks (rscotr_upsample_lovasz_sort_tile /
# _sort_workgroup return the built values)
LOVASZ_SORT_TILE, LOVASZ_SORT_WORKGROUP = 2048, 8192
_lovasz_slots = {}  # (classes, device) -> int32 device tensor: a constant of the config, made once (also ahead of a capture)


def upsample_lovasz(seg_logit, label, ignore_index=255, classes='present', per_image=False, class_weight=None, reduction='none',
                    loss_weight=1.0):
    """mmseg 0.28 LovaszLoss (loss_type='multi_class': lovasz_softmax) as BaseDecodeHead.losses reaches it, fused: bilinear resize
    (align_corners=False) to the label size, softmax, and per summed class c over the pixels with label != ignore_index
        fg = [label == c],  e = |fg - p_c| sorted descending (equal errors: ascending flat pixel index),
        loss_c = sum_k e_(k) g_k,  g the discrete gradient of the Jaccard index along the sorted order (formed in closed form
        from integer counts: 1 / U_k at a foreground element, I_k / (U_k (U_k - 1)) at a background one);
        loss = loss_weight * mean_c class_weight[c] loss_c.
    classes: 'present' (the classes with a foreground pixel), 'all', or a list of distinct class indices (absent ones included:
    such a class costs its largest p_c).  per_image: the above per image, then reduction 'mean' or 'sum' over the images (an
    image without a valid pixel gives 0 and counts); per_image=False takes reduction='none' only (the loss is a scalar already;
    mmseg asserts the same).  A non-ignored label outside [0, C) is background for every class.  No valid pixel at all: 0.
    Neither the up-sampled logits nor the probabilities are materialised; the ranking is a segmented stable radix sort on the
    device (rscotr_upsample_lovasz_*): bit-reproducible, graph-capturable.  Memory: 20 bytes per (summed class slot, pixel) —
    16 of workspace and the 4 of the saved gradient plane; `classes` as a list bounds it at wide heads.
    seg_logit (B,C,h,w), label (B,H,W) int64, class_weight a float tensor / list of C entries or None -> loss 0-d."""
    C = seg_logit.shape[1]
    if C == 1:
        raise ValueError('upsample_lovasz: the multi-class Lovasz loss needs more than one channel')
    if per_image:
        if reduction not in ('mean', 'sum'):
            raise NotImplementedError(f"upsample_lovasz: per_image=True with reduction={reduction!r} is a vector loss (only "
                                      "'mean' and 'sum')")
    elif reduction != 'none':
        raise NotImplementedError(f"upsample_lovasz: per_image=False with reduction={reduction!r}: write reduction='none' or "
                                  'per_image=True (mmseg asserts the same)')
    slots = None
    if isinstance(classes, str):
        if classes not in ('present', 'all'):
            raise ValueError(f"upsample_lovasz: classes={classes!r} ('present', 'all' or a list of class indices)")
    else:
        cl = tuple(int(c) for c in classes)
        if not cl or len(set(cl)) != len(cl) or min(cl) < 0 or max(cl) >= C:
            raise ValueError(f'upsample_lovasz: classes={list(cl)!r} must be distinct indices in [0, {C})')
        key = (cl, str(seg_logit.device))
        slots = _lovasz_slots.get(key)
        if slots is None:
            slots = _lovasz_slots[key] = torch.tensor(cl, dtype=torch.int32, device=seg_logit.device)
    if class_weight is not None and not torch.is_tensor(class_weight):
        class_weight = torch.as_tensor(class_weight, dtype=torch.float32, device=seg_logit.device)
    return _UpsampleLovasz.apply(seg_logit, label, ignore_index, slots, classes == 'present', bool(per_image),
                                 reduction == 'mean', class_weight, loss_weight)


class _DetProposals(Function):
    """Two-stage proposal selection of the DINO transformer (transformer.py:226-241) as one launch per direction
    (rscotr_det_proposals / _bwd): row maximum, top-k, the proposal add, both gathers and the sigmoid forward; the two
    scattered gradients backward (every row of d(enc_cls) / d(enc_reg) written once: no zero-fill, no scatter-add)."""

    @staticmethod
    def forward(ctx, enc_cls, enc_reg, proposals, K):
        B, N, C = enc_cls.shape
        cls2, reg2, prop = _f32c(enc_cls), _f32c(enc_reg), _f32c(proposals)
        assert reg2.shape == (B, N, 4) and prop.shape[1:] == (N, 4) and prop.shape[0] in (1, B)
        _chk(cls2, reg2, prop)
        dev = cls2.device
        idx = torch.empty((B, K), dtype=torch.int64, device=dev)
        score = torch.empty((B, K, C), dtype=torch.float32, device=dev)
        unact = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
        anchor = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
        inv = torch.empty((B, N), dtype=torch.int32, device=dev)
        lib.call('rscotr_det_proposals', cls2.data_ptr(), reg2.data_ptr(), prop.data_ptr(), int(prop.shape[0] == B and B > 1),
                 idx.data_ptr(), score.data_ptr(), unact.data_ptr(), anchor.data_ptr(), inv.data_ptr(), B, N, C, K, _stream())
        ctx.save_for_backward(anchor, inv)
        ctx.geom = (B, N, C, K)
        ctx.mark_non_differentiable(idx, unact)
        ctx.set_materialize_grads(False)
        return idx, score, unact, anchor

    @staticmethod
    def backward(ctx, _gi, g_score, _gu, g_anchor):
        anchor, inv = ctx.saved_tensors
        B, N, C, K = ctx.geom
        need = ctx.needs_input_grad
        gs = None if g_score is None else _f32c(g_score)
        ga = None if g_anchor is None else _f32c(g_anchor)
        d_cls = torch.empty((B, N, C), dtype=torch.float32, device=anchor.device) if need[0] else None
        d_reg = torch.empty((B, N, 4), dtype=torch.float32, device=anchor.device) if need[1] else None
        if d_cls is not None or d_reg is not None:
            lib.call('rscotr_det_proposals_bwd', _ptr(gs), _ptr(ga), anchor.data_ptr(), inv.data_ptr(), _ptr(d_cls), _ptr(d_reg),
                     B, N, C, K, _stream())
        return d_cls, d_reg, None, None


DET_PROPOSALS_MAX_N, DET_PROPOSALS_MAX_K = 36864, 1024


def det_proposals(enc_cls, enc_reg, proposals, K):
    """-> (topk_idx (B,K) int64, topk_score (B,K,C), topk_unact (B,K,4) detached, topk_anchor (B,K,4)): the K tokens with the
    largest class score (torch.topk order: descending; equal scores: lower index first), their class rows, enc_reg + proposals
    and its sigmoid.  enc_cls (B,N,C), enc_reg (B,N,4), proposals (B|1,N,4) (no gradient)."""
    return _DetProposals.apply(enc_cls, enc_reg, proposals.detach(), int(K))


def det_targets(q_for_gt, gt_lab, gt_boxn, Q, num_classes):
    """q_for_gt (S,B,G) int32 (ops.lsap_device), gt_lab (B,G) int64, gt_boxn (B,G,4) -> (labels (S,B,Q) int64, bbox_targets
    (S,B,Q,4), bbox_weights (S,B,Q,4)) of the assignment (detr_head.py:475-543), one launch."""
    S, B, G = q_for_gt.shape
    assert q_for_gt.dtype == torch.int32 and gt_lab.dtype == torch.int64 and gt_lab.shape == (B, G)
    q_for_gt, gt_lab, gt_boxn = q_for_gt.contiguous(), gt_lab.contiguous(), _f32c(gt_boxn)
    _chk(q_for_gt, gt_lab, gt_boxn)
    dev = gt_boxn.device
    labels = torch.empty((S, B, Q), dtype=torch.int64, device=dev)
    bt = torch.empty((S, B, Q, 4), dtype=torch.float32, device=dev)
    bw = torch.empty((S, B, Q, 4), dtype=torch.float32, device=dev)
    lib.call('rscotr_det_targets', q_for_gt.data_ptr(), gt_lab.data_ptr(), gt_boxn.data_ptr(), labels.data_ptr(), bt.data_ptr(),
             bw.data_ptr(), S, B, Q, G, int(num_classes), _stream())
    return labels, bt, bw
