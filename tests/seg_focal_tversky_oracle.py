"""fp64 torch restatements (test infrastructure only) of the sigmoid focal and the Tversky seg losses the fused kernels
implement (`ops.upsample_focal`: rscotr_upsample_focal_*, `ops.upsample_tversky`: rscotr_upsample_tversky_*), written apart
from the package: F.interpolate, the formulas; gradients come from autograd.  Inputs: `dice_inputs` of tests/seg_dice_oracle.py.

mmseg is not installed.  The contracts below are restated from mmseg 0.28 `FocalLoss` (py_sigmoid_focal_loss) and `TverskyLoss`
as `BaseDecodeHead.losses` reaches them AS READ: parity with mmseg by reading, unpinned (as tests/seg_dice_oracle.py is).

With z = seg_logit (B,C,h,w), y = label (B,H,W) int64, u = bilinear_resize(z, (H,W), align_corners=False):

FocalLoss (the head's ignore_index):
    t[b,c,.] = [y == c]                                an ignored pixel, or any label outside [0, C), has no positive class
    v[b,.]   = [y != ignore_index]
    s = sigmoid(u);  q = (1 - s) t + s (1 - t)
    e = BCE_with_logits(u, t) * (alpha_c t + (1 - alpha_c)(1 - t)) * q^gamma * class_weight[c] * v
    loss = loss_weight * (sum e / (B*H*W*C) for 'mean': ignored pixels count in the divisor | sum e for 'sum')
  (mmseg's F.one_hot would raise on a non-ignored label >= C; here such a pixel is all-negative.)

TverskyLoss (its OWN ignore_index):
    p = softmax(u, dim=1);  t[b,c,.] = [clamp(y, 0, C-1) == c];  v = [y != ignore_index]
    TP = sum_pix p t v;  FP = sum_pix p (1 - t) v;  FN = sum_pix (1 - p) t v        all three masked, unlike Dice's den
    l[c] = mean_b (1 - (TP + smooth) / (TP + alpha FP + beta FN + smooth))
    loss = loss_weight / C * sum_{c != ignore_index} class_weight[c] * l[c]         the skipped channel counts in C"""
import torch
import torch.nn.functional as F

from seg_dice_oracle import dice_inputs  # noqa: F401  (the inputs of both families)


def _leaf(logit, label, dtype):
    z = logit.detach().to(dtype).requires_grad_(True)
    return z, F.interpolate(z, size=label.shape[-2:], mode='bilinear', align_corners=False)


def _per_class(x, C, dtype, default):
    if x is None:
        x = default
    if not torch.is_tensor(x) and not isinstance(x, (list, tuple)):
        return torch.full((C,), float(x), dtype=dtype)
    return (x.to(dtype) if torch.is_tensor(x) else torch.tensor(x, dtype=dtype)).reshape(C)


def focal_contract(logit, label, ignore_index=255, gamma=2.0, alpha=0.5, class_weight=None, reduction='mean', loss_weight=1.0,
                   dtype=torch.float64):
    """-> (loss 0-d, differentiable w.r.t. the returned leaf; the leaf (B,C,h,w) in `dtype`)."""
    z, u = _leaf(logit, label, dtype)
    B, C = z.shape[:2]
    t = (label.unsqueeze(1) == torch.arange(C).view(1, C, 1, 1)).to(dtype)
    v = (label != ignore_index).to(dtype).unsqueeze(1)
    a = _per_class(alpha, C, dtype, 0.5).view(1, C, 1, 1)
    cw = _per_class(class_weight, C, dtype, 1.0).view(1, C, 1, 1)
    s = torch.sigmoid(u)
    q = (1 - s) * t + s * (1 - t)
    e = F.binary_cross_entropy_with_logits(u, t, reduction='none') * (a * t + (1 - a) * (1 - t)) * q.pow(gamma) * cw * v
    total = e.sum()
    if reduction == 'mean':
        total = total / e.numel()
    return loss_weight * total, z


def tversky_contract(logit, label, ignore_index=255, alpha=0.3, beta=0.7, smooth=1.0, class_weight=None, loss_weight=1.0,
                     dtype=torch.float64):
    """-> (loss 0-d, differentiable w.r.t. the returned leaf; the leaf (B,C,h,w) in `dtype`)."""
    z, u = _leaf(logit, label, dtype)
    B, C = z.shape[:2]
    p = F.softmax(u, dim=1)
    t = F.one_hot(label.clamp(0, C - 1), C).permute(0, 3, 1, 2).to(dtype)
    v = (label != ignore_index).to(dtype).unsqueeze(1)
    tp = (p * t * v).flatten(2).sum(-1)
    fp = (p * (1 - t) * v).flatten(2).sum(-1)
    fn = ((1 - p) * t * v).flatten(2).sum(-1)
    per_class = (1 - (tp + smooth) / (tp + alpha * fp + beta * fn + smooth)).mean(0)
    cw = _per_class(class_weight, C, dtype, 1.0)
    keep = torch.ones(C, dtype=dtype)
    if 0 <= ignore_index < C:
        keep[ignore_index] = 0
    return loss_weight * (per_class * cw * keep).sum() / C, z


def _reference(contract, logit, label, scale, kw):
    loss, z = contract(logit, label, **kw)
    (loss * scale).backward()
    return float(loss.detach()), z.grad


def focal_reference(logit, label, scale=1.7, **kw):
    """-> (loss as a float, d(scale * loss) / d logit in fp64 (or kw['dtype']))."""
    return _reference(focal_contract, logit, label, scale, kw)


def tversky_reference(logit, label, scale=1.7, **kw):
    """-> (loss as a float, d(scale * loss) / d logit in fp64 (or kw['dtype']))."""
    return _reference(tversky_contract, logit, label, scale, kw)
