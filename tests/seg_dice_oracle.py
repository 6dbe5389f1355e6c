"""fp64 torch restatement (test infrastructure only) of the Dice seg loss the fused kernels implement
(`ops.upsample_dice`: rscotr_upsample_dice_fwd / _bwd), written apart from the package: F.interpolate, softmax, the sums;
gradients come from autograd.

mmseg is not installed.  The contract below is restated from mmseg 0.28 `DiceLoss` as `BaseDecodeHead.losses` reaches it AS
REMEMBERED: parity with mmseg by reading, unpinned (as tests/randaug_oracle.py is for mmcls).

With z = seg_logit (B,C,h,w), y = label (B,H,W) int64:
    u        = bilinear_resize(z, (H,W), align_corners=False)
    p        = softmax(u, dim=1)
    t[b,c,.] = [clamp(y, 0, C-1) == c]                  one-hot of the CLAMPED label: an ignored 255 lands in channel C-1
    v[b,.]   = [y != ignore_index]                      DiceLoss's OWN ignore_index
    num[b,c] = 2 * sum_pix p t v + smooth               masked by v
    den[b,c] = sum_pix (p^2 + t) + smooth               NOT masked by v (mmseg's quirk, kept); exponent 2
    l[c]     = mean_b (1 - num[b,c] / den[b,c])
    loss     = loss_weight * sum_{c != ignore_index} class_weight[c] * l[c] / C      (the skipped channel counts in the divisor)
`reduction` and `avg_factor` act on a scalar in mmseg: they change nothing and are not parameters here."""
import torch
import torch.nn.functional as F


def dice_inputs(B, C, h, w, H, W, ignore=255, ignored=0.05, seed=0):
    """Blocky labels (constant over 1 .. 8 pixel squares, as segmentation maps are) with a few per cent ignored, logits of
    the CE tests' magnitude, class weights in [0.25, 4.25).  -> (logit fp32, label int64, class_weight fp32)."""
    g = torch.Generator().manual_seed(1000 * seed + C * H + w)
    logit = torch.randn(B, C, h, w, generator=g) * 3
    blk = max(1, min(8, H // 4, W // 4))
    coarse = torch.randint(0, C, (B, (H + blk - 1) // blk, (W + blk - 1) // blk), generator=g)
    label = coarse.repeat_interleave(blk, 1).repeat_interleave(blk, 2)[:, :H, :W].contiguous()
    label[torch.rand(B, H, W, generator=g) < ignored] = ignore
    cw = 0.25 + 4 * torch.rand(C, generator=g)
    return logit, label, cw


def dice_contract(logit, label, ignore_index=255, smooth=1.0, class_weight=None, loss_weight=1.0, dtype=torch.float64):
    """-> (loss 0-d, differentiable w.r.t. the returned leaf; the leaf (B,C,h,w) in `dtype`)."""
    z = logit.detach().to(dtype).requires_grad_(True)
    B, C = z.shape[:2]
    p = F.softmax(F.interpolate(z, size=label.shape[-2:], mode='bilinear', align_corners=False), dim=1)
    t = F.one_hot(label.clamp(0, C - 1), C).permute(0, 3, 1, 2).to(dtype)
    v = (label != ignore_index).to(dtype).unsqueeze(1)
    num = 2 * (p * t * v).flatten(2).sum(-1) + smooth
    den = (p * p + t).flatten(2).sum(-1) + smooth
    per_class = (1 - num / den).mean(0)
    cw = torch.ones(C, dtype=dtype) if class_weight is None else torch.as_tensor(class_weight).to(dtype)
    keep = torch.ones(C, dtype=dtype)
    if 0 <= ignore_index < C:
        keep[ignore_index] = 0
    return loss_weight * (per_class * cw * keep).sum() / C, z


def dice_reference(logit, label, ignore_index=255, smooth=1.0, class_weight=None, loss_weight=1.0, scale=1.7,
                   dtype=torch.float64):
    """-> (loss as a float, d(scale * loss) / d logit in `dtype`)."""
    loss, z = dice_contract(logit, label, ignore_index, smooth, class_weight, loss_weight, dtype)
    (loss * scale).backward()
    return float(loss.detach()), z.grad
