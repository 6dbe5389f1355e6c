"""fp64 torch restatement (test infrastructure only) of the Lovasz-softmax seg loss the fused kernels implement
(`ops.upsample_lovasz`: rscotr_upsample_lovasz_fwd / _bwd), written apart from the package: F.interpolate, softmax, a STABLE
descending torch.sort, cumulative sums; gradients come from autograd.

mmseg is not installed.  The contract below is restated from mmseg 0.28 `LovaszLoss(loss_type='multi_class')` as
`BaseDecodeHead.losses` reaches it AS REMEMBERED: parity with mmseg by reading, unpinned (as tests/seg_dice_oracle.py is).

With z = seg_logit (B,C,h,w), y = label (B,H,W) int64:
    u = bilinear_resize(z, (H,W), align_corners=False),  p = softmax(u, dim=1)
    P = the pixels with y != ignore_index in (b, y, x) order (of the batch, or of one image with per_image)
    for a summed class c:  fg_i = [y_i == c] (a label outside [0, C) is background for every class),  e_i = |fg_i - p_i,c|
        e sorted descending, equal errors in ascending pixel order;  G = sum fg;  F_k / Bk_k the foreground / background count
        among the first k + 1 sorted elements;  I_k = G - F_k,  U_k = G + Bk_k,  J_k = 1 - I_k / U_k,
        g_0 = J_0,  g_k = J_k - J_{k-1},  loss_c = sum_k e_(k) g_k
    classes='present': the classes with G > 0;  'all' / a list: all / the listed classes (an absent class costs max p_c)
    loss(P) = mean over the summed classes of class_weight[c] * loss_c;   0 when P is empty or no class is summed
    per_image=False: loss_weight * loss(batch);   per_image=True: loss_weight * mean | sum over the images of loss(image)
The Jaccard differences are taken in the oracle's dtype (fp64: no cancellation to speak of); g does not depend on p."""
import torch
import torch.nn.functional as F


def lovasz_inputs(B, C, h, w, H, W, ignore=255, ignored=0.05, seed=0):
    """Blocky labels (constant over 1 .. 8 pixel squares, as segmentation maps are) with a few per cent ignored, logits of
    the CE tests' magnitude, class weights in [0.25, 4.25).  -> (logit fp32, label int64, class_weight fp32)."""
    g = torch.Generator().manual_seed(1000 * seed + C * H + w + 17)
    logit = torch.randn(B, C, h, w, generator=g) * 3
    blk = max(1, min(8, H // 4, W // 4))
    coarse = torch.randint(0, C, (B, (H + blk - 1) // blk, (W + blk - 1) // blk), generator=g)
    label = coarse.repeat_interleave(blk, 1).repeat_interleave(blk, 2)[:, :H, :W].contiguous()
    label[torch.rand(B, H, W, generator=g) < ignored] = ignore
    cw = 0.25 + 4 * torch.rand(C, generator=g)
    return logit, label, cw


def lovasz_grad(fg_sorted):
    """The discrete gradient of the Jaccard index along the sorted order: fg_sorted (n,) of 0 / 1 -> g (n,)."""
    n = fg_sorted.numel()
    gts = fg_sorted.sum()
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (1 - fg_sorted).cumsum(0)
    jac = 1 - inter / union
    if n > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return jac


def lovasz_flat(probs, labels, classes='present', class_weight=None):
    """probs (n, C), labels (n,) of the valid pixels of one segment group -> its loss (0-d)."""
    n, C = probs.shape
    if n == 0:
        return probs.sum() * 0
    listed = list(range(C)) if isinstance(classes, str) else list(classes)
    losses = []
    for c in listed:
        fg = (labels == c).to(probs.dtype)
        if classes == 'present' and float(fg.sum()) == 0:
            continue
        err = (fg - probs[:, c]).abs()
        err_sorted, perm = torch.sort(err, dim=0, descending=True, stable=True)
        loss = torch.dot(err_sorted, lovasz_grad(fg[perm]))
        if class_weight is not None:
            loss = loss * class_weight[c]
        losses.append(loss)
    if not losses:
        return probs.sum() * 0
    return torch.stack(losses).mean()


def lovasz_contract(logit, label, ignore_index=255, classes='present', per_image=False, class_weight=None, reduction='none',
                    loss_weight=1.0, dtype=torch.float64):
    """-> (loss 0-d, differentiable w.r.t. the returned leaf; the leaf (B,C,h,w) in `dtype`)."""
    z = logit.detach().to(dtype).requires_grad_(True)
    B, C = z.shape[:2]
    p = F.softmax(F.interpolate(z, size=label.shape[-2:], mode='bilinear', align_corners=False), dim=1)
    cw = None if class_weight is None else torch.as_tensor(class_weight).to(dtype)

    def group(pb, lb):  # pb (b, C, H, W), lb (b, H, W)
        flat = pb.permute(0, 2, 3, 1).reshape(-1, C)
        lab = lb.reshape(-1)
        valid = lab != ignore_index
        return lovasz_flat(flat[valid], lab[valid], classes, cw)

    if per_image:
        assert reduction in ('mean', 'sum')
        per = torch.stack([group(p[b:b + 1], label[b:b + 1]) for b in range(B)])
        loss = per.mean() if reduction == 'mean' else per.sum()
    else:
        assert reduction == 'none'
        loss = group(p, label)
    return loss_weight * loss, z


def lovasz_reference(logit, label, ignore_index=255, classes='present', per_image=False, class_weight=None, reduction='none',
                     loss_weight=1.0, scale=1.7, dtype=torch.float64):
    """-> (loss as a float, d(scale * loss) / d logit in `dtype`)."""
    loss, z = lovasz_contract(logit, label, ignore_index, classes, per_image, class_weight, reduction, loss_weight, dtype)
    (loss * scale).backward()
    return float(loss.detach()), z.grad
