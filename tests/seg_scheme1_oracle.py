"""Reference of Mask2FormerHead scheme 1 (models/multi/seg_head/mask2former_head.py:118-125) in the reference's own order of
operations: cls_pred by F.linear, mask_pred by einsum('bqd,bdhw->bqhw'), then einsum('bqc,bqhw->bchw') — the (B,Q,h,w) mask
logits ARE formed here; csrc/seg_mix.hip re-associates the two products and never forms them.

    class_logits_ref     the two einsums in fp64 with their gradients (what ops.seg_class_logits computes)
    class_logits_sums    the sums of absolute values of the terms of every output's chain (for a rounding bound)
    seg_forward_scheme1  oracle.model.seg_forward with the scheme-1 tail: a drop-in for OM.seg_forward"""
import torch
import torch.nn.functional as F

from oracle import model as OM

_seg_forward = OM.seg_forward            # (bound at import: a test may point OM.seg_forward at seg_forward_scheme1)
_seg_forward_head = OM.seg_forward_head


def _einsums(cls, e, mf):
    B, P, D = mf.shape
    mask_pred = torch.einsum('bqd,bdhw->bqhw', e, mf.transpose(1, 2).reshape(B, D, P, 1))
    return torch.einsum('bqc,bqhw->bchw', cls, mask_pred).reshape(B, -1, P)


def class_logits_ref(cls, e, mf, g=None):
    """cls (B,Q,K), e (B,Q,D), mf (B,P,D) mask features in token layout, g (B,K,P) upstream gradient or None -> dict of fp64
    tensors on the inputs' device: seg (B,K,P) and, with g, dcls, de, dmf."""
    cls, e, mf = (t.detach().double().requires_grad_(g is not None) for t in (cls, e, mf))
    seg = _einsums(cls, e, mf)
    out = dict(seg=seg.detach())
    if g is not None:
        seg.backward(g.detach().double())
        out.update(dcls=cls.grad, de=e.grad, dmf=mf.grad)
    return out


def class_logits_sums(cls, e, mf, g):
    """Sum of |term| over the chain of every output, fp64:
        seg  sum_q sum_d |cls||e||mf|                 dmf  sum_k |g| sum_q |cls||e|
        dcls sum_d |e| sum_p |g||mf|                  de   sum_k |cls| sum_p |g||mf|"""
    c, e, m, g = (t.detach().double().abs() for t in (cls, e, mf, g))
    mix = torch.einsum('bqk,bqd->bkd', c, e)
    dmix = torch.einsum('bkp,bpd->bkd', g, m)
    return dict(seg=torch.einsum('bkd,bpd->bkp', mix, m), dmf=torch.einsum('bkp,bkd->bpd', g, mix),
                dcls=torch.einsum('bqd,bkd->bqk', e, dmix), de=torch.einsum('bqk,bkd->bqd', c, dmix))


def seg_forward_scheme1(neck_feats, P, cfg, enc_layers, inject_masks=None):
    """-> (seg_mask (B, num_classes + 1, h, w), masks) like oracle.model.seg_forward: the same decoder (every forward_head
    call produces mask_pred and the next attention mask as in scheme 2), and on the last call's post-norm output
    cls_pred = cls_embed(.), seg_mask = einsum('bqc,bqhw->bchw', cls_pred, mask_pred)."""
    last = {}

    def head(dec_out, mask_feature, target_size, P_, heads=8):
        last['dec_out'] = dec_out
        return _seg_forward_head(dec_out, mask_feature, target_size, P_, heads)

    OM.seg_forward_head = head
    try:
        mask_pred, masks = _seg_forward(neck_feats, P, cfg, enc_layers, inject_masks=inject_masks)
    finally:
        OM.seg_forward_head = _seg_forward_head
    d = OM._ln(last['dec_out'], P, 'seg_head.transformer_decoder.post_norm').transpose(0, 1)
    cls_pred = F.linear(d, P['seg_head.cls_embed.weight'], P['seg_head.cls_embed.bias'])
    return torch.einsum('bqc,bqhw->bchw', cls_pred, mask_pred), masks
