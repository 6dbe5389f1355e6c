"""Segmentation decoder (`type='Mask2FormerHead'` + `MlvlSegPixelDecoder`) over the shared encoder.

Mirrors models/multi/seg_head/pixel_decoder.py:14-170 and mask2former_head.py:18-208 (plus
mmseg 0.28 `BaseDecodeHead.losses` reached at mask2former_head.py:204) with the reference's
parameter names.  Tokens are batch-first.
"""
import copy

import torch
import torch.nn as nn

from . import ops
from .layers import LevelGeometry
from .registry import MODELS


@MODELS.register_module()
class CrossEntropyLoss(nn.Module):
    """mmseg CrossEntropyLoss as the seg head uses it: the options are stored here and applied by the fused kernels
    (ops.upsample_ce / ops.upsample_ce_weighted).  class_weight: a list / tuple of floats or the path of a .npy file, one
    entry per logit channel (checked at the first call)."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0,
                 loss_name='loss_ce', avg_non_ignore=False):
        super().__init__()
        if use_sigmoid or use_mask:
            raise NotImplementedError('CrossEntropyLoss: use_sigmoid / use_mask are not implemented (softmax CE only)')
        if reduction not in ('mean', 'sum'):
            raise NotImplementedError(f"CrossEntropyLoss: reduction={reduction!r} (only 'mean' and 'sum')")
        self.reduction, self.class_weight, self.avg_non_ignore = reduction, _class_weight_list(class_weight), bool(avg_non_ignore)
        self.loss_weight, self.loss_name = loss_weight, loss_name
        self._cw = {}  # device -> tensor (not a buffer: the state dict keeps the reference's keys)

    @property
    def is_default(self):
        return self.class_weight is None and not self.avg_non_ignore and self.reduction == 'mean'

    def weight_on(self, device, num_channels):
        return _class_weight_on(self, device, num_channels)


def _class_weight_list(class_weight):
    """mmseg get_class_weight: None, a list / tuple of floats, or the path of a .npy file -> None or a list of floats."""
    if isinstance(class_weight, str):
        if not class_weight.endswith('.npy'):
            raise ValueError(f'class_weight file {class_weight!r}: only .npy is read')
        import numpy as np
        return np.load(class_weight).astype('float64').reshape(-1).tolist()
    if isinstance(class_weight, (list, tuple)):
        return [float(v) for v in class_weight]
    if class_weight is not None:
        raise TypeError(f'class_weight must be a list / tuple of floats or a .npy path, got {type(class_weight).__name__}')
    return None


def _class_weight_on(loss, device, num_channels):
    """The loss module's class weights as a tensor on `device` (cached per device), checked against the logit channels."""
    if loss.class_weight is None:
        return None
    if len(loss.class_weight) != num_channels:
        raise ValueError(f'class_weight has {len(loss.class_weight)} entries, the logits have {num_channels} channels')
    t = loss._cw.get(str(device))
    if t is None:
        t = loss._cw[str(device)] = torch.tensor(loss.class_weight, dtype=torch.float32, device=device)
    return t


@MODELS.register_module()
class DiceLoss(nn.Module):
    """mmseg 0.28 DiceLoss as the seg head uses it: the options are stored here and applied by the fused kernels
    (ops.upsample_dice).  As in mmseg, forward swallows the `weight` and `ignore_index` that BaseDecodeHead.losses passes: a
    pixel sampler's mask and the head's ignore_index do not reach this loss; its OWN ignore_index masks the numerator and
    skips that channel.  reduction / avg_factor act on a scalar: 'mean', 'sum' and 'none' are the same loss.  No parameters,
    no buffers: the state dict keeps the reference's keys."""

    def __init__(self, smooth=1, exponent=2, reduction='mean', class_weight=None, loss_weight=1.0, ignore_index=255,
                 loss_name='loss_dice'):
        super().__init__()
        if exponent != 2:
            raise NotImplementedError(f'DiceLoss: exponent={exponent!r} (the fused kernels implement exponent 2)')
        if reduction not in ('mean', 'sum', 'none'):
            raise ValueError(f"DiceLoss: reduction={reduction!r} (one of 'mean', 'sum', 'none')")
        self.smooth, self.exponent, self.reduction = float(smooth), 2, reduction
        self.class_weight = _class_weight_list(class_weight)
        self.loss_weight, self.ignore_index, self.loss_name = float(loss_weight), int(ignore_index), loss_name
        self._cw = {}

    def weight_on(self, device, num_channels):
        return _class_weight_on(self, device, num_channels)

    def forward(self, seg_logit, label, **kwargs):
        """seg_logit (B,C,h,w) at the head's resolution, label (B,H,W) int64 -> loss_weight * dice (0-d)."""
        cw = self.weight_on(seg_logit.device, seg_logit.shape[1])
        return ops.upsample_dice(seg_logit, label, self.ignore_index, smooth=self.smooth, class_weight=cw,
                                 loss_weight=self.loss_weight)


@MODELS.register_module()
class TverskyLoss(nn.Module):
    """mmseg 0.28 TverskyLoss as the seg head uses it: the options are stored here and applied by the fused kernels
    (ops.upsample_tversky).  Like DiceLoss, forward swallows the `weight` and `ignore_index` that BaseDecodeHead.losses passes: a
    pixel sampler's mask and the head's ignore_index do not reach this loss; its OWN ignore_index masks the three sums and skips
    that channel.  No parameters, no buffers: the state dict keeps the reference's keys."""

    def __init__(self, smooth=1, class_weight=None, loss_weight=1.0, ignore_index=255, alpha=0.3, beta=0.7,
                 loss_name='loss_tversky'):
        super().__init__()
        if alpha + beta != 1.0:
            raise ValueError(f'TverskyLoss: alpha + beta must be 1.0, got {alpha} + {beta}')
        if not smooth > 0:
            raise ValueError(f'TverskyLoss: smooth={smooth!r} (> 0: an all-ignored image would be 0 / 0)')
        self.smooth, self.alpha, self.beta = float(smooth), float(alpha), float(beta)
        self.class_weight = _class_weight_list(class_weight)
        self.loss_weight, self.ignore_index, self.loss_name = float(loss_weight), int(ignore_index), loss_name
        self._cw = {}

    def weight_on(self, device, num_channels):
        return _class_weight_on(self, device, num_channels)

    def forward(self, seg_logit, label, **kwargs):
        """seg_logit (B,C,h,w) at the head's resolution, label (B,H,W) int64 -> loss_weight * tversky (0-d)."""
        cw = self.weight_on(seg_logit.device, seg_logit.shape[1])
        return ops.upsample_tversky(seg_logit, label, self.ignore_index, alpha=self.alpha, beta=self.beta, smooth=self.smooth,
                                    class_weight=cw, loss_weight=self.loss_weight)


class FocalLoss(nn.Module):
    """mmseg 0.28 FocalLoss (the sigmoid form) as the seg head uses it: the options are stored here and applied by the fused
    kernels (ops.upsample_focal) with the HEAD's ignore_index, as BaseDecodeHead.losses passes it.  alpha: a float or a list of
    one float per logit channel; class_weight as CrossEntropyLoss takes it.  Not in MODELS: that name is the det head's mmdet
    holder (det_head.FocalLoss); the seg head resolves its loss_decode entries through _SEG_LOSSES.  No parameters, no buffers."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.5, reduction='mean', class_weight=None, loss_weight=1.0,
                 loss_name='loss_focal'):
        super().__init__()
        if not use_sigmoid:
            raise NotImplementedError('FocalLoss: use_sigmoid=False is not implemented (mmseg supports the sigmoid form only)')
        if reduction not in ('mean', 'sum'):
            raise NotImplementedError(f"FocalLoss: reduction={reduction!r} (only 'mean' and 'sum')")
        if not gamma >= 0:
            raise ValueError(f'FocalLoss: gamma must be >= 0, got {gamma}')
        if isinstance(alpha, (list, tuple)):
            alpha = [float(v) for v in alpha]
        elif isinstance(alpha, (int, float)) and not isinstance(alpha, bool):
            alpha = float(alpha)
        else:
            raise TypeError(f'FocalLoss: alpha must be a float or a list of floats, got {type(alpha).__name__}')
        self.gamma, self.alpha, self.reduction = float(gamma), alpha, reduction
        self.class_weight = _class_weight_list(class_weight)
        self.loss_weight, self.loss_name = float(loss_weight), loss_name
        self._cw, self._alpha = {}, {}

    def weight_on(self, device, num_channels):
        return _class_weight_on(self, device, num_channels)

    def alpha_on(self, device, num_channels):
        """The scalar alpha, or the per-class list as a tensor on `device` (cached per device), checked against the channels."""
        if not isinstance(self.alpha, list):
            return self.alpha
        if len(self.alpha) != num_channels:
            raise ValueError(f'alpha has {len(self.alpha)} entries, the logits have {num_channels} channels')
        t = self._alpha.get(str(device))
        if t is None:
            t = self._alpha[str(device)] = torch.tensor(self.alpha, dtype=torch.float32, device=device)
        return t

    def forward(self, seg_logit, label, ignore_index=255, **kwargs):
        """seg_logit (B,C,h,w) at the head's resolution, label (B,H,W) int64 -> loss_weight * focal (0-d)."""
        C = seg_logit.shape[1]
        return ops.upsample_focal(seg_logit, label, ignore_index, gamma=self.gamma, alpha=self.alpha_on(seg_logit.device, C),
                                  class_weight=self.weight_on(seg_logit.device, C), reduction=self.reduction,
                                  loss_weight=self.loss_weight)


@MODELS.register_module()
class LovaszLoss(nn.Module):
    """mmseg 0.28 LovaszLoss, loss_type='multi_class', as the seg head uses it: the options are stored here and applied by the
    fused kernels (ops.upsample_lovasz) with the HEAD's ignore_index, as BaseDecodeHead.losses passes it (like FocalLoss); the
    sampler's `weight` is swallowed, as mmseg's Lovasz ignores it (like DiceLoss).  classes: 'present', 'all' or a list of class
    indices; per_image=False takes reduction='none' (mmseg's constructor asserts the same, so the default-argument
    dict(type='LovaszLoss') is refused), per_image=True takes 'mean' or 'sum' over the images.
    Memory: the device sort holds two ping-pong (key, payload) pairs and the gradient plane per summed class slot, 20 bytes per
    (slot, pixel): 73 MB at 7 classes and 2 x 512 x 512, about 1 GB at a 100-channel head unless `classes` lists the few classes
    to sum (classes=[0, 1, 2, 3, 4, 5]: 63 MB).  No parameters, no buffers: the state dict keeps the reference's keys."""

    def __init__(self, loss_type='multi_class', classes='present', per_image=False, reduction='mean', class_weight=None,
                 loss_weight=1.0, loss_name='loss_lovasz'):
        super().__init__()
        if loss_type != 'multi_class':
            raise NotImplementedError(f"LovaszLoss: loss_type={loss_type!r} (only 'multi_class': the binary hinge form is not "
                                      'implemented)')
        if reduction not in ('mean', 'sum', 'none'):
            raise ValueError(f"LovaszLoss: reduction={reduction!r} (one of 'mean', 'sum', 'none')")
        if per_image and reduction == 'none':
            raise NotImplementedError("LovaszLoss: per_image=True with reduction='none' is a vector loss (only 'mean' and 'sum')")
        if not per_image and reduction != 'none':
            raise NotImplementedError(f"LovaszLoss: per_image=False with reduction={reduction!r}: mmseg's own constructor "
                                      "asserts there; write reduction='none' or per_image=True")
        if isinstance(classes, str):
            if classes not in ('present', 'all'):
                raise ValueError(f"LovaszLoss: classes={classes!r} ('present', 'all' or a list of class indices)")
        elif isinstance(classes, (list, tuple)) and classes and all(isinstance(c, int) and not isinstance(c, bool) for c in classes):
            classes = [int(c) for c in classes]
            if len(set(classes)) != len(classes) or min(classes) < 0:
                raise ValueError(f'LovaszLoss: classes={classes!r} must be distinct non-negative class indices')
        else:
            raise TypeError(f"LovaszLoss: classes must be 'present', 'all' or a non-empty list of ints, got {classes!r}")
        self.loss_type, self.classes, self.per_image, self.reduction = loss_type, classes, bool(per_image), reduction
        self.class_weight = _class_weight_list(class_weight)
        self.loss_weight, self.loss_name = float(loss_weight), loss_name
        self._cw = {}

    def weight_on(self, device, num_channels):
        return _class_weight_on(self, device, num_channels)

    def forward(self, seg_logit, label, ignore_index=255, **kwargs):
        """seg_logit (B,C,h,w) at the head's resolution, label (B,H,W) int64 -> loss_weight * lovasz (0-d)."""
        cw = self.weight_on(seg_logit.device, seg_logit.shape[1])
        return ops.upsample_lovasz(seg_logit, label, ignore_index, classes=self.classes, per_image=self.per_image,
                                   class_weight=cw, reduction=self.reduction, loss_weight=self.loss_weight)


# the types a seg head's loss_decode entries resolve to (every one but the first as an entry of a list only)
_SEG_LOSSES = {'CrossEntropyLoss': CrossEntropyLoss, 'DiceLoss': DiceLoss, 'FocalLoss': FocalLoss, 'TverskyLoss': TverskyLoss,
               'LovaszLoss': LovaszLoss}


def _build_seg_loss(cfg):
    args = copy.deepcopy(dict(cfg))
    return _SEG_LOSSES[args.pop('type')](**args)


@MODELS.register_module()
class OHEMPixelSampler:
    """mmseg OHEMPixelSampler with a probability threshold: keep the non-ignored pixels whose label probability is below
    max(thresh, the (min_kept * batch)-th smallest one).  The selection runs on the device inside ops.upsample_ce_weighted."""

    def __init__(self, context=None, thresh=0.7, min_kept=100000):
        if thresh is None:
            raise NotImplementedError('OHEMPixelSampler: the loss-ranked variant (thresh=None) is not implemented')
        if min_kept < 0:
            raise ValueError(f'OHEMPixelSampler: min_kept must be >= 0, got {min_kept}')
        self.thresh, self.min_kept = float(thresh), int(min_kept)


@MODELS.register_module()
class MlvlSegPixelDecoder(nn.Module):
    def __init__(self, num_encoder_levels=4, in_channels=(256, 512, 1024, 2048), strides=(4, 8, 16, 32),
                 feat_channels=256, out_channels=256, num_outs=3, norm_cfg=dict(type='GN', num_groups=32),
                 act_cfg=dict(type='ReLU'), positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
                 init_cfg=None):
        super().__init__()
        self.strides = list(strides)
        self.num_input_levels = len(in_channels)
        self.num_encoder_levels = num_encoder_levels
        assert self.num_input_levels == self.num_encoder_levels, \
            'the MTL configs feed every level through the shared encoder (empty FPN branch)'
        self.postional_encoding = MODELS.build(positional_encoding)
        self.level_encoding = nn.Embedding(num_encoder_levels, feat_channels)
        self.lateral_convs = nn.ModuleList()
        self.output_convs = nn.ModuleList()
        self.mask_feature = nn.Conv2d(feat_channels, out_channels, kernel_size=1, stride=1, padding=0)
        self.num_outs = num_outs
        self._pe_cache = {}

    def init_weights(self):
        nn.init.kaiming_uniform_(self.mask_feature.weight, a=1)  # caffe2_xavier_init
        nn.init.constant_(self.mask_feature.bias, 0)
        nn.init.normal_(self.level_encoding.weight, mean=0, std=1)

    def forward(self, encoder, neck_feats, backbone_feats):
        B = backbone_feats[0].shape[0]
        device = neck_feats[0].device
        inputs, shapes, refs = [], [], []
        for i in range(self.num_encoder_levels):
            level_idx = self.num_input_levels - i - 1  # low -> high resolution
            f = neck_feats[level_idx]
            h, w = f.shape[-2:]
            inputs.append(f.flatten(2).transpose(1, 2))
            shapes.append((h, w))
            refs.append(_grid_refs(h, w, self.strides[level_idx], device))
        x = torch.cat(inputs, 1)
        # level_encoding.weight[i] + positional encoding per level, concatenated (pixel_decoder.py:108-118): one launch
        # over the token-layout encoding of the level shapes (a constant)
        pkey = (tuple(shapes), str(device))
        pe_tok = self._pe_cache.get(pkey)
        if pe_tok is None:
            pe_tok = self._pe_cache[pkey] = torch.cat(
                [self.postional_encoding.unpadded(1, h, w, device).flatten(2).transpose(1, 2) for h, w in shapes], 1).contiguous()
        pos = ops.level_embed_add(None, self.level_encoding.weight, [h * w for h, w in shapes], const=pe_tok, batch=B)
        geom = LevelGeometry.get(shapes, device)
        # (a constant of the level shapes and the batch size: materialised once — every encoder layer's sampling kernel wants
        # it dense, and an expanded view would be copied by each of them)
        rkey = (tuple(shapes), B, str(device), 'ref')
        ref = self._pe_cache.get(rkey)
        if ref is None:
            ref = self._pe_cache[rkey] = torch.cat(refs, 0)[None, :, None].expand(B, -1, self.num_encoder_levels, -1).contiguous()
        # the reference passes an all-False padding mask: value.masked_fill is the identity
        memory = encoder(x, None, None, query_pos=pos, query_key_padding_mask=None, reference_points=ref,
                         **geom.kwargs())
        # one split (its backward is ONE concatenation; slicing level by level costs a full-size zero-fill + copy per level
        # and an add per level in backward)
        levels = torch.split(memory, [h * w for h, w in shapes], dim=1)
        outs = [ops.tokens_to_map(lv, hw) for lv, hw in zip(levels, shapes)]  # channels-last views
        multi_scale_features = outs[:self.num_outs]
        # 1x1 conv = MFMA GEMM on the tokens of the finest level
        h, w = shapes[-1]
        mf = ops.linear(levels[-1], self.mask_feature.weight.view(self.mask_feature.weight.shape[0], -1), self.mask_feature.bias, range_out=False)
        mask_feature = ops.tokens_to_map(mf, (h, w))
        return mask_feature, multi_scale_features


_ref_cache = {}


def _grid_refs(h, w, stride, device):
    """MlvlPointGenerator.single_level_grid_priors (offset 0.5) / (w*stride, h*stride)."""
    key = (h, w, stride, str(device))
    r = _ref_cache.get(key)
    if r is None:
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device),
                                torch.arange(w, dtype=torch.float32, device=device), indexing='ij')
        pts = torch.stack([(xs.reshape(-1) + 0.5) * stride, (ys.reshape(-1) + 0.5) * stride], -1)
        r = pts / (torch.tensor([[w, h]], dtype=torch.float32, device=device) * stride)
        _ref_cache[key] = r
    return r


@MODELS.register_module()
class Mask2FormerHead(nn.Module):
    def __init__(self, in_channels, feat_channels, out_channels, num_classes=5, num_queries=100,
                 num_transformer_feat_level=4, scheme=1, pixel_decoder=None, enforce_decoder_input_project=False,
                 transformer_decoder=None, positional_encoding=None, ignore_index=255,
                 loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), align_corners=False,
                 init_cfg=None, sampler=None):
        super().__init__()
        if scheme not in (1, 2):
            raise NotImplementedError(f'Mask2FormerHead: scheme={scheme!r} (1: class logits mixed from the queries, 2: the queries are '
                                      'the output channels)')
        assert not align_corners
        self.scheme, self.num_classes, self.num_queries = scheme, num_classes, num_queries
        self.align_corners, self.ignore_index = align_corners, ignore_index
        self.num_transformer_feat_level = num_transformer_feat_level
        attn_cfgs = transformer_decoder['transformerlayers']['attn_cfgs']
        self.num_heads = (attn_cfgs[0] if isinstance(attn_cfgs, (list, tuple)) else attn_cfgs)['num_heads']
        self.num_transformer_decoder_layers = transformer_decoder['num_layers']
        pd = copy.deepcopy(dict(pixel_decoder))
        pd.update(in_channels=in_channels, feat_channels=feat_channels, out_channels=out_channels)
        self.pixel_decoder = MODELS.build(pd)
        self.transformer_decoder = MODELS.build(transformer_decoder)
        self.decoder_embed_dims = self.transformer_decoder.embed_dims
        assert self.decoder_embed_dims == feat_channels and not enforce_decoder_input_project
        self.decoder_input_projs = nn.ModuleList([nn.Identity() for _ in range(num_transformer_feat_level)])
        self.decoder_positional_encoding = MODELS.build(positional_encoding)
        self.query_embed = nn.Embedding(num_queries, feat_channels)
        self.query_feat = nn.Embedding(num_queries, feat_channels)
        self.level_embed = nn.Embedding(num_transformer_feat_level, feat_channels)
        if scheme == 1:  # mask2former_head.py:78-79 (num_classes + 1 channels; init_weights leaves it at nn.Linear's default)
            self.cls_embed = nn.Linear(feat_channels, num_classes + 1)
        self.mask_embed = nn.Sequential(
            nn.Linear(feat_channels, feat_channels), nn.ReLU(inplace=True),
            nn.Linear(feat_channels, feat_channels), nn.ReLU(inplace=True),
            nn.Linear(feat_channels, out_channels))
        # a dict or a list of dicts, as mmseg's BaseDecodeHead takes it (mask2former_head.py:85-93); no parameters, no keys
        # The single-dict form stays what it was, one CrossEntropyLoss; a DiceLoss is an entry of a loss_decode LIST (next to a
        # CrossEntropyLoss entry as in mmseg's documented pair, or on its own: [dict(type='DiceLoss')])
        # FocalLoss, TverskyLoss and LovaszLoss are list entries like DiceLoss.  The entry types resolve through _SEG_LOSSES: 'FocalLoss' in
        # MODELS is the det head's holder
        is_list = isinstance(loss_decode, (list, tuple))
        cfgs = list(loss_decode) if is_list else [loss_decode]
        allowed = tuple(_SEG_LOSSES) if is_list else ('CrossEntropyLoss',)
        for c in cfgs:
            if not isinstance(c, dict) or c.get('type') not in allowed:
                name = c.get('type') if isinstance(c, dict) else type(c).__name__
                if name in _SEG_LOSSES:
                    raise NotImplementedError(f"loss_decode type {name!r} as a single dict: {name} is taken as an entry of a "
                                              f"loss_decode list, e.g. [dict(type='CrossEntropyLoss'), dict(type={name!r})]")
                raise NotImplementedError(f'loss_decode type {name!r}: the fused seg losses implement CrossEntropyLoss, and DiceLoss, '
                                          'FocalLoss, TverskyLoss and LovaszLoss as entries of a list, only')
        built = [_build_seg_loss(c) for c in cfgs]
        self.loss_decode = nn.ModuleList(built) if isinstance(loss_decode, (list, tuple)) else built[0]
        if sampler is not None and any(isinstance(ld, FocalLoss) for ld in built):
            # (mmseg hands the sampler's (B,H,W) weight to a (B*H*W, C) loss and fails there itself)
            raise NotImplementedError('a pixel sampler with a FocalLoss entry in loss_decode: mmseg cannot apply the sampler\'s '
                                      'per-pixel weight to the per-class focal loss')
        self.sampler = None
        if sampler is not None:
            if not isinstance(sampler, dict) or sampler.get('type') != 'OHEMPixelSampler':
                name = sampler.get('type') if isinstance(sampler, dict) else type(sampler).__name__
                raise NotImplementedError(f'sampler type {name!r}: only OHEMPixelSampler is implemented')
            self.sampler = MODELS.build(sampler)

    def init_weights(self):
        self.pixel_decoder.init_weights()
        for p in self.transformer_decoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_normal_(p)

    def forward_head(self, decoder_out, mask_feature, attn_mask_target_size):
        """decoder_out (B,Q,C) -> (mask_pred (B,Q,h,w), attn_mask bool (B,Q,hw_next))."""
        pn = self.transformer_decoder.post_norm
        d = ops.layer_norm(decoder_out, pn.weight, pn.bias)
        m = self.mask_embed
        e = ops.mlp(d, [(m[0].weight, m[0].bias), (m[2].weight, m[2].bias), (m[4].weight, m[4].bias)], act='relu', range_out=False)  # (read by the mask-logit products on the fp32 pipe)
        B_, C_, h_, w_ = mask_feature.shape
        # einsum('bqd,bdhw->bqhw') on the token view of the mask features (channels-last map: free) -> MFMA GEMM
        mask_pred = ops.mask_logits(e, mask_feature.permute(0, 2, 3, 1).reshape(B_, h_ * w_, C_)).view(B_, -1, h_, w_)
        attn_mask = ops.seg_attn_mask(mask_pred, attn_mask_target_size, self.num_heads)
        return mask_pred, attn_mask

    def forward_class_logits(self, decoder_out, mask_feature):
        """Scheme 1, the last prediction (mask2former_head.py:118-125): decoder_out (B,Q,C) -> seg logits (B,K,h,w),
        K = num_classes + 1.  einsum('bqc,bqhw->bchw', cls_pred, mask_pred) without mask_pred: ops.seg_class_logits mixes the mask
        embeddings into K rows first and passes over the mask features once.  No attention mask either: nothing reads it."""
        pn = self.transformer_decoder.post_norm
        d = ops.layer_norm(decoder_out, pn.weight, pn.bias)
        m = self.mask_embed
        e = ops.mlp(d, [(m[0].weight, m[0].bias), (m[2].weight, m[2].bias), (m[4].weight, m[4].bias)], act='relu', range_out=False)
        cls_pred = ops.linear(d, self.cls_embed.weight, self.cls_embed.bias, range_out=False)
        B_, C_, h_, w_ = mask_feature.shape
        # (the channels-last map is a view of the pixel decoder's token tensor: flattening it back is free)
        seg = ops.seg_class_logits(cls_pred, e, mask_feature.permute(0, 2, 3, 1).reshape(B_, h_ * w_, C_))
        return seg.view(B_, -1, h_, w_)

    def forward(self, encoder, neck_feats, backbone_feats, img_metas, record=None):
        B = len(img_metas)
        device = neck_feats[0].device
        mask_features, memorys = self.pixel_decoder(encoder, neck_feats, backbone_feats)
        dec_in, dec_pos = [], []
        for i in range(self.num_transformer_feat_level):
            m = memorys[i]
            # (the map is a channels-last view of this level's rows of the encoder memory: read in place, batch-strided)
            dec_in.append(ops.level_embed_add(m.flatten(2).transpose(1, 2), self.level_embed.weight,
                                              [m.shape[-2] * m.shape[-1]], row0=i))
            dec_pos.append(self.decoder_positional_encoding.unpadded(B, m.shape[-2], m.shape[-1], device)
                           .flatten(2).transpose(1, 2))
        query_feat = ops.batch_param(self.query_feat.weight, B)
        query_embed = ops.batch_param(self.query_embed.weight, B)
        mask_pred, attn_mask = self.forward_head(query_feat, mask_features, memorys[0].shape[-2:])
        if record is not None:
            record['attn_masks'] = []
        nlay = self.num_transformer_decoder_layers
        # query_embed feeds both attentions of every layer: one handle each (their gradients are summed by ops.fan_out's
        # backward in 3 launches instead of 17 pairwise adds)
        n_att = len(self.transformer_decoder.layers[0].attentions)
        qe = ops.fan_out(query_embed, nlay * n_att)
        # key + key_pos of a level is the same for every layer that attends to it: formed once per level (values only; the
        # attention's backward still returns d(key)); query + query_embed leaves the previous layer's last norm
        key_sums = [torch.add(k.detach(), p) for k, p in zip(dec_in, dec_pos)]
        q_sum = None
        for i in range(nlay):
            li = i % self.num_transformer_feat_level
            layer = self.transformer_decoder.layers[i]
            query_embed = tuple(qe[i * n_att:(i + 1) * n_att])
            if record is not None:  # in the reference's (B*heads, Q, hw) form
                record['attn_masks'].append(attn_mask.unsqueeze(1).expand(-1, self.num_heads, -1, -1).flatten(0, 1))
            nxt = qe[(i + 1) * n_att] if i + 1 < nlay else None
            query_feat = layer(query_feat, dec_in[li], dec_in[li], query_pos=query_embed, key_pos=dec_pos[li],
                               attn_masks=[attn_mask, None], query_key_padding_mask=None, key_padding_mask=None,
                               query_sum=q_sum, key_sum=key_sums[li], next_query_pos=nxt)
            if nxt is not None:
                query_feat, q_sum = query_feat
            if self.scheme == 1 and nxt is None:
                return self.forward_class_logits(query_feat, mask_features)
            mask_pred, attn_mask = self.forward_head(
                query_feat, mask_features, memorys[(i + 1) % self.num_transformer_feat_level].shape[-2:])
        return mask_pred  # only the last prediction is supervised (mask2former_head.py:199)

    def forward_test(self, neck_feats, backbone_feats, img_metas, shared_encoder):
        """mask2former_head.py:207-209."""
        return self(shared_encoder, neck_feats, backbone_feats, img_metas)

    def losses(self, seg_logit, seg_label):
        entries = list(self.loss_decode) if isinstance(self.loss_decode, nn.ModuleList) else [self.loss_decode]
        ce = [ld for ld in entries if isinstance(ld, CrossEntropyLoss)]
        if len(ce) == len(entries):
            return self._ce_losses(ce, seg_logit, seg_label)
        # a list with DiceLoss / TverskyLoss / FocalLoss / LovaszLoss entries: the cross-entropy entries take the path they take
        # alone; every other entry is one fused call (the sampler's mask and the head's ignore_index do not reach a Dice or
        # Tversky entry, as in mmseg; a Focal or Lovasz entry takes the head's ignore_index); entries of one name add up
        out = self._ce_losses(ce, seg_logit, seg_label) if ce else {}
        acc_seg = out.pop('acc_seg', None)
        label = seg_label.squeeze(1)
        for ld in entries:
            if isinstance(ld, (DiceLoss, TverskyLoss, FocalLoss, LovaszLoss)):
                loss = ld(seg_logit, label, ignore_index=self.ignore_index)
                out[ld.loss_name] = out[ld.loss_name] + loss if ld.loss_name in out else loss
        if acc_seg is None:  # no cross-entropy entry: mmseg reports the accuracy all the same
            with torch.no_grad():
                _, acc_seg = ops.upsample_ce(seg_logit.detach(), label, self.ignore_index)
        out['acc_seg'] = acc_seg
        return out

    def _ce_losses(self, entries, seg_logit, seg_label):
        if self.sampler is None and len(entries) == 1 and entries[0].is_default:
            loss, acc = ops.upsample_ce(seg_logit, seg_label.squeeze(1), self.ignore_index)
            return {entries[0].loss_name: loss * entries[0].loss_weight, 'acc_seg': acc}
        # any option set: one fused call per entry (entries of one name add up, as in BaseDecodeHead.losses)
        label = seg_label.squeeze(1)
        ohem = None if self.sampler is None else (self.sampler.thresh, self.sampler.min_kept)
        out, acc_seg = {}, None
        for ld in entries:
            loss, acc, _ = ops.upsample_ce_weighted(
                seg_logit, label, self.ignore_index, class_weight=ld.weight_on(seg_logit.device, seg_logit.shape[1]),
                avg_non_ignore=ld.avg_non_ignore, reduction=ld.reduction, ohem=ohem)
            loss = loss * ld.loss_weight
            out[ld.loss_name] = out[ld.loss_name] + loss if ld.loss_name in out else loss
            if acc_seg is None:
                acc_seg = acc
        out['acc_seg'] = acc_seg
        return out

    def forward_train(self, neck_feats, backbone_feats, img_metas, gt_semantic_seg, shared_encoder, record=None):
        seg_logits = self.forward(shared_encoder, neck_feats, backbone_feats, img_metas, record)
        if record is not None:
            record['seg_logit'] = seg_logits
        return self.losses(seg_logits, gt_semantic_seg)

    def forward_test(self, neck_feats, backbone_feats, img_metas, shared_encoder):
        return self.forward(shared_encoder, neck_feats, backbone_feats, img_metas)
