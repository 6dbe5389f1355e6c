"""Segmentation evaluation on the device: the inference tail of MTL.simple_test_seg (resample, flip, arg-max), that of
MTL.aug_test_seg (the same over V views: softmax, mean, arg-max), that of test mode 'slide' (the windows' logits merged,
rescaled, arg-maxed) and mmseg's pre_eval areas (intersect_and_union), one launch each (csrc/seg_eval.hip).  No op synchronises with the host."""
import numpy as np
import torch

from .core import _chk, _f32c, _stream, lib

_FLIP = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}


def seg_predict(logit, canvas_hw, crop_hw=None, out_hw=None, flip=None):
    """logit (B, C, h, w) -> uint8 label maps (B, Ho, Wo): arg-max over the channels of the logits resampled to the canvas
    (bilinear, align_corners=False) and, when `out_hw` is given (rescale), cropped to `crop_hw` (default: the canvas) and
    resampled to `out_hw`; without it the maps have the canvas size.  flip: None | 'horizontal' | 'vertical', applied to
    the finished map.  See include/rscotr.h, rscotr_seg_predict_u8."""
    if flip not in _FLIP:
        raise ValueError(f"flip must be None, 'horizontal' or 'vertical', got {flip!r}")
    logit = _f32c(logit.detach())
    _chk(logit)
    B, C, h, w = logit.shape
    H, W = (int(v) for v in canvas_hw)
    rescale = out_hw is not None
    if crop_hw is not None and not rescale:
        raise ValueError('crop_hw needs out_hw (the crop belongs to the rescale stage)')
    hs, ws = (H, W) if crop_hw is None else (int(v) for v in crop_hw)
    Ho, Wo = (int(v) for v in out_hw) if rescale else (H, W)
    out = torch.empty((B, max(Ho, 0), max(Wo, 0)), dtype=torch.uint8, device=logit.device)
    lib.call('rscotr_seg_predict_u8', logit.data_ptr(), out.data_ptr(), B, C, h, w, H, W, int(rescale), hs, ws, Ho, Wo,
             _FLIP[flip], _stream())
    return out


def _pair(v, what):
    v = tuple(int(a) for a in v) if isinstance(v, (tuple, list)) else (int(v), int(v))
    if len(v) != 2:
        raise ValueError(f'{what} is (y, x) or one integer, got {v!r}')
    return v


def slide_windows(H, W, crop_size, stride):
    """The window grid of mmseg's EncoderDecoder.slide_inference on an (H, W) canvas -> [(y1, y2, x1, x2)] in visiting order
    (row-major, y outer).  Per axis max(n - crop + stride - 1, 0) // stride + 1 windows, window i ending at
    min(i * stride + crop, n) and starting max(end - crop, 0): the last one is shifted back inside the image, and an axis
    shorter than the crop has one window, the whole axis.  ValueError: a non-positive size, or a stride larger than the crop
    on an axis where the image exceeds the crop (pixels between two windows would be covered by none)."""
    H, W = int(H), int(W)
    (ch, cw), (sy, sx) = _pair(crop_size, 'crop_size'), _pair(stride, 'stride')
    if min(H, W, ch, cw, sy, sx) <= 0:
        raise ValueError(f'slide_windows: non-positive size (canvas {H} x {W}, crop_size {(ch, cw)}, stride {(sy, sx)})')
    for n, crop, s, axis in ((H, ch, sy, 'y'), (W, cw, sx, 'x')):
        if n > crop and s > crop:
            raise ValueError(f'slide_windows: stride {s} larger than the crop {crop} on the {axis} axis ({n} pixels): '
                             'pixels between two windows would be covered by none')

    def axis(n, crop, s):
        spans = []
        for i in range(max(n - crop + s - 1, 0) // s + 1):
            b = min(i * s + crop, n)
            spans.append((max(b - crop, 0), b))
        return spans
    return [(y1, y2, x1, x2) for y1, y2 in axis(H, ch, sy) for x1, x2 in axis(W, cw, sx)]


def seg_predict_slide(logits, batch, canvas_hw, crop_size, stride, crop_hw=None, out_hw=None, flip=None):
    """The tail of test mode 'slide' as ONE launch.  logits (len(windows) * batch, C, h, w): the head's logits of every window
    of slide_windows(*canvas_hw, crop_size, stride) in visiting order, the batch innermost.  -> uint8 label maps (batch, Ho, Wo):
    arg-max over the channels of the canvas map (per pixel the in-order sum over the covering windows of the window's logits
    resampled to the window size, bilinear, align_corners=False, divided by their number) and, when `out_hw` is given
    (rescale), cropped to `crop_hw` (default: the canvas) and resampled to `out_hw`; without it the maps have the canvas
    size.  flip: None | 'horizontal' | 'vertical', applied to the finished map.  See include/rscotr.h,
    rscotr_seg_predict_slide_u8."""
    if flip not in _FLIP:
        raise ValueError(f"flip must be None, 'horizontal' or 'vertical', got {flip!r}")
    H, W = (int(v) for v in canvas_hw)
    (ch, cw), (sy, sx) = _pair(crop_size, 'crop_size'), _pair(stride, 'stride')
    windows = slide_windows(H, W, (ch, cw), (sy, sx))
    B = int(batch)
    if B <= 0:
        raise ValueError(f'seg_predict_slide: non-positive batch {B}')
    if logits.dim() != 4 or logits.shape[0] != len(windows) * B:
        raise ValueError(f'seg_predict_slide: logits {tuple(logits.shape)} are not (windows * batch, C, h, w) with '
                         f'{len(windows)} windows x batch {B}')
    rescale = out_hw is not None
    if crop_hw is not None and not rescale:
        raise ValueError('crop_hw needs out_hw (the crop belongs to the rescale stage)')
    logits = _f32c(logits.detach())
    _chk(logits)
    _, C, h, w = logits.shape
    hs, ws = (H, W) if crop_hw is None else (int(v) for v in crop_hw)
    Ho, Wo = (int(v) for v in out_hw) if rescale else (H, W)
    out = torch.empty((B, max(Ho, 0), max(Wo, 0)), dtype=torch.uint8, device=logits.device)
    lib.call('rscotr_seg_predict_slide_u8', logits.data_ptr(), out.data_ptr(), B, C, h, w, H, W, ch, cw, sy, sx, int(rescale),
             hs, ws, Ho, Wo, _FLIP[flip], _stream())
    return out


def seg_predict_tta(logits, canvases, crops, out_hw, flips):
    """Multi-scale / flip test-time augmentation (mmseg aug_test, mode 'whole') as ONE launch.  logits: V tensors
    (B, C, h_v, w_v) with the same B and C on one device; canvases[v]: the padded input size (H, W) of view v; crops[v]: its
    img_shape (hs, ws), or None for the canvas; flips[v]: None | 'horizontal' | 'vertical'; out_hw: the common ori_shape
    (Ho, Wo).  -> uint8 label maps (B, Ho, Wo): arg-max over the channels of the mean over the views of softmax(view resampled
    to the canvas, cropped, resampled to out_hw, un-flipped).  See include/rscotr.h, rscotr_seg_predict_tta_u8."""
    V = len(logits)
    if not (len(canvases) == len(crops) == len(flips) == V):
        raise ValueError(f'one canvas, crop and flip per view: {V} logits, {len(canvases)} canvases, {len(crops)} crops, '
                         f'{len(flips)} flips')
    for f in flips:
        if f not in _FLIP:
            raise ValueError(f"flip must be None, 'horizontal' or 'vertical', got {f!r}")
    for t in logits:
        if t.dim() != 4 or t.shape[:2] != logits[0].shape[:2] or t.device != logits[0].device:
            raise ValueError(f'every view is (B, C, h, w) with the same B and C on one device: {[tuple(t.shape) for t in logits]}')
    if V == 0:
        raise ValueError('seg_predict_tta takes at least one view')
    Ho, Wo = (int(v) for v in out_hw)
    held = [_f32c(t.detach()) for t in logits]  # (alive until the launch is enqueued)
    _chk(*held)
    B, C = held[0].shape[:2]
    rows = np.zeros((V, 8), dtype=np.int64)
    for v, (t, canvas, crop, flip) in enumerate(zip(held, canvases, crops, flips)):
        H, W = (int(a) for a in canvas)
        hs, ws = (H, W) if crop is None else (int(a) for a in crop)
        rows[v] = [t.data_ptr(), t.shape[2], t.shape[3], H, W, hs, ws, _FLIP[flip]]
    out = torch.empty((B, max(Ho, 0), max(Wo, 0)), dtype=torch.uint8, device=held[0].device)
    lib.call('rscotr_seg_predict_tta_u8', rows.ctypes.data, out.data_ptr(), V, B, C, Ho, Wo, _stream())
    return out


def seg_areas(pred, gt, num_classes, ignore_index=255, reduce_zero_label=False):
    """pred, gt uint8 (B, Hp, Wp) (gt: raw label maps) -> int64 (B, 4, C): area_intersect, area_union, area_pred_label,
    area_label per image and class (mmseg intersect_and_union).  See include/rscotr.h, rscotr_seg_areas_u8."""
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise TypeError('seg_areas takes uint8 prediction and label maps')
    if pred.dim() != 3 or pred.shape != gt.shape:
        raise ValueError(f'prediction {tuple(pred.shape)} and label maps {tuple(gt.shape)} must both be (B, Hp, Wp)')
    pred, gt = pred.contiguous(), gt.contiguous()
    _chk(pred, gt)
    B, Hp, Wp = pred.shape
    out = torch.zeros((B, 4, max(int(num_classes), 0)), dtype=torch.int64, device=pred.device)
    lib.call('rscotr_seg_areas_u8', pred.data_ptr(), gt.data_ptr(), out.data_ptr(), B, Hp, Wp, int(num_classes),
             int(ignore_index), int(bool(reduce_zero_label)), _stream())
    return out
