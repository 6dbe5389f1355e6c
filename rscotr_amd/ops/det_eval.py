"""Detection evaluation on the device: the inference tail of DINOHead._get_bboxes_single (sigmoid, top-k over (query, class),
box decoding) for a batch in one launch, and COCOeval's per-image matching for every (image, class, area range, IoU
threshold) of a batch in one launch (csrc/det_eval.hip).  Neither op synchronises with the host."""
import torch

from .core import _chk, _f32c, _stream, lib

DET_DECODE_MAX_KEYS = 36864  # Q * C (the keys of one image live in LDS)
DET_DECODE_MAX_K = 1024
DET_MATCH_MAX_GT = 1024      # ground truths of one (image, class); the caller checks it on the host, where it knows the counts
DET_MATCH_MAX_K = 1024
DET_MATCH_MAX_T = 16
DET_MATCH_MAX_FLAG_WORDS = 8192  # min(max_det, K) * A


def det_decode_fits(Q, C, K):
    """Whether rscotr_det_decode_f32 takes the shape (outside it the caller keeps the torch chain)."""
    return Q > 0 and C > 0 and 0 < K <= min(Q * C, DET_DECODE_MAX_K) and Q * C <= DET_DECODE_MAX_KEYS


def det_decode(cls, box, meta, K, rescale):
    """cls (B, Q, C) last-layer logits, box (B, Q, 4) normalised cxcywh, meta (B, 6) fp32 device table of img_h, img_w and
    the four scale-factor entries -> dets (B, K, 5) fp32 [x1, y1, x2, y2, score], labels (B, K) int64, rows in
    torch.topk(sorted=True) order, ties to the lower flat (query, class) index.  RuntimeError outside Q * C <= 36864,
    K <= min(Q * C, 1024).  See include/rscotr.h, rscotr_det_decode_f32."""
    cls, box, meta = _f32c(cls.detach()), _f32c(box.detach()), _f32c(meta)
    _chk(cls, box, meta)
    if cls.dim() != 3 or box.shape != cls.shape[:2] + (4,) or meta.shape != (cls.shape[0], 6):
        raise ValueError(f'det_decode takes (B, Q, C), (B, Q, 4) and (B, 6), got {tuple(cls.shape)}, {tuple(box.shape)}, '
                         f'{tuple(meta.shape)}')
    B, Q, C = cls.shape
    K = int(K)
    dets = torch.empty((B, max(K, 0), 5), dtype=torch.float32, device=cls.device)
    labels = torch.empty((B, max(K, 0)), dtype=torch.int64, device=cls.device)
    lib.call('rscotr_det_decode_f32', cls.data_ptr(), box.data_ptr(), meta.data_ptr(), dets.data_ptr(), labels.data_ptr(),
             B, Q, C, K, int(bool(rescale)), _stream())
    return dets, labels


def det_match(dets, labels, n_det, gt_boxes, gt_labels, gt_offsets, area_ranges, iou_thrs, num_classes, max_det):
    """COCOeval.evaluateImg for a batch (rscotr_amd.metrics._evaluate_img, to the comparison).  dets (B, K, 5) fp32 and labels
    (B, K) int64 in descending score order per image, n_det (B) int32; ground truths of the batch concatenated: gt_boxes
    (G, 4) fp32 xyxy, gt_labels (G) int64, gt_offsets (B + 1) int64; area_ranges (A, 2) and iou_thrs (T) fp64 — all device
    tensors.  -> flags (B, K, A) int32 (bit t: matched at threshold t; bit 16 + t: ignored at t; 0x80000000: dropped) and
    npig (B, C, A) int32.  At most DET_MATCH_MAX_GT ground truths per (image, class): the caller checks that on the host.
    See include/rscotr.h, rscotr_det_match."""
    dev = dets.device
    want = ((dets, torch.float32), (labels, torch.int64), (n_det, torch.int32), (gt_boxes, torch.float32),
            (gt_labels, torch.int64), (gt_offsets, torch.int64), (area_ranges, torch.float64), (iou_thrs, torch.float64))
    if any(t.dtype != d for t, d in want):
        raise TypeError('det_match takes fp32 boxes, int64 labels / offsets, int32 n_det and fp64 ranges / thresholds')
    if dets.dim() != 3 or dets.shape[2] != 5 or labels.shape != dets.shape[:2] or n_det.shape != dets.shape[:1]:
        raise ValueError('det_match takes dets (B, K, 5), labels (B, K), n_det (B)')
    B, K, _ = dets.shape
    G = gt_boxes.shape[0]
    if gt_boxes.shape != (G, 4) or gt_labels.shape != (G,) or gt_offsets.shape != (B + 1,) or area_ranges.dim() != 2 or \
            area_ranges.shape[1] != 2 or iou_thrs.dim() != 1:
        raise ValueError('det_match takes gt_boxes (G, 4), gt_labels (G), gt_offsets (B + 1), area_ranges (A, 2), iou_thrs (T)')
    ts = [t.contiguous() for t, _ in want]
    _chk(*ts)
    A, T, C = area_ranges.shape[0], iou_thrs.shape[0], int(num_classes)
    flags = torch.empty((B, K, A), dtype=torch.int32, device=dev)
    npig = torch.empty((B, max(C, 0), A), dtype=torch.int32, device=dev)
    lib.call('rscotr_det_match', *(t.data_ptr() if t.numel() else 0 for t in ts), flags.data_ptr(), npig.data_ptr(), B, K, G,
             C, A, T, int(max_det), _stream())
    return flags, npig
