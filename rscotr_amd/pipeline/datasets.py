"""Thin readers for the three datasets' on-disk layouts (decode with Pillow; BGR like mmcv.imread's default backend) with their
`evaluate` / `pre_eval`, and a minimal batch loader over them."""
import json
import os
import random

import numpy as np
import torch

from .. import ops


def _imread_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))[..., ::-1].copy()


class FolderClsDataset:
    """mmcls CustomDataset without an annotation file: `data_prefix/<class name>/<image>`; classes = sorted folder
    names (data/NWPU-RESISC45/train, configs/_base_/cls/resisc_swin_224.py:55-58)."""
    task = 'cls'
    EXT = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif')

    def __init__(self, data_prefix):
        self.CLASSES = sorted(d for d in os.listdir(data_prefix) if os.path.isdir(os.path.join(data_prefix, d)))
        self.items = [(os.path.join(data_prefix, c, f), i) for i, c in enumerate(self.CLASSES)
                      for f in sorted(os.listdir(os.path.join(data_prefix, c))) if f.lower().endswith(self.EXT)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        path, label = self.items[i]
        return dict(img=_imread_bgr(path), gt_label=label, filename=path)

    def evaluate(self, results, metric='accuracy', metric_options=None, indices=None, logger=None, **kwargs):
        """mmcls BaseDataset.evaluate: `results` = per-sample score vectors in dataset order -> {'accuracy_top-1', 'accuracy_top-5'}
        in percent (metric_options: topk, thrs)."""
        from ..metrics import accuracy
        metrics = [metric] if isinstance(metric, str) else list(metric)
        if set(metrics) - {'accuracy'}:
            raise ValueError(f'metric {set(metrics) - {"accuracy"}} is not supported (accuracy only)')
        opt = dict(topk=(1, 5)) if metric_options is None else dict(metric_options)
        labels = [self.items[i][1] for i in (range(len(self.items)) if indices is None else indices)]
        assert len(results) == len(labels), 'dataset testing results should be of the same length as gt_labels'
        topk = opt.get('topk', (1, 5))
        return accuracy(results, labels, topk=(topk,) if isinstance(topk, int) else tuple(topk), thrs=opt.get('thrs'))


class CocoDetDataset:
    """mmdet CocoDataset on DIOR's converted annotations (configs/_base_/det/dior.py:41-47): images without boxes and
    crowd / degenerate boxes are dropped as mmdet's `_filter_imgs` / `_parse_ann_info` do; labels index `classes`."""
    task = 'det'

    def __init__(self, ann_file, img_prefix, classes):
        with open(ann_file) as fh:
            coco = json.load(fh)
        self.CLASSES = tuple(classes)
        cat = {c['id']: self.CLASSES.index(c['name']) for c in coco['categories'] if c['name'] in self.CLASSES}
        anns = {}
        for a in coco['annotations']:
            anns.setdefault(a['image_id'], []).append(a)
        self.items = []
        for im in coco['images']:
            boxes, labels = [], []
            for a in anns.get(im['id'], []):
                x, y, w, h = a['bbox']
                if a.get('ignore', False) or a.get('iscrowd', False) or a['category_id'] not in cat:
                    continue
                if w < 1 or h < 1 or a.get('area', w * h) <= 0:
                    continue
                if max(0, min(x + w, im['width']) - max(x, 0)) * max(0, min(y + h, im['height']) - max(y, 0)) == 0:
                    continue
                boxes.append([x, y, x + w, y + h])
                labels.append(cat[a['category_id']])
            if boxes and min(im['width'], im['height']) >= 32:
                self.items.append((os.path.join(img_prefix, im['file_name']), np.asarray(boxes, np.float32),
                                   np.asarray(labels, np.int64)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        path, boxes, labels = self.items[i]
        return dict(img=_imread_bgr(path), gt_bboxes=boxes, gt_labels=labels, filename=path)

    def device_eval_ok(self):
        """Whether `ops.det_match` takes this dataset: no (image, class) holds more ground truths than its cap (counted once,
        on the host)."""
        ok = getattr(self, '_device_eval_ok', None)
        if ok is None:
            most = max((int(np.bincount(it[2]).max()) for it in self.items if len(it[2])), default=0)
            ok = self._device_eval_ok = most <= ops.DET_MATCH_MAX_GT
        return ok

    def pre_eval(self, dets, labels, indices, iou_thrs=None, max_det=100, device=None):
        """COCOeval.evaluateImg for one batch on the device.  dets: per image (K, 5) device tensors [x1, y1, x2, y2, score] in
        original-image coordinates and descending score order (or one (B, K, 5) tensor), labels: (K,) int64 each, `indices`:
        their positions in the dataset.  The ground truths of those images are uploaded and `ops.det_match` runs with COCO's
        area ranges, `iou_thrs` (default: COCO's ten) and `max_det`.  -> per image a tuple (dets, labels, flags (K, A) int32,
        npig (C, A) int32) of device tensors, the kind `evaluate` accumulates with `metrics.coco_accumulate`; nothing comes
        back to the host.  A dataset with more than `ops.DET_MATCH_MAX_GT` ground truths of one class in one image takes the
        host route instead: -> per image the per-class list of (k, 5) arrays of `mtl.bbox2result`."""
        from ..metrics import coco_area_ranges, coco_iou_thrs
        indices = [int(i) for i in indices]
        assert len(dets) == len(labels) == len(indices), 'one index per image'
        C = len(self.CLASSES)
        if not indices:
            return []
        if not self.device_eval_ok():
            from ..mtl import bbox2result
            return [bbox2result(d, l, C) for d, l in zip(dets, labels)]
        dets = dets if torch.is_tensor(dets) else torch.stack(list(dets))
        labels = labels if torch.is_tensor(labels) else torch.stack(list(labels))
        dev = torch.device(device) if device is not None else dets.device
        dets, labels = dets.to(dev, torch.float32), labels.to(dev, torch.int64)
        B, K = labels.shape
        thrs = coco_iou_thrs(iou_thrs)
        self._pre_eval_cfg = (tuple(float(t) for t in thrs), int(max_det))
        gb = [self.items[i][1].reshape(-1, 4) for i in indices]
        gl = [self.items[i][2].reshape(-1) for i in indices]
        off = np.concatenate([[0], np.cumsum([len(g) for g in gl])]).astype(np.int64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        flags, npig = ops.det_match(dets, labels, torch.full((B,), K, dtype=torch.int32, device=dev),
                                    up(np.concatenate(gb).astype(np.float32)), up(np.concatenate(gl).astype(np.int64)), up(off),
                                    up(coco_area_ranges()), up(thrs), C, int(max_det))
        return [tuple(t) for t in zip(dets.unbind(0), labels.unbind(0), flags.unbind(0), npig.unbind(0))]

    def evaluate(self, results, metric='bbox', logger=None, jsonfile_prefix=None, classwise=False, proposal_nums=(100, 300, 1000),
                 iou_thrs=None, metric_items=None, **kwargs):
        """mmdet CocoDataset.evaluate(metric='bbox') -> bbox_mAP / _50 / _75 / _s / _m / _l (COCOeval semantics,
        rscotr_amd/metrics.py).  `results` (dataset order) are either per image a LIST (per class) of (k, 5) arrays in
        original-image coordinates, matched and accumulated on the host (`coco_bbox_map`), or per image a TUPLE (dets, labels,
        flags, npig) of the pre_eval test loop (`engine._test_det(on_device=True)`), matched on the device and only accumulated
        here (`coco_accumulate`): the kind of `results` decides the route, and both give the same dict.  The tuples must have
        been matched with this call's `iou_thrs` and `max_det = proposal_nums[0]`: that is the caller's contract.  The check below only catches the common slip (it
        compares with the last `pre_eval` of THIS object; tuples unpickled from another process are taken on trust)."""
        from ..metrics import coco_accumulate, coco_bbox_map, coco_iou_thrs
        metrics = [metric] if isinstance(metric, str) else list(metric)
        if metrics != ['bbox']:
            raise KeyError(f'metric {metrics} is not supported (bbox only)')
        assert len(results) == len(self.items), 'one result per image'
        if len(results) and isinstance(results[0], tuple) and len(results[0]) == 4:
            cfg = getattr(self, '_pre_eval_cfg', None)
            if cfg is not None and cfg != (tuple(float(t) for t in coco_iou_thrs(iou_thrs)), int(proposal_nums[0])):
                raise ValueError(f'results were pre-evaluated with (iou_thrs, max_det) = {cfg}, evaluate() asks for '
                                 f'{(iou_thrs, proposal_nums[0])}')
            out = coco_accumulate(results, self.CLASSES, iou_thrs=iou_thrs, classwise=classwise)
        else:
            out = coco_bbox_map(results, [it[1] for it in self.items], [it[2] for it in self.items], self.CLASSES,
                                iou_thrs=iou_thrs, max_det=proposal_nums[0], classwise=classwise)
        if metric_items is not None:
            keep = {f'bbox_{m}' for m in metric_items}
            out = type(out)((k, v) for k, v in out.items() if k in keep or k == 'bbox_mAP_copypaste' or k.startswith('bbox_AP.'))
        return out


class TileSegDataset:
    """mmseg CustomDataset / PotsdamDataset: `img_dir/<name>.png` + `ann_dir/<name>.png` single-channel label tiles
    (configs/_base_/seg/potsdam_IRRG_all.py:52-62)."""
    task = 'seg'
    CLASSES = ('impervious_surface', 'building', 'low_vegetation', 'tree', 'car', 'clutter')

    def __init__(self, img_dir, ann_dir, img_suffix='.png', seg_map_suffix='.png', reduce_zero_label=True, ignore_index=255):
        names = sorted(f[:-len(img_suffix)] for f in os.listdir(img_dir) if f.endswith(img_suffix))
        self.items = [(os.path.join(img_dir, n + img_suffix), os.path.join(ann_dir, n + seg_map_suffix)) for n in names]
        self.reduce_zero_label, self.ignore_index = reduce_zero_label, ignore_index  # (mmseg PotsdamDataset: True, 255)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        ip, ap = self.items[i]
        with Image.open(ap) as im:
            seg = np.asarray(im).astype(np.uint8)
        return dict(img=_imread_bgr(ip), gt_semantic_seg=seg, filename=ip)

    def _label_map(self, i):
        from PIL import Image
        with Image.open(self.items[i][1]) as im:
            return np.asarray(im).astype(np.uint8)

    def pre_eval(self, preds, indices, device=None):
        """mmseg CustomDataset.pre_eval for one batch: `preds` = the label maps (uint8 device tensors, or NumPy maps) of the
        images `indices` -> int64 (len(preds), 4, C) on the device: area_intersect, area_union, area_pred_label, area_label
        per image (ops.seg_areas).  The raw label tiles are read and uploaded as uint8; nothing comes back to the host.
        These are mmseg's areas: a kept pixel whose prediction is >= C (a head with more channels than the dataset has
        classes) still counts in area_label, whereas the confusion matrix of the label-map route drops that pixel — see
        `evaluate`."""
        indices = [int(i) for i in indices]
        assert len(preds) == len(indices), 'one index per prediction'
        if device is None:
            device = preds[0].device if torch.is_tensor(preds[0]) and preds[0].is_cuda else 'cuda'
        dev = torch.device(device)

        def u8(p):
            if not torch.is_tensor(p):
                p = torch.from_numpy(np.ascontiguousarray(p))
            if p.dtype != torch.uint8:  # (host maps are int64: a label that does not fit a byte must not wrap into a class)
                if p.numel() and (int(p.min()) < 0 or int(p.max()) > 255):
                    raise ValueError('pre_eval takes label maps with values in 0 .. 255')
                p = p.to(torch.uint8)
            return p.to(dev)
        pred = torch.stack([u8(p) for p in preds])
        gt = torch.from_numpy(np.stack([self._label_map(i) for i in indices])).to(dev)
        return ops.seg_areas(pred, gt, len(self.CLASSES), ignore_index=self.ignore_index,
                             reduce_zero_label=self.reduce_zero_label)

    def evaluate(self, results, metric='mIoU', logger=None, gt_seg_maps=None, device=None, **kwargs):
        """mmseg CustomDataset.evaluate -> aAcc, mIoU / mAcc, mFscore / mPrecision / mRecall, mDice and the per-class values, as
        fractions.  `results` (dataset order) are either per-image label maps at the original size (arrays or tensors: the
        confusion matrix is accumulated on the device, rscotr_amd/metrics.py) or the per-image 4-tuples (area_intersect,
        area_union, area_pred_label, area_label) of the pre_eval test loop (`engine._test_seg(pre_eval=True)`), which are summed
        over the images and need no label map here.  The `pre_eval` / `classwise` keys of the reference's config are accepted:
        the kind of `results` decides the route, and per-class values are always returned.  The two routes agree exactly
        while every prediction is a class of the dataset (< C).  They differ for a pixel predicted >= C: mmseg's areas keep it
        in area_label (it lowers aAcc, Acc and Recall, as in the reference's pre_eval mode), the confusion matrix drops it
        from every count."""
        from ..metrics import confusion_matrix, seg_metrics, seg_metrics_from_areas
        assert len(results) == len(self.items), 'one result per image'
        if len(results) and isinstance(results[0], (tuple, list)) and len(results[0]) == 4:
            total = sum(torch.stack([torch.as_tensor(a).reshape(-1).cpu().long() for a in r]) for r in results)
            return seg_metrics_from_areas(total[0], total[2], total[3], self.CLASSES, metrics=metric)

        def gts():
            if gt_seg_maps is not None:
                yield from gt_seg_maps
                return
            for i in range(len(self.items)):
                yield self._label_map(i)
        results = [r.cpu().numpy() if torch.is_tensor(r) else r for r in results]
        cm = confusion_matrix(results, gts(), len(self.CLASSES), ignore_index=self.ignore_index,
                              reduce_zero_label=self.reduce_zero_label, device=device)
        return seg_metrics(cm, self.CLASSES, metrics=metric)


class DeviceLoader:
    """Minimal batch loader over one of the datasets above: shuffled index batches, decoded on the host, everything
    else in `DeviceCollate`.  `len()` = batches per epoch; `.dataset.task` is what MultiDataLoader tags batches with."""

    def __init__(self, dataset, collate, batch_size, shuffle=True, drop_last=True, seed=0, test_mode=False):
        self.dataset, self.collate, self.batch_size = dataset, collate, batch_size
        self.shuffle, self.drop_last, self.rng = shuffle, drop_last, np.random.RandomState(seed)
        self.py_rng = random.Random(seed)  # RandAugment's second generator (mmcls draws its policies from `random`)
        # test_mode: dataset order, every sample, batches of {task, img, img_metas} only — what `engine.single_gpu_test` feeds
        # `model(return_loss=False, **data)` (the collate should be built with flip_prob = 0 and no crop)
        self.test_mode = test_mode
        if test_mode:
            self.shuffle, self.drop_last = False, False

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = self.rng.permutation(len(self.dataset)) if self.shuffle else np.arange(len(self.dataset))
        for b in range(len(self)):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            if getattr(self.collate, 'rand_augment', None) is not None:
                batch = self.collate([self.dataset[int(i)] for i in idx], self.rng, self.py_rng)
            else:
                batch = self.collate([self.dataset[int(i)] for i in idx], self.rng)
            yield dict(task=self.dataset.task, img=batch['img'], img_metas=batch['img_metas']) if self.test_mode else batch
