"""Host side of the on-device detection evaluation (no GPU): `metrics.coco_accumulate` over pre-matched detections gives
exactly `coco_bbox_map`'s dict, and `CocoDetDataset.evaluate` takes that route for per-image tuples.  Also home of what
test_det_eval_gpu.py shares with these tests: the detection-matching cases and the packing of the host's `_evaluate_img` into
the flag layout of `ops.det_match` (include/rscotr.h, rscotr_det_match)."""
import json

import numpy as np
import pytest
import torch

from rscotr_amd.metrics import _AREA, _evaluate_img, coco_accumulate, coco_bbox_map, coco_iou_thrs

CLASSES = ('c0', 'c1', 'c2', 'c3')
K = 40
DROPPED = np.int32(-(1 << 31))


def _jitter(rng, boxes, amount):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    return (b + rng.uniform(-amount, amount, size=b.shape)).astype(np.float32)


def match_cases():
    """-> dets (3, K, 5) fp32 in descending score order per image, labels (3, K) int64, n_det (3,), gt_boxes / gt_labels per
    image.  Together: an IoU of exactly 0.5; two ground truths of equal IoU to one detection; ground truths on both sides
    of (and on) 32^2 and 96^2; an unmatched detection outside an area range; a class with detections and no ground truth,
    one with ground truth and no detection, one with neither; six detections of one class (more than max_det = 3); 130
    ground truths of one (image, class); n_det < K."""
    rng = np.random.RandomState(11)
    img = []
    # ---- image 0
    gt0 = [([0, 0, 1, 1], 0), ([10, 10, 30, 20], 0), ([10, 20, 30, 30], 0),  # exact 0.5; the equal pair
           ([100, 100, 120, 120], 1), ([200, 100, 240, 140], 1), ([300, 100, 400, 200], 1), ([100, 300, 132, 332], 1),
           ([200, 300, 296, 396], 1), ([400, 300, 431, 331], 1), ([50, 400, 147, 497], 1),  # 400, 1600, 1e4, 32^2, 96^2, 31^2, 97^2
           ([500, 500, 540, 560], 3)]                                                   # class 3: ground truth, no detection
    d0 = [([0, 0, 2, 1], 0), ([10, 10, 30, 30], 0), ([10, 11, 30, 21], 0), ([600, 600, 604, 604], 0),  # the last: unmatched, small
          ([600, 10, 800, 300], 0)]                                                                    # unmatched, large
    d0 += [(b, 1) for b in _jitter(rng, [g for g, l in gt0 if l == 1], 3.0)]
    d0 += [(b, 1) for b in _jitter(rng, [g for g, l in gt0 if l == 1][:4], 9.0)]
    d0 += [([700, 700, 750, 790], 2), ([20, 700, 45, 720], 2), ([300, 700, 500, 900], 2)]  # class 2: detections, no ground truth
    img.append((gt0, d0, None))
    # ---- image 1: six detections of class 0; 130 ground truths of class 1 on a grid; class 3 has neither
    gt1 = [([40, 40, 90, 100], 0), ([45, 48, 95, 105], 0)]
    grid = [[20 * (i % 13), 200 + 20 * (i // 13), 20 * (i % 13) + 14 + (i % 5) * 8, 200 + 20 * (i // 13) + 12 + (i % 7) * 6]
            for i in range(130)]
    gt1 += [(g, 1) for g in grid]
    gt1 += [([600, 20, 700, 90], 2)]
    d1 = [(b, 0) for b in _jitter(rng, [[40, 40, 90, 100]] * 3 + [[45, 48, 95, 105]] * 3, 6.0)]
    d1 += [(b, 1) for b in _jitter(rng, [grid[i] for i in (0, 5, 64, 65, 70, 100, 129, 129, 12)], 2.5)]
    d1 += [(grid[77], 1), (grid[77], 1)]  # IoU exactly 1 twice: the second finds its ground truth taken
    d1 += [(b, 2) for b in _jitter(rng, [[600, 20, 700, 90]] * 2, 15.0)]
    img.append((gt1, d1, None))
    # ---- image 2: n_det < K, random boxes of classes 0 .. 2
    gb = rng.uniform(0, 300, size=(14, 2))
    gwh = rng.uniform(8, 130, size=(14, 2))
    gt2 = [(np.concatenate([p, p + s]).astype(np.float32), int(l)) for p, s, l in zip(gb, gwh, rng.randint(0, 3, size=14))]
    d2 = [(_jitter(rng, gt2[i][0], 0.12 * float(gwh[i].min()))[0], gt2[i][1] if rng.rand() < 0.8 else int(rng.randint(0, 3)))
          for i in rng.randint(0, 14, size=17)]
    img.append((gt2, d2, 17))

    dets = np.zeros((len(img), K, 5), np.float32)
    labels = np.zeros((len(img), K), np.int64)
    n_det = np.zeros(len(img), np.int32)
    gt_boxes, gt_labels = [], []
    for i, (gt, d, n) in enumerate(img):
        order = rng.permutation(len(d))  # classes interleaved along the score order
        assert len(d) <= K
        n_det[i] = len(d)
        for r, j in enumerate(order):
            dets[i, r, :4] = np.asarray(d[j][0], np.float32)
            dets[i, r, 4] = np.float32(0.97 - 0.02 * r)
            labels[i, r] = d[j][1]
        # rows at and beyond n_det do not exist: plausible-looking content that must not be read
        dets[i, len(d):] = dets[i, :1]
        labels[i, len(d):] = 1
        gt_boxes.append(np.asarray([g for g, _ in gt], np.float32).reshape(-1, 4))
        gt_labels.append(np.asarray([l for _, l in gt], np.int64))
    assert n_det[2] == 17 and n_det.max() <= K
    return dets, labels, n_det, gt_boxes, gt_labels


def host_results(dets, labels, n_det):
    """The list route's input: per image the per-class (k, 5) arrays (mtl.bbox2result of the existing rows)."""
    return [[dets[i, :n_det[i]][labels[i, :n_det[i]] == c] for c in range(len(CLASSES))] for i in range(len(dets))]


def host_flags(dets, labels, n_det, gt_boxes, gt_labels, iou_thrs, max_det):
    """flags (B, K, A) int32 and npig (B, C, A) int32 from `_evaluate_img` over every (image, class, area range)."""
    thrs = coco_iou_thrs(iou_thrs)
    B, A, C = len(dets), len(_AREA), len(CLASSES)
    flags = np.full((B, dets.shape[1], A), DROPPED, np.int32)
    npig = np.zeros((B, C, A), np.int32)
    for i in range(B):
        for c in range(C):
            rows = np.nonzero(labels[i, :n_det[i]] == c)[0]
            dt = dets[i, rows].astype(np.float64).reshape(-1, 5)
            gt = gt_boxes[i].astype(np.float64).reshape(-1, 4)[gt_labels[i] == c]
            for a, rng in enumerate(_AREA.values()):
                s, m, ig, n = _evaluate_img(dt, gt, rng, thrs, max_det)
                assert np.array_equal(s, dt[:max_det, 4])  # (already in score order: the first max_det rows are kept)
                npig[i, c, a] = n
                word = np.zeros(m.shape[1], np.int64)
                for t in range(len(thrs)):
                    word |= (m[t].astype(np.int64) << t) | (ig[t].astype(np.int64) << (16 + t))
                flags[i, rows[:max_det], a] = word.astype(np.uint32).view(np.int32) if len(word) else word.astype(np.int32)
    return flags, npig


def _same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        x, y = a[k], b[k]
        assert x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (k, x, y)


@pytest.fixture(scope='module')
def cases():
    return match_cases()


def _tuples(cases, iou_thrs, max_det, as_tensor=False):
    dets, labels, n_det, gb, gl = cases
    flags, npig = host_flags(dets, labels, n_det, gb, gl, iou_thrs, max_det)
    wrap = torch.from_numpy if as_tensor else (lambda x: x)
    return [tuple(wrap(np.ascontiguousarray(x[i])) for x in (dets, labels, flags, npig)) for i in range(len(dets))]


@pytest.mark.parametrize('classwise', [False, True])
@pytest.mark.parametrize('iou_thrs', [None, [0.5]])
@pytest.mark.parametrize('max_det', [100, 3])
def test_accumulate_of_host_flags_is_coco_bbox_map(cases, classwise, iou_thrs, max_det):
    dets, labels, n_det, gb, gl = cases
    want = coco_bbox_map(host_results(dets, labels, n_det), gb, gl, CLASSES, iou_thrs=iou_thrs, max_det=max_det,
                         classwise=classwise)
    got = coco_accumulate(_tuples(cases, iou_thrs, max_det), CLASSES, iou_thrs=iou_thrs, classwise=classwise)
    _same(got, want)
    assert want['bbox_mAP'] > 0 and want['bbox_mAP_s'] >= 0 and want['bbox_mAP_l'] >= 0  # (every area range is populated)


def test_cases_hold_what_they_claim(cases):
    """The properties the matching cases are there for (so that a change to them cannot quietly lose one)."""
    from rscotr_amd.metrics import _iou_xyxy
    dets, labels, n_det, gb, gl = cases
    assert _iou_xyxy(np.array([[0., 0, 2, 1]]), np.array([[0., 0, 1, 1]]))[0, 0] == 0.5
    two = _iou_xyxy(np.array([[10., 10, 30, 30]]), gb[0][1:3].astype(np.float64))[0]
    assert two[0] == two[1] == 0.5
    flags, npig = host_flags(dets, labels, n_det, gb, gl, None, 3)
    k = int(np.nonzero((dets[0, :, :4] == np.float32([10, 10, 30, 30])).all(1))[0][0])
    assert flags[0, k, 0] & 1  # matched at 0.5 ... (which of the two: the GPU test compares the later detection's outcome)
    assert (np.bincount(labels[1, :n_det[1]], minlength=4)[0] == 6) and (flags[1, :n_det[1]][labels[1, :n_det[1]] == 0, 0] ==
                                                                        np.int32(-(1 << 31))).sum() == 3
    assert (gl[1] == 1).sum() == 130 and n_det[2] < K
    areas = (gb[0][:, 2] - gb[0][:, 0]) * (gb[0][:, 3] - gb[0][:, 1])
    assert {1024.0, 9216.0, 961.0, 9409.0} <= set(areas.tolist())
    assert not (gl[0] == 2).any() and (labels[0, :n_det[0]] == 2).any()      # detections, no ground truth
    assert (gl[0] == 3).any() and not (labels[0, :n_det[0]] == 3).any()      # ground truth, no detection
    assert not (gl[1] == 3).any() and not (labels[1, :n_det[1]] == 3).any()  # neither
    assert npig[0, 1].tolist() == [7, 3, 3, 3] and npig[1, 3].tolist() == [0, 0, 0, 0]
    # an unmatched detection outside an area range is ignored there and counted elsewhere
    k = int(np.nonzero((dets[0, :, :4] == np.float32([600, 600, 604, 604])).all(1))[0][0])
    assert flags[0, k].tolist() == [0, 0, 0x3ff << 16, 0x3ff << 16]


def _dataset(tmp_path, cases):
    from rscotr_amd.pipeline import CocoDetDataset
    dets, labels, n_det, gb, gl = cases
    images = [dict(id=i, file_name=f'{i}.png', width=1000, height=1000) for i in range(len(gb))]
    anns = []
    for i, (b, l) in enumerate(zip(gb, gl)):
        for (x1, y1, x2, y2), c in zip(b.tolist(), l.tolist()):
            anns.append(dict(id=len(anns), image_id=i, category_id=c + 1, bbox=[x1, y1, x2 - x1, y2 - y1], iscrowd=0))
    (tmp_path / 'det.json').write_text(json.dumps(dict(images=images, annotations=anns,
                                                       categories=[dict(id=k + 1, name=n) for k, n in enumerate(CLASSES)])))
    return CocoDetDataset(str(tmp_path / 'det.json'), str(tmp_path), classes=CLASSES)


def test_evaluate_takes_the_route_of_the_results_kind(cases, tmp_path, monkeypatch):
    from rscotr_amd import metrics
    dets, labels, n_det, gb, gl = cases
    ds = _dataset(tmp_path, cases)
    assert all(np.array_equal(it[1], b) and np.array_equal(it[2], l) for it, b, l in zip(ds.items, gb, gl))
    kw = dict(iou_thrs=[0.5], classwise=True, proposal_nums=(3, 300, 1000), metric_items=['mAP', 'mAP_50'])
    want = ds.evaluate(host_results(dets, labels, n_det), **kw)
    assert 'bbox_mAP_75' not in want and 'bbox_AP.c1' in want
    calls = []
    real = metrics.coco_accumulate
    monkeypatch.setattr(metrics, 'coco_accumulate', lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(metrics, 'coco_bbox_map', lambda *a, **k: pytest.fail('tuples must not take the host matching route'))
    _same(ds.evaluate(_tuples(cases, [0.5], 3, as_tensor=True), **kw), want)
    _same(ds.evaluate(_tuples(cases, [0.5], 3), **kw), want)
    assert len(calls) == 2
    with pytest.raises(AssertionError):
        ds.evaluate(_tuples(cases, [0.5], 3)[:2], **kw)
