"""Host side of the pre_eval segmentation mode (no GPU): metrics from class areas, TileSegDataset.evaluate on the 4-tuples of
the pre_eval test loop, the loop's index bookkeeping and the evaluation hook's `test_kwargs`."""
import numpy as np
import pytest
import torch

from rscotr_amd.engine import MultiDatasetsEvalHook, single_gpu_test
from rscotr_amd.metrics import seg_metrics, seg_metrics_from_areas


def _same(a, b):
    assert list(a) == list(b)
    va, vb = np.array(list(a.values()), dtype=np.float64), np.array(list(b.values()), dtype=np.float64)
    assert np.array_equal(va, vb, equal_nan=True), (a, b)


def test_metrics_from_areas_equal_the_confusion_matrix_route():
    cm = torch.tensor([[50, 3, 0, 2], [4, 30, 1, 0], [0, 0, 0, 0], [7, 0, 5, 11]], dtype=torch.int64)  # class 2 never labelled
    names = ('a', 'b', 'c', 'd')
    for metrics in ('mIoU', ['mFscore', 'mIoU'], ['mDice'], ['mIoU', 'mDice', 'mFscore']):
        for kw in (dict(), dict(nan_to_num=0), dict(beta=2)):
            _same(seg_metrics_from_areas(cm.diag(), cm.sum(0), cm.sum(1), names, metrics=metrics, **kw),
                  seg_metrics(cm, names, metrics=metrics, **kw))
    # NumPy vectors and lists are taken too
    _same(seg_metrics_from_areas(cm.diag().numpy(), cm.sum(0).tolist(), cm.sum(1), names), seg_metrics(cm, names))
    with pytest.raises(KeyError):
        seg_metrics_from_areas(cm.diag(), cm.sum(0), cm.sum(1), names, metrics='mAP')


def test_metrics_from_areas_hand_worked_two_classes():
    # 10 kept pixels: 6 labelled x (4 predicted x), 4 labelled y (3 predicted y): pred x = 4 + 1 = 5, pred y = 3 + 2 = 5
    approx = lambda v: pytest.approx(v, abs=1e-9)  # (round(x * 100, 2) / 100 in binary)
    out = seg_metrics_from_areas([4, 3], [5, 5], [6, 4], ('x', 'y'), metrics=['mIoU', 'mFscore'])
    assert out['aAcc'] == approx(0.7)
    assert out['IoU.x'] == approx(0.5714) and out['IoU.y'] == approx(0.5)            # 4 / (6 + 5 - 4), 3 / (4 + 5 - 3)
    assert out['Acc.x'] == approx(0.6667) and out['Acc.y'] == approx(0.75)           # 4 / 6, 3 / 4
    assert out['Precision.x'] == approx(0.8) and out['Precision.y'] == approx(0.6)   # 4 / 5, 3 / 5
    assert out['Recall.x'] == approx(0.6667) and out['Recall.y'] == approx(0.75)
    assert out['Fscore.x'] == approx(0.7273) and out['Fscore.y'] == approx(0.6667)   # 2 * .8 * (2/3) / (.8 + 2/3), 2 * .6 * .75 / 1.35
    assert out['mIoU'] == approx(0.5357) and out['mAcc'] == approx(0.7083)           # means of the unrounded values


def _tile_dataset(root, n=3, size=16, seed=0):
    from PIL import Image
    from rscotr_amd.pipeline import TileSegDataset
    rng = np.random.RandomState(seed)
    (root / 'img').mkdir(); (root / 'ann').mkdir()
    for i in range(n):
        Image.fromarray(rng.randint(0, 255, size=(size, size, 3)).astype(np.uint8)).save(root / 'img' / f't{i}.png')
        Image.fromarray(rng.randint(0, 7, size=(size, size)).astype(np.uint8)).save(root / 'ann' / f't{i}.png')
    return TileSegDataset(str(root / 'img'), str(root / 'ann')), rng


def _areas(pred, raw_label, C):
    """intersect_and_union with reduce_zero_label and ignore_index 255, predictions inside the classes."""
    label = raw_label.astype(np.int64) - 1
    keep = label >= 0
    p, l = pred.astype(np.int64)[keep], label[keep]
    hist = lambda v: torch.from_numpy(np.bincount(v[v < C], minlength=C).astype(np.int64))
    inter, ap, al = hist(p[p == l]), hist(p), hist(l)
    return inter, ap + al - inter, ap, al


def test_tile_dataset_evaluates_area_tuples_without_the_library(tmp_path, monkeypatch):
    from rscotr_amd import _lib
    monkeypatch.setattr(_lib._Lib, 'load', lambda self: (_ for _ in ()).throw(AssertionError('library call on the host route')))
    ds, rng = _tile_dataset(tmp_path)
    C = len(ds.CLASSES)
    preds = [rng.randint(0, C, size=(16, 16)).astype(np.int64) for _ in range(3)]
    tuples = [_areas(p, ds._label_map(i), C) for i, p in enumerate(preds)]
    metric = ['mFscore', 'mIoU']
    got = ds.evaluate(tuples, metric=metric, device='cpu', pre_eval=True, classwise=True)
    # the label-map route (confusion matrix) on the same predictions, and the sums of the tuples fed to the metrics directly
    _same(got, ds.evaluate(preds, metric=metric, device='cpu'))
    _same(got, ds.evaluate([torch.from_numpy(p) for p in preds], metric=metric, device='cpu'))
    total = [sum(t[k] for t in tuples) for k in range(4)]
    assert torch.equal(total[1], total[2] + total[3] - total[0])
    _same(got, seg_metrics_from_areas(total[0], total[2], total[3], ds.CLASSES, metrics=metric))
    with pytest.raises(AssertionError):
        ds.evaluate(tuples[:2], metric=metric, device='cpu')


class _AreaDS:
    task = 'seg'

    def __init__(self, n):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def pre_eval(self, preds, indices):
        self.calls.append(list(indices))
        return torch.stack([torch.full((4, 3), int(p), dtype=torch.int64) for p in preds])


class _Loader(list):
    def __init__(self, dataset, batches):
        super().__init__(batches)
        self.dataset = dataset


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.CLASSES, self.calls = None, []

    def forward(self, task, img, img_metas, return_loss=True, **kw):
        assert not return_loss and not self.training and not torch.is_grad_enabled()
        self.calls.append(dict(kw))
        return [torch.tensor(int(v)) for v in img]


def test_pre_eval_loop_indices_and_result_layout():
    mk = lambda xs: dict(task='seg', img=torch.tensor(xs), img_metas=[{}] * len(xs))
    ds = _AreaDS(3)
    loader = _Loader(ds, [mk([5, 6]), mk([7])])
    model = _Model().train()
    res = single_gpu_test(model, dict(potsdam=loader), kwargs_dict=dict(seg=dict(pre_eval=True, opacity=0.3)))['potsdam']
    assert ds.calls == [[0, 1], [2]] and model.calls == [dict(on_device=True)] * 2 and model.training
    assert len(res) == 3 and all(isinstance(r, tuple) and len(r) == 4 for r in res)
    assert [int(r[0][0]) for r in res] == [5, 6, 7] and all(a.dtype == torch.int64 and tuple(a.shape) == (3,) for a in res[0])
    # a batch sampler names the indices
    loader.batch_sampler = [[2, 0], [1]]
    ds.calls.clear()
    single_gpu_test(model, dict(potsdam=loader), kwargs_dict=dict(seg=dict(pre_eval=True)))
    assert ds.calls == [[2, 0], [1]]
    # pre_eval=False: the plain loop, the model's own results
    model.calls.clear()
    plain = single_gpu_test(model, dict(potsdam=loader), kwargs_dict=dict(seg=dict(pre_eval=False)))['potsdam']
    assert [int(p) for p in plain] == [5, 6, 7] and model.calls == [{}] * 2


class _Runner:
    def __init__(self):
        self.model, self.iter, self.epoch, self.meta = _Model(), 4, 0, {}
        self.log_buffer_output, self.log_buffer_ready, self.logger = {}, False, None


def test_eval_hook_passes_test_kwargs():
    class DS(_AreaDS):
        def evaluate(self, results, logger=None, **kw):
            return {'mIoU': float(len(results))}
    loaders = dict(potsdam=_Loader(DS(2), []))
    seen = []

    def test_fn(*args, **kwargs):
        seen.append((args, kwargs))
        return dict(potsdam=[0, 0])
    r = _Runner()
    MultiDatasetsEvalHook(loaders, interval=4, by_epoch=False, test_fn=test_fn).after_train_iter(r)
    assert seen == [((r.model, loaders), {})]  # the default makes the call it always made
    tk = dict(seg=dict(pre_eval=True))
    MultiDatasetsEvalHook(loaders, interval=4, by_epoch=False, test_fn=test_fn, test_kwargs=tk,
                          seg=dict(metric='mIoU')).after_train_iter(r)
    assert seen[1] == ((r.model, loaders), dict(kwargs_dict=tk))
    assert r.log_buffer_output['potsdam.mIoU'] == 2.0
