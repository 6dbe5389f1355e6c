"""synth.make_batch: the default batches are pinned by digest (bench.py, the synthetic loader and every seeded test draw
them), and the padded / non-square batches follow mmdet's Resize + Pad(size_divisor=32) + Normalize layout."""
import hashlib

import numpy as np
import pytest
import torch

from rscotr_amd import synth


def batch_digest(obj, h=None):
    """sha256 over every tensor / array (dtype, shape, bytes) and every other value (repr) of a nested batch, keys sorted."""
    top = h is None
    h = h or hashlib.sha256()
    if torch.is_tensor(obj):
        t = obj.detach().cpu().contiguous()
        h.update(f'T{t.dtype}{tuple(t.shape)}'.encode())
        h.update(t.numpy().tobytes())
    elif isinstance(obj, np.ndarray):
        a = np.ascontiguousarray(obj)
        h.update(f'A{a.dtype}{a.shape}'.encode())
        h.update(a.tobytes())
    elif isinstance(obj, dict):
        for k in sorted(obj):
            h.update(f'K{k}'.encode())
            batch_digest(obj[k], h)
    elif isinstance(obj, (list, tuple)):
        h.update(f'L{len(obj)}'.encode())
        for v in obj:
            batch_digest(v, h)
    else:
        h.update(f'V{obj!r}'.encode())
    return h.hexdigest() if top else None


# recorded with the square-only generator, before canvases and per-image shapes were added
DEFAULT_DIGESTS = {
    ('cls', 2, 64, 3): '5a77cb7d19af69d27e7ef2232294cd62eca2fd30a390a8b8aa60459b68a384c9',
    ('cls', 2, 512, 17): 'b51c9a915cf16921f6cd851b02d4d8bb712d82435b64a677bc1ae2b38b865e95',
    ('det', 2, 64, 3): '97c3ccd832bbf07b76df0b7b8bb3eb502984e772ff89df14960a0131d130f192',
    ('det', 2, 512, 17): 'b419b6151796be5c0e96b65cf9d65da31f5aa601079c18defe3d2f64eda6d031',
    ('seg', 2, 64, 3): 'fa03ca1516605cc35c1948127d646c306b9e26f746d13a56c9b348ae9ee343c4',
    ('seg', 2, 512, 17): 'fabec5899175faedec43eabd4a965912d84e159ba385ecd25b3e58bcd2da1186',
}


@pytest.mark.parametrize('key', sorted(DEFAULT_DIGESTS))
def test_default_batches_are_unchanged(key):
    task, bs, size, seed = key
    assert batch_digest(synth.make_batch(task, bs, size, seed=seed)) == DEFAULT_DIGESTS[key]


def test_explicit_full_shapes_draw_the_default_batch():
    """A square canvas given as a tuple, with every image filling it, is the default batch."""
    for task in ('cls', 'det', 'seg'):
        a = synth.make_batch(task, 2, 64, seed=3)
        b = synth.make_batch(task, 2, (64, 64), seed=3, img_shapes=[(64, 64), (64, 64)])
        assert batch_digest(a) == batch_digest(b), task


@pytest.mark.parametrize('canvas,shapes', [((64, 96), [(64, 70), (50, 96)]), ((96, 64), [(96, 64), (33, 17), (80, 40)]),
                                           ((512, 512), [(512, 384), (448, 512)])])
def test_padded_batch_layout(canvas, shapes):
    H, W = canvas
    B = len(shapes)
    for task in ('cls', 'det', 'seg'):
        b = synth.make_batch(task, B, canvas, seed=5, img_shapes=shapes)
        assert b['img'].shape == (B, 3, H, W)
        for i, ((h, w), m) in enumerate(zip(shapes, b['img_metas'])):
            assert m['img_shape'] == m['ori_shape'] == (h, w, 3) and m['pad_shape'] == (H, W, 3)
            img = b['img'][i]
            # mmdet Pad after Normalize: zeros outside the image, the image itself untouched
            assert torch.equal(img[:, h:], torch.zeros_like(img[:, h:])) and torch.equal(img[:, :, w:], torch.zeros_like(img[:, :, w:]))
            assert bool((img[:, :h, :w] != 0).all())
        if task == 'det':
            assert len(b['gt_bboxes']) == len(b['gt_bboxes_host']) == B
            for (h, w), bx, hb, lab, hl in zip(shapes, b['gt_bboxes'], b['gt_bboxes_host'], b['gt_labels'], b['gt_labels_host']):
                assert bx.dtype == torch.float32 and bx.shape[0] >= 1 and bx.shape == (lab.shape[0], 4)
                assert np.array_equal(bx.numpy(), hb) and np.array_equal(lab.numpy(), hl)
                assert bool((bx[:, 0] >= 0).all() and (bx[:, 1] >= 0).all()), bx
                assert bool((bx[:, 2] <= w).all() and (bx[:, 3] <= h).all()), (bx, h, w)
                assert bool((bx[:, 2] > bx[:, 0]).all() and (bx[:, 3] > bx[:, 1]).all())
        if task == 'seg':
            lab = b['gt_semantic_seg']
            assert lab.shape == (B, 1, H, W) and lab.dtype == torch.int64
            for i, (h, w) in enumerate(shapes):
                assert bool((lab[i, :, h:] == 255).all() and (lab[i, :, :, w:] == 255).all())
                inside = lab[i, :, :h, :w]
                assert bool(((inside < 5) | (inside == 255)).all()) and float((inside == 255).float().mean()) < 0.1


def test_bad_image_shapes_are_refused():
    with pytest.raises(AssertionError):
        synth.make_batch('det', 2, (64, 96), img_shapes=[(64, 97), (64, 96)])
    with pytest.raises(AssertionError):
        synth.make_batch('det', 2, 64, img_shapes=[(64, 64)])
