"""Seeded synthetic batches for the three tasks: the benchmark and the parity
tests feed the product path and the oracle from this one generator.  Shapes follow what the
reference's pipelines hand to `MTL.forward` (configs/_base_/{cls,det,seg}/*.py), data are random.
"""
import numpy as np
import torch

TASK_DATASET = dict(cls='resisc', det='dior', seg='potsdam')


def make_batch(task, batch_size=2, size=512, seed=0, device='cpu', num_cls=45, num_det=20, num_seg=5,
               max_gt=20, img_shapes=None):
    """`size` is the canvas: an int (square) or an (H, W) tuple.  `img_shapes` (one (h, w) per image, h <= H, w <= W)
    places each image in the top-left corner of the canvas, as mmdet's Pad does after Normalize: pixels outside it are 0,
    its seg labels there are 255 (seg_pad_val), its det boxes lie inside it, and its metas carry img_shape = ori_shape =
    (h, w, 3), pad_shape = (H, W, 3).  With an int size and no img_shapes the draws are those of a square, unpadded batch."""
    H, W = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if img_shapes is None:
        img_shapes = [(H, W)] * batch_size
    img_shapes = [(int(h), int(w)) for h, w in img_shapes]
    assert len(img_shapes) == batch_size and all(0 < h <= H and 0 < w <= W for h, w in img_shapes), (img_shapes, H, W)
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    img = torch.randn(batch_size, 3, H, W, generator=g)
    for i, (h, w) in enumerate(img_shapes):
        img[i, :, h:, :] = 0
        img[i, :, :, w:] = 0
    metas = [dict(img_shape=(h, w, 3), ori_shape=(h, w, 3), pad_shape=(H, W, 3),
                  scale_factor=1.0, flip=False, filename=f'synthetic_{seed}_{i}') for i, (h, w) in enumerate(img_shapes)]
    batch = dict(task=task, dataset_name=TASK_DATASET[task], img=img.to(device), img_metas=metas)
    if task == 'cls':
        batch['gt_label'] = torch.from_numpy(rs.randint(0, num_cls, batch_size)).long().to(device)
    elif task == 'det':
        boxes, labels, hboxes, hlabels = [], [], [], []
        for h, w in img_shapes:
            G = int(rs.randint(1, max_gt + 1))
            cxy = rs.uniform(0.1, 0.9, (G, 2)) * np.array([w, h])
            wh = rs.uniform(16, min(200, min(h, w) / 2), (G, 2))
            b = np.concatenate([cxy - wh / 2, cxy + wh / 2], 1).clip(0, np.array([w, h, w, h])).astype(np.float32)
            lab = rs.randint(0, num_det, G).astype(np.int64)
            boxes.append(torch.from_numpy(b).to(device))
            labels.append(torch.from_numpy(lab).to(device))
            hboxes.append(b)
            hlabels.append(lab)
        batch['gt_bboxes'], batch['gt_labels'] = boxes, labels
        # host copies of the ground truth, explicitly in the batch (the det head lays a batch out on the host when it gets
        # them: DetStatic checks them against the device tensors' shapes)
        batch['gt_bboxes_host'], batch['gt_labels_host'] = hboxes, hlabels
    elif task == 'seg':
        blk = 32 if min(H, W) >= 64 else 8
        coarse = rs.randint(0, num_seg, (batch_size, 1, (H + blk - 1) // blk, (W + blk - 1) // blk))
        lab = np.kron(coarse, np.ones((1, 1, blk, blk), dtype=np.int64))[:, :, :H, :W]
        lab[rs.uniform(size=lab.shape) < 0.02] = 255
        for i, (h, w) in enumerate(img_shapes):
            lab[i, :, h:, :] = 255
            lab[i, :, :, w:] = 255
        batch['gt_semantic_seg'] = torch.from_numpy(lab).long().to(device)
    else:
        raise ValueError(task)
    return batch


def make_rnd(model, batch, seed=0, device='cpu', drop_path=True):
    """Explicit stochastic draws for one step: DropPath keep flags, the cls augment, CDN noise."""
    g = torch.Generator().manual_seed(seed + 12345)
    B = batch['img'].shape[0]
    rnd = {}
    rates = torch.tensor(model.backbone.drop_path_rates).repeat_interleave(2)
    if drop_path and float(rates.max()) > 0:
        rnd['drop_keep'] = torch.floor((1 - rates)[:, None] + torch.rand(rates.shape[0], B, generator=g)).to(device)
    else:
        rnd['drop_keep'] = None
    if batch['task'] == 'cls' and model.cls_augments is not None:
        rnd['cls_aug'] = model.cls_augments.draw(B, batch['img'].shape[-2:], np.random.RandomState(seed + 7))
    if batch['task'] == 'det':
        gen = model.bbox_head.dn_generator
        counts = [int(l.shape[0]) for l in batch['gt_labels']]
        ng = gen.get_num_groups(max(counts))
        K = 2 * ng * sum(counts)
        rnd['cdn'] = dict(label_p=torch.rand(K, generator=g).to(device),
                          new_label=torch.randint(0, gen.num_classes, (K,), generator=g).to(device),
                          rand_sign=torch.randint(0, 2, (K, 4), generator=g).float().to(device),
                          rand_part=torch.rand(K, 4, generator=g).to(device))
    return rnd


def to_cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_cpu(v) for v in obj)
    return obj
