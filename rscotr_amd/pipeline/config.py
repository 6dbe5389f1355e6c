"""The mm*-config interpreter of the device input path: a dataset config's pipeline (a list of transform dicts) -> the collate
that runs it."""
from .collate import PHOTOMETRIC, DeviceCollate, SegTTACollate
from .randaug import ra_unsupported

_PASSIVE = {'LoadImageFromFile', 'ImageToTensor', 'ToTensor', 'DefaultFormatBundle', 'Collect', 'Normalize'}
# RandomRotate's place: the collate rotates the cropped, flipped window, in front of the colour stages
_BEFORE_ROTATE = ('Resize', 'RandomCrop', 'RandomFlip', 'RandomResizedCrop', 'RandomRotate')
_AFTER_ROTATE = ('PhotoMetricDistortion', 'Normalize', 'Pad')
_ROTATE_PLACE = ('the device collate rotates the cropped, flipped window, after Resize / RandomCrop / RandomFlip and before '
                 'PhotoMetricDistortion / Normalize / Pad')


def build_collate(task, pipeline_cfg, device, unsupported='raise'):
    """Map an mm* pipeline (a list of transform dicts, as in the dataset configs) to a DeviceCollate.

    Understood: LoadImageFromFile, LoadAnnotations (reduce_zero_label), Resize (mmseg / mmdet img_scale + ratio_range +
    keep_ratio, for 'det' and 'seg' also a list of scales + multiscale_mode 'value' | 'range'; mmcls size + backend +
    interpolation), AutoAugment for task 'det' (policies of Resize and mmdet RandomCrop(crop_type, allow_negative_crop=True)
    behind a RandomFlip: the DETR multi-scale recipe), RandomResizedCrop, RandomCrop, RandomFlip (direction 'horizontal' |
    'vertical', for 'det' also 'diagonal' or a list of directions with mmdet's flip_ratio, a float or a list; an unknown
    direction, or a list for 'cls' / 'seg', raises ValueError), RandomRotate for task 'seg' (prob, degree, pad_val, seg_pad_val,
    center; it stands after Resize / RandomCrop / RandomFlip and before PhotoMetricDistortion / Normalize / Pad: anywhere else,
    or with auto_bound=True, it raises NotImplementedError, for another task ValueError), PhotoMetricDistortion,
    RandomErasing, Normalize, Pad, ImageToTensor, ToTensor, DefaultFormatBundle, Collect, MultiScaleFlipAug (its single
    scale and its transforms; flip=False — for task 'seg' also flip=True, `img_ratios` and several scales, up to
    SEG_TTA_MAX_VIEWS views: the result is then a SegTTACollate) and RandAugment when `policies` is a non-empty list of the 13 implemented types
    (RA_OPS) whose warps ask for 'nearest' or 'bicubic'.  Anything else (a RandAugment with an empty list, another policy or
    another interpolation among them) raises NotImplementedError naming it, unless unsupported='skip': then it is left out and
    listed in `collate.skipped`, and the random stream no longer matches the reference's (the skipped transform's draws are
    not made)."""
    assert unsupported in ('raise', 'skip')
    kw, skipped, norm, tta, seen = dict(flip_prob=0.0), [], None, None, []

    def visit(t, scale=None):
        nonlocal norm, tta
        t = dict(t)
        typ = t.pop('type')
        if 'RandomRotate' in seen and typ in _BEFORE_ROTATE:
            raise NotImplementedError(f'{typ} after RandomRotate: {_ROTATE_PLACE}')
        seen.append(typ)
        if typ in _PASSIVE:
            if typ == 'Normalize':
                norm = t
        elif typ == 'LoadAnnotations':
            kw['reduce_zero_label'] = bool(t.get('reduce_zero_label', False))
        elif typ == 'MultiScaleFlipAug':
            sc, ratios = t.get('img_scale'), t.get('img_ratios')
            rl = [] if ratios is None else (list(ratios) if isinstance(ratios, (list, tuple)) else [ratios])
            # (one ratio other than 1.0 is a one-view plan: the planner applies it, the single-view path below would not)
            several = len(rl) > 1 or any(r != 1.0 for r in rl) or (isinstance(sc, list) and len(sc) != 1)
            if task == 'seg' and (t.get('flip', False) or several):  # test-time augmentation: SegTTACollate plans the views
                tta = dict(img_scale=sc if sc is None or isinstance(sc, list) else tuple(sc), img_ratios=ratios,
                           flip=bool(t.get('flip', False)), flip_direction=t.get('flip_direction', 'horizontal'))
                sc = None
            else:
                if t.get('flip', False):
                    raise NotImplementedError('MultiScaleFlipAug(flip=True)')
                if isinstance(sc, list):
                    if len(sc) != 1:
                        raise NotImplementedError('MultiScaleFlipAug with several scales')
                    sc = sc[0]
            for u in t.get('transforms', []):
                visit(u, tuple(sc) if sc is not None else None)
        elif typ == 'Resize':
            if 'size' in t:  # mmcls
                size = t['size']
                kw['resize'] = dict(size=(size, size) if isinstance(size, int) else tuple(size))
            else:
                sc = t.get('img_scale', scale)
                if tta is not None:  # (the scale is the view's; the other Resize arguments are kept for every view)
                    if sc is not None or t.get('ratio_range') is not None:
                        raise NotImplementedError('Resize with its own img_scale / ratio_range inside a multi-view MultiScaleFlipAug')
                    kw['tta_resize'] = dict(keep_ratio=t.get('keep_ratio', True))
                    kw['resize_backend'] = _backend(t)
                    return
                if sc is None:  # MultiScaleFlipAug(img_scale=None, img_ratios=[1.0]): the image's own size
                    return
                multi = {}
                if isinstance(sc, list):
                    if len(sc) == 1:
                        sc = sc[0]
                    elif task not in ('det', 'seg'):
                        raise NotImplementedError('Resize with several img_scale values')
                    else:  # a scale drawn per sample (mmseg / mmdet Resize.random_select / random_sample)
                        sc, multi = [tuple(v) for v in sc], dict(multiscale_mode=t.get('multiscale_mode', 'range'))
                kw['resize'] = dict(img_scale=sc if multi else tuple(sc), ratio_range=t.get('ratio_range'),
                                    keep_ratio=t.get('keep_ratio', True), **multi)
            kw['resize_backend'] = _backend(t)
        elif typ == 'RandomResizedCrop':
            kw['random_resized_crop'] = {k: t[k] for k in ('size', 'scale', 'ratio', 'max_attempts') if k in t}
            kw['resize_backend'] = _backend(t)
        elif typ == 'RandomCrop':
            cs = t['crop_size']
            kw['crop_size'] = (cs, cs) if isinstance(cs, int) else tuple(cs)
            kw['cat_max_ratio'] = t.get('cat_max_ratio', 1.0)
            kw['ignore_index'] = t.get('ignore_index', 255)
        elif typ == 'AutoAugment' and task == 'det':
            policies = []
            for k, pol in enumerate(t['policies']):
                steps = []
                for u in pol:
                    if u.get('type') in ('Resize', 'RandomCrop'):
                        steps.append(dict(u))
                    elif unsupported == 'skip':
                        skipped.append(u.get('type'))
                    else:
                        raise NotImplementedError(f"AutoAugment policy {k}: {u.get('type')} is not implemented by the device "
                                                  "collate (a policy holds Resize and RandomCrop only; build_collate(..., "
                                                  "unsupported='skip') leaves it out)")
                policies.append(steps)
            kw['auto_augment'] = dict(policies=policies)
        elif typ == 'RandomFlip' and tta is not None:
            pass  # (MultiScaleFlipAug sets the flip of every view)
        elif typ == 'RandomFlip' and 'auto_augment' in kw:
            raise NotImplementedError('RandomFlip after AutoAugment (the chain flips the source in front of its geometry)')
        elif typ == 'RandomFlip':
            kw['flip_prob'] = t.get('flip_prob', t.get('flip_ratio', t.get('prob', 0.0))) or 0.0
            kw['flip_direction'] = t.get('direction', 'horizontal')  # (DeviceCollate validates it for the task)
        elif typ == 'RandomRotate':
            if task != 'seg':
                raise ValueError(f"RandomRotate is mmseg's: task 'seg' only, not {task!r}")
            if t.get('auto_bound', False):
                raise NotImplementedError('RandomRotate(auto_bound=True) changes the frame size')
            late = [s for s in seen[:-1] if s in _AFTER_ROTATE]
            if late:
                raise NotImplementedError(f'RandomRotate after {late[0]}: {_ROTATE_PLACE}')
            kw['rotate'] = t
        elif typ == 'PhotoMetricDistortion':
            kw['photometric'] = dict(PHOTOMETRIC, **t)
        elif typ == 'RandomErasing':
            kw['random_erasing'] = dict(t)
        elif typ == 'Pad':
            if t.get('size_divisor'):
                kw['size_divisor'] = t['size_divisor']
            if t.get('size') is not None and 'crop_size' not in kw:
                raise NotImplementedError('Pad(size=...) without RandomCrop')
            kw['seg_pad_val'] = t.get('seg_pad_val', 255)
        elif typ == 'RandAugment' and ra_unsupported(t) is None:
            kw['rand_augment'] = t
        elif unsupported == 'skip':
            skipped.append(typ)
        else:
            what = f'RandAugment: {ra_unsupported(t)}' if typ == 'RandAugment' else typ
            raise NotImplementedError(f'{what} is not implemented by the device collate (build_collate(..., '
                                      f"unsupported='skip') leaves it out)")
    for t in pipeline_cfg:
        visit(t)
    if 'auto_augment' in kw:  # (it is the whole geometry of its batch, and its launches carry no colour stage)
        for name, key in (('Resize', 'resize'), ('RandomResizedCrop', 'random_resized_crop'), ('RandomCrop', 'crop_size'),
                          ('PhotoMetricDistortion', 'photometric'), ('RandomErasing', 'random_erasing'),
                          ('RandAugment', 'rand_augment')):
            if key in kw:
                raise NotImplementedError(f'{name} together with AutoAugment')
    if tta is not None:
        kw.pop('flip_prob')
        col = SegTTACollate(device, tta, resize=kw.pop('tta_resize', None), img_norm_cfg=norm, **kw)
    else:
        col = DeviceCollate(task, device, img_norm_cfg=norm, **kw)
    col.skipped = skipped
    return col


def _backend(t):
    backend, interp = t.get('backend', 'cv2'), t.get('interpolation', 'bilinear')
    if (backend, interp) not in (('cv2', 'bilinear'), ('pillow', 'bicubic')):
        raise NotImplementedError(f'{t.get("type", "resize")}: backend={backend!r}, interpolation={interp!r} '
                                  "(cv2 bilinear and pillow bicubic are implemented)")
    return backend
