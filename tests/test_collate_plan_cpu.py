"""The host plans of the device input collate (DeviceCollate's plain, table and RandAugment routes, SegTTACollate), pinned against
a recording made on the commit before rscotr_amd/pipeline.py was split into a package with one plan under the three routes
(tests/golden/make_collate_plan_golden.py wrote tests/golden/collate_plan.npz there).  Everything in front of a launch is host
code: no GPU and no library."""
import importlib.util
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_collate_plan_golden',
                                                  os.path.join(GOLDEN_DIR, 'make_collate_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_collate_plans_match_the_recorded_launches():
    gen = _generator()
    want = np.load(gen.GOLDEN)
    tables, seq = gen.record()
    assert seq == [str(s) for s in want['sequence']]
    assert sorted(tables) == sorted(k for k in want.files if k != 'sequence')
    for k, t in tables.items():
        assert t.dtype == want[k].dtype and t.shape == want[k].shape and np.array_equal(t, want[k]), k
    # what the cases were built to reach
    launches = lambda case: [s.split('|')[1] for s in seq if s.startswith(case + '|rscotr')]
    assert launches('plain_cls') == ['rscotr_img_prep_u8'] and launches('plain_seg') == ['rscotr_img_prep_u8',
                                                                                         'rscotr_seg_label_prep_u8']
    assert launches('aug_seg') == ['rscotr_img_aug_u8', 'rscotr_seg_label_aug_u8'] and launches('aug_seg_nolabels') == ['rscotr_img_aug_u8']
    assert launches('randaug0') == ['rscotr_img_frames_u8', 'rscotr_randaug_u8', 'rscotr_randaug_u8', 'rscotr_img_aug_u8']
    assert launches('randaug_none') == ['rscotr_img_frames_u8', 'rscotr_img_aug_u8'] and len(launches('tta')) == 4
    assert [s.split('|')[2].split(',')[0] for s in seq if s.startswith('empty_') and '|rscotr' in s] == ['0', '0', '0', '0>0', '0>0', '0']
    # the plain det batch and the resized one both flip a box and leave one; plain seg crops one sample and pads another
    for case in ('plain_det', 'aug_det'):
        flips = {'flip:True' in s for s in seq if s.startswith(case + '|meta|')}
        assert flips == {True, False}, case
    m = tables['plain_seg_00_meta']  # {crc, H, W, stride, x0, y0, w, h, flip, 0}
    assert (m[0, 6] < m[0, 2] and m[0, 7] < m[0, 1]) and (m[1, 6] < 40 and m[1, 7] < 48)
    assert np.array_equal(m[:, 4:9], tables['plain_seg_01_meta'][:, 4:9])
    assert (tables['aug_cls_00_meta'][:, 16:18] > 0).all(), 'erase_prob = 1: every sample carries a patch'
    # RandAugment: at least one warp, one statistics operation and one unapplied slot among the recorded slots
    ops = np.concatenate([tables[f'randaug{s}_{k:02d}_rmeta'][:, 0] for s in gen.RA_SEEDS for k in (1, 2)])
    assert np.isin(ops, gen.RA_WARP_OPS).any() and np.isin(ops, (1, 2, 8)).any() and (ops == 0).any()
    assert any(tables[f'randaug{s}_{k:02d}_warp'].size for s in gen.RA_SEEDS for k in (1, 2))
    assert any(s.split(',')[3] == '1' for s in seq if '|rscotr_randaug_u8|' in s), 'a slot that asks for the statistics pass'


def test_recording_leaves_the_library_and_ops_alone():
    from rscotr_amd import ops
    from rscotr_amd._lib import lib
    stream = ops._stream
    _generator().record()
    assert 'call' not in vars(lib) and ops._stream is stream
