"""Recorded dataset pipelines of the reference's DINO det recipe, for tests/test_det_autoaug_cpu.py.

The reference's configs/det/dino_4scale_swin-t-p4-w7_1x1_50e_dior.py (which inherits dino_4scale_r50_1x1_50e_dior.py) is loaded
with rscotr_amd.Config, and its `data.train.pipeline` and `data.test.pipeline` are stored as plain JSON (tuples as lists) in
tests/golden/reference_det_pipeline.json.  Nothing of the reference's text is stored: only what loading it produced.

Re-run:  python tests/golden/make_det_pipeline_golden.py REFERENCE_ROOT
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'reference_det_pipeline.json')
CONFIG = os.path.join('configs', 'det', 'dino_4scale_swin-t-p4-w7_1x1_50e_dior.py')


def plain(o):
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    return o


def main(ref_root):
    sys.path.insert(0, ROOT)
    from rscotr_amd import Config
    cfg = Config.fromfile(os.path.join(ref_root, CONFIG), import_custom_modules=False)  # (its model code is not needed)
    out = dict(config=CONFIG.replace(os.sep, '/'), train=plain(cfg.data['train']['pipeline']),
               test=plain(cfg.data['test']['pipeline']))
    with open(OUT, 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', OUT, [t['type'] for t in out['train']], [t['type'] for t in out['test']])


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
