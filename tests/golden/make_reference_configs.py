"""Recorded values of the reference's own config files and of its `train_model` signature, for tests/test_host_cpu.py.

Each config file under the reference's configs/multi (and configs/multi/slvl_strategies) is loaded with rscotr_amd.Config,
and its model / optimizer / schedule fields are stored as plain JSON (tuples as lists; machine-local checkpoint paths, which
the reference hard-codes under /home/, as null).  The argument names and defaults of `train_model` in mtl/apis/train.py are
read with `ast`.  Nothing of the reference's text is stored: only what loading it produced, in
tests/golden/reference_configs.json.

Re-run:  python tests/golden/make_reference_configs.py REFERENCE_ROOT
"""
import ast
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'reference_configs.json')
KEYS = ('model', 'optimizer', 'optimizer_config', 'lr_config', 'runner', 'dist_params')


def plain(o):
    """dict / list skeleton of a config value; machine-local checkpoint paths become None."""
    if isinstance(o, str) and o.startswith('/home/'):
        return None
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    return o


def main(ref_root):
    sys.path.insert(0, ROOT)
    from rscotr_amd import Config
    multi = os.path.join(ref_root, 'configs', 'multi')
    files = sorted(glob.glob(os.path.join(multi, '*.py')) + glob.glob(os.path.join(multi, 'slvl_strategies', '*.py')))
    configs = {}
    for path in files:
        if os.path.basename(path) == 'default_runtime.py':
            continue
        cfg = Config.fromfile(path)
        configs[os.path.relpath(path, multi)] = {k: plain(cfg.get(k)) for k in KEYS}
    with open(os.path.join(ref_root, 'mtl', 'apis', 'train.py')) as fh:
        fn = [n for n in ast.parse(fh.read()).body if isinstance(n, ast.FunctionDef) and n.name == 'train_model'][0]
    train_model = dict(args=[a.arg for a in fn.args.args], defaults=[ast.literal_eval(d) for d in fn.args.defaults])
    with open(OUT, 'w') as fh:
        json.dump(dict(configs=configs, train_model=train_model), fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', OUT, len(configs), 'configs')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
