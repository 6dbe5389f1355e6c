"""bench.py's launcher: `python bench.py --gpus N` must START N ranks (one process per GPU over RCCL,
what tools/train.py:173-182 / mtl/apis/train.py:37-46 get from `init_dist(args.launcher, ...)`) and print ONE JSON line with
n_gpus == rccl_ranks == N; an inconsistent --gpus / WORLD_SIZE pair must fail loudly instead of running one rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(kw)
    return env


def test_gpus_flag_that_disagrees_with_the_world_size_fails_loudly():
    """(no GPU needed: the check precedes everything else)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--launcher', 'none'],
                       capture_output=True, text=True, timeout=300, env=_env())
    assert r.returncode != 0 and '--gpus 8' in r.stderr and r.stdout.strip() == ''
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'],
                       capture_output=True, text=True, timeout=300, env=_env(WORLD_SIZE='4', RANK='0', LOCAL_RANK='0'))
    assert r.returncode != 0 and 'WORLD_SIZE=4' in r.stderr and r.stdout.strip() == ''


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_spawn_path_starts_the_ranks_and_prints_one_line(cuda):
    """The N > 1 path of `python bench.py --gpus N` on the one GPU of this box: --launcher spawn re-runs the command under
    torch.distributed.run with one rank, RSCOTR_DIST_SINGLE=1 makes that rank a one-rank RCCL group -> n_gpus == rccl_ranks == 1,
    every task graphed, exactly one JSON line on stdout."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--launcher', 'spawn', '--steps', '2',
                        '--warmup', '1', '--size', '256', '--no-cpu-baseline', '--no-roofline', '--exchange', 'inline'],
                       capture_output=True, text=True, timeout=1100, env=_env(RSCOTR_DIST_SINGLE='1'))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out['n_gpus'] == 1 and out['config']['rccl_ranks'] == 1 and out['config']['exchange'] == 'inline'
    assert out['config']['hipgraph_tasks'] == ['cls', 'det', 'seg'] and out['value'] > 0
    assert 'starting 1 rank(s)' in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_plain_run_and_dumped_outputs_repeat(cuda, tmp_path):
    """A plain `bench.py` run (no --full) prints the headline line only — ms_per_step for exactly --steps timed steps, no
    roofline / per-task / CPU-baseline fields — and --dump-outputs writes float .npy files under 64 MB in all.  Two runs
    with the same arguments start from the same inputs, so what they dump is bitwise equal (the step is deterministic:
    tests/test_determinism_gpu.py)."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f'run{i}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                            '--size', '256', '--dump-outputs', str(d)], capture_output=True, text=True, timeout=550, env=_env())
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        out = json.loads(lines[0])
        assert out['steps'] == 2 and out['ms_per_step'] > 0 and out['value'] > 0 and out['unit'] == 'images/s'
        assert abs(out['value'] - 3 * 2 * 1000.0 / out['ms_per_step']) < 1e-6 * out['value']
        assert not any(k.startswith('roofline') for k in out) and 'cpu_baseline' not in out and 'per_task_ms' not in out
        files = sorted(p.name for p in d.iterdir())
        assert 'params_sample.npy' in files and 'grads_sample.npy' in files
        assert {f.split('.')[1] for f in files if f.startswith('log_vars.')} == {'cls', 'det', 'seg'}
        arrs = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert np.abs(arrs['grads_sample.npy']).max() > 0
        dumps.append(arrs)
    a, b = dumps
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(a[f], b[f]), f
