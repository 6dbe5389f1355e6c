"""The seg iteration of the main config at 512^2, B = 2, with Mask2FormerHead scheme 2 (the config's: the 100 mask logits are
the output channels) and scheme 1 (num_classes + 1 class channels mixed from the queries: ops.seg_class_logits), as the
runner executes it (captured and replayed).  ms per iteration from device events around windows of N iterations, the two
schemes alternating (a fresh model and runner per turn: one optimizer arena is live at a time).
`python scripts/bench_seg_scheme.py [iterations per window] [turns]`."""
import copy, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from rscotr_amd import MODELS, Config
from rscotr_amd.data import build_synthetic_multidataloader
from rscotr_amd.runner import build_runner

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'multi',
                   'MTL_slvlcls_swin-t-p4-w7_1x1_resisc&dior&potsdam.py')
dev = torch.device('cuda:0')
N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
TURNS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
WINDOWS, WARM = 3, 6
print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
cfg = Config.fromfile(CFG)
times = {1: [], 2: []}
for turn in range(TURNS):
    for scheme in (2, 1):
        mcfg = copy.deepcopy(cfg.model)
        mcfg['seg_head']['scheme'] = scheme
        torch.manual_seed(0)
        np.random.seed(2022)
        model = MODELS.build(mcfg)
        model.init_weights()
        model.to(dev).train()
        loader = build_synthetic_multidataloader(cfg, dev, size=512, batch_size=2, tasks=('seg',))
        runner = build_runner(model, cfg, loader, logger=lambda m: None)
        with runner.on_stream():
            for _ in range(WARM):
                out = runner.train_iter()
            torch.cuda.synchronize()
            assert 'seg' in runner.graphed, runner.graphed
            for _ in range(WINDOWS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(N):
                    out = runner.train_iter()
                e1.record()
                torch.cuda.synchronize()
                times[scheme].append(e0.elapsed_time(e1) / N)
        print(f'turn {turn} scheme {scheme}: {["%.3f" % t for t in times[scheme][-WINDOWS:]]} ms / iteration, '
              f'last log {dict(out["log_vars"])}', flush=True)
        runner.optimizer.close()
        del runner, model, loader
        torch.cuda.empty_cache()
for s in (2, 1):
    t = sorted(times[s])
    print(f'scheme {s}: median {t[len(t) // 2]:.3f} ms   min {t[0]:.3f}   max {t[-1]:.3f}   ({len(t)} windows x {N} iterations)', flush=True)
m1, m2 = (sorted(times[s])[len(times[s]) // 2] for s in (1, 2))
print(f'scheme 1 / scheme 2 = {m1 / m2:.4f}', flush=True)
