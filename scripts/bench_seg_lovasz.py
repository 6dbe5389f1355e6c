"""The fused Lovasz-softmax seg loss (ops.upsample_lovasz: rscotr_upsample_lovasz_fwd / _bwd) forward + backward at two shapes —
logits 2 x 7 x 64 x 64 (scheme 1, the step's shape; classes='present') and 2 x 100 x 64 x 64 (scheme 2) with
classes=[0 .. 5], labels 512 x 512, 10 % of the pixels ignored — against two yardsticks measured in the same run:
    torch composition   interpolate -> softmax -> per class |fg - p|, torch.sort, the Jaccard differences, a dot product ->
                        autograd on the device: what a user writes without the kernel (it materialises the up-sampled logits and
                        the probabilities, and synchronises with the host for 'present')
    upsample_ce         ops.upsample_ce forward + backward at the same shape: sets the scale
us per forward + backward pair (and per forward alone) from device events around warmed-up, alternating rounds, and the
workspace of the sort; then the seg iteration of the benchmark config (batch 2, 512 x 512, the iteration captured in a graph as
the product runs it) with loss_decode = [CE] and [CE, Lovasz(reduction='none', loss_weight=3)].
`python scripts/bench_seg_lovasz.py [pairs per window] [iterations per window]`: small windows suit a kernel-trace run, which
gives the per-kernel times; 0 pairs skips the op part, 0 iterations the model part."""
import copy, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from rscotr_amd import ops
from rscotr_amd.ops.core import lib

dev = torch.device('cuda:0')
h, w, H, W = 64, 64, 512, 512
ROUNDS = 5
N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
# library launches per pair: Lovasz = memset + key pass + plan + 4 x (histogram, scan, scatter) + count + apply + fold, then the
# per-pixel S pass + gather; CE = forward kernel + fold, gather
LAUNCHES = {'upsample_lovasz': 3 + 12 + 3 + 2, 'upsample_ce': 3}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def torch_lovasz(logit, label, ignore_index=255, classes='present', loss_weight=1.0):
    C = logit.shape[1]
    p = F.softmax(F.interpolate(logit, size=label.shape[-2:], mode='bilinear', align_corners=False), dim=1)
    p = p.permute(0, 2, 3, 1).reshape(-1, C)
    lab = label.reshape(-1)
    valid = lab != ignore_index
    p, lab = p[valid], lab[valid]
    losses = []
    for c in (range(C) if isinstance(classes, str) else classes):
        fg = (lab == c).to(p.dtype)
        if classes == 'present' and fg.sum() == 0:
            continue
        err, perm = torch.sort((fg - p[:, c]).abs(), dim=0, descending=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1 - (gts - fs.cumsum(0)) / (gts + (1 - fs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(err, jac))
    return loss_weight * torch.stack(losses).mean()


def bench_shape(B, C, classes):
    g = torch.Generator().manual_seed(0)
    logit = (torch.randn(B, C, h, w, generator=g) * 3).to(dev).requires_grad_(True)
    label = torch.randint(0, C if isinstance(classes, str) else len(classes), (B, H, W), generator=g)
    label = torch.where(torch.rand(B, H, W, generator=g) < 0.6,
                        F.interpolate(logit.detach().cpu(), size=(H, W), mode='bilinear').argmax(1), label)
    label[torch.rand(B, H, W, generator=g) < 0.1] = 255
    label = label.to(dev)

    def pair(f):
        return lambda: torch.autograd.grad(f(), logit)[0]

    def fwd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    lov = lambda: ops.upsample_lovasz(logit, label, 255, classes=classes, loss_weight=3.0)
    comp = lambda: torch_lovasz(logit, label, 255, classes, loss_weight=3.0)
    ce = lambda: ops.upsample_ce(logit, label, 255)[0]
    a, b = lov().detach(), comp().detach()
    ga, gb = pair(lov)(), pair(comp)()
    nslots = C if isinstance(classes, str) else len(classes)
    nws = lib.rscotr_upsample_lovasz_workspace(B, C, nslots, H, W, 0)
    print(f'B={B} C={C} classes={classes if isinstance(classes, str) else "list of %d" % nslots} {h}x{w} -> {H}x{W}: fused loss '
          f'{float(a):.7f}  torch composition (fp32, unstable sort, differenced Jaccard) {float(b):.7f}  gradient difference '
          f'{float((ga - gb).abs().max() / gb.abs().max()):.2e} of the largest', flush=True)
    print(f'  workspace {nws / 1e6:.1f} MB + gradient plane {4 * nslots * B * H * W / 1e6:.1f} MB '
          f'({(nws + 4 * nslots * B * H * W) / (nslots * B * H * W):.1f} B per slot and pixel)', flush=True)
    fns = {'upsample_lovasz': pair(lov), 'torch composition': pair(comp), 'upsample_ce': pair(ce),
           'upsample_lovasz fwd': fwd(lov), 'torch composition fwd': fwd(comp), 'upsample_ce fwd': fwd(ce)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
        for k, fn in fns.items():
            times[k].append(timed(fn, max(N // 10, 3) if 'torch' in k else N))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k in fns:
        print(f'  {k:22s} median {med[k] * 1e3:9.1f} us   min {min(times[k]) * 1e3:9.1f}   max {max(times[k]) * 1e3:9.1f}', flush=True)
    bwd = {k: med[k] - med[k + ' fwd'] for k in ('upsample_lovasz', 'upsample_ce')}
    print(f'  torch composition / upsample_lovasz = {med["torch composition"] / med["upsample_lovasz"]:.1f}x   '
          f'upsample_lovasz / upsample_ce = {med["upsample_lovasz"] / med["upsample_ce"]:.2f}x   '
          f'backward alone (pair - forward): lovasz {bwd["upsample_lovasz"] * 1e3:.1f} us, ce {bwd["upsample_ce"] * 1e3:.1f} us',
          flush=True)
    print(f'  {LAUNCHES["upsample_lovasz"]} library launches per Lovasz pair ({LAUNCHES["upsample_ce"]} per CE pair)', flush=True)


def bench_iteration():
    from rscotr_amd import Config, MODELS, synth
    from rscotr_amd.optim import build_optimizer
    from rscotr_amd.runner import IterBasedRunner
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'multi',
                        'MTL_slvlcls_swin-t-p4-w7_1x1_resisc&dior&potsdam.py')
    cfg = Config.fromfile(path)
    batches = [synth.make_batch('seg', 2, 512, seed=100 + i, device=dev) for i in range(4)]

    class Loop:
        def __iter__(self):
            i = 0
            while True:
                b = batches[i % 4]
                i += 1
                yield dict(b, img_metas=[dict(m) for m in b['img_metas']])

    ce = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
    lov = dict(type='LovaszLoss', loss_name='loss_lovasz', reduction='none', loss_weight=3.0)
    # one configuration after the other: the optimizer's gradient arena and the weight-plane caches are process-wide, so a
    # second live runner would pull them from under the first one's captured graph
    for name, loss_decode in (('[CE]', [ce]), ('[CE, Lovasz]', [ce, lov])):
        mcfg = copy.deepcopy(cfg.model)
        mcfg['seg_head']['loss_decode'] = loss_decode
        torch.manual_seed(0)
        np.random.seed(2022)
        model = MODELS.build(mcfg)
        model.init_weights()
        model.to(dev).train()
        r = IterBasedRunner(model, build_optimizer(model, cfg.optimizer, cfg.optimizer_config), Loop(), graph_tasks=('seg',))
        for _ in range(4):
            out = r.train_iter()
        print(f'  {name}: log_vars {dict(out["log_vars"])}', flush=True)
        v = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(ITERS):
                r.train_iter()
            torch.cuda.synchronize()
            v.append((time.time() - t0) / ITERS * 1e3)
        print(f'  seg iteration {name:14s} median {sorted(v)[1]:7.2f} ms   min {min(v):7.2f}   max {max(v):7.2f}   (3 windows x {ITERS})', flush=True)
        r.optimizer.close()
        del r, model


print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
if N > 0:
    bench_shape(2, 7, 'present')
    bench_shape(2, 100, list(range(6)))
if ITERS > 0:
    bench_iteration()
