"""The fused Dice seg loss (ops.upsample_dice: rscotr_upsample_dice_fwd / _bwd) forward + backward at two shapes — logits
2 x 100 x 64 x 64 (scheme 2) and 2 x 6 x 64 x 64 (scheme 1), labels 512 x 512, 10 % of the pixels ignored — against two yardsticks
measured in the same run:
    torch composition   interpolate -> softmax -> one-hot -> sums -> autograd on the device: what a user writes without the kernel
                        (it materialises the up-sampled logits and the probabilities)
    upsample_ce         ops.upsample_ce forward + backward at the same shape: sets the scale
us per forward + backward pair (and per forward alone) from device events around warmed-up, alternating rounds; then the seg
iteration of the benchmark config (batch 2, 512 x 512, the iteration captured in a graph as the product runs it) with
loss_decode = [CE] and [CE, Dice(loss_weight=3)].
`python scripts/bench_seg_dice.py [pairs per window] [iterations per window]`: small windows suit a kernel-trace run, which gives
the per-kernel times; 0 pairs skips the op part, 0 iterations the model part."""
import copy, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from rscotr_amd import ops

dev = torch.device('cuda:0')
h, w, H, W = 64, 64, 512, 512
ROUNDS = 5
N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
# library launches per pair: Dice = forward kernel + fold / coefficients, per-pixel S pass + gather; CE = forward kernel + fold, gather
LAUNCHES = {'upsample_dice': 4, 'upsample_ce': 3}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def torch_dice(logit, label, ignore_index=255, smooth=1.0, loss_weight=1.0):
    C = logit.shape[1]
    p = F.softmax(F.interpolate(logit, size=label.shape[-2:], mode='bilinear', align_corners=False), dim=1)
    t = F.one_hot(label.clamp(0, C - 1), C).permute(0, 3, 1, 2).to(p.dtype)
    v = (label != ignore_index).to(p.dtype).unsqueeze(1)
    num = 2 * (p * t * v).flatten(2).sum(-1) + smooth
    den = (p * p + t).flatten(2).sum(-1) + smooth
    return loss_weight * (1 - num / den).mean(0).sum() / C


def bench_shape(B, C):
    g = torch.Generator().manual_seed(0)
    logit = (torch.randn(B, C, h, w, generator=g) * 3).to(dev).requires_grad_(True)
    label = torch.randint(0, C, (B, H, W), generator=g)
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

    dice = lambda: ops.upsample_dice(logit, label, 255, loss_weight=3.0)
    comp = lambda: torch_dice(logit, label, 255, loss_weight=3.0)
    ce = lambda: ops.upsample_ce(logit, label, 255)[0]
    a, b = dice().detach(), comp().detach()
    ga, gb = pair(dice)(), pair(comp)()
    print(f'B={B} C={C} {h}x{w} -> {H}x{W}: fused loss {float(a):.7f}  torch composition (fp32) {float(b):.7f}  '
          f'gradient difference {float((ga - gb).abs().max() / gb.abs().max()):.2e} of the largest', flush=True)
    fns = {'upsample_dice': pair(dice), 'torch composition': pair(comp), 'upsample_ce': pair(ce),
           'upsample_dice fwd': fwd(dice), 'torch composition fwd': fwd(comp), 'upsample_ce fwd': fwd(ce)}
    for fn in fns.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
        for k, fn in fns.items():
            times[k].append(timed(fn, max(N // 10, 3) if 'torch' in k else N))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k in fns:
        print(f'  {k:22s} median {med[k] * 1e3:9.1f} us   min {min(times[k]) * 1e3:9.1f}   max {max(times[k]) * 1e3:9.1f}', flush=True)
    bwd = {k: med[k] - med[k + ' fwd'] for k in ('upsample_dice', 'upsample_ce')}
    # algorithmic bytes of the fused pair (the _Prof brackets of ops/losses.py)
    nbytes = 20 * B * C * h * w + 48 * B * H * W
    print(f'  torch composition / upsample_dice = {med["torch composition"] / med["upsample_dice"]:.1f}x   '
          f'upsample_dice / upsample_ce = {med["upsample_dice"] / med["upsample_ce"]:.2f}x   '
          f'backward alone (pair - forward): dice {bwd["upsample_dice"] * 1e3:.1f} us, ce {bwd["upsample_ce"] * 1e3:.1f} us '
          f'({bwd["upsample_dice"] / max(bwd["upsample_ce"], 1e-9):.2f}x)', flush=True)
    print(f'  {LAUNCHES["upsample_dice"]} library launches per Dice pair ({LAUNCHES["upsample_ce"]} per CE pair); '
          f'{nbytes / 1e6:.1f} MB algorithmic = {nbytes / (med["upsample_dice"] * 1e-3) / 1e12:.3f} TB/s over the pair '
          f'(these kernels are bound by their exponentials and LDS traffic, not by HBM)', flush=True)


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
    # one configuration after the other: the optimizer's gradient arena and the weight-plane caches are process-wide, so a
    # second live runner would pull them from under the first one's captured graph
    for name, loss_decode in (('[CE]', [ce]), ('[CE, Dice]', [ce, dict(type='DiceLoss', loss_name='loss_dice', loss_weight=3.0)])):
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
        print(f'  seg iteration {name:12s} median {sorted(v)[1]:7.2f} ms   min {min(v):7.2f}   max {max(v):7.2f}   (3 windows x {ITERS})', flush=True)
        r.optimizer.close()
        del r, model


print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
if N > 0:
    bench_shape(2, 100)
    bench_shape(2, 6)
if ITERS > 0:
    bench_iteration()
