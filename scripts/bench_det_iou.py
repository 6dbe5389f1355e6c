"""The kind-parameterised det loss launches at the shapes of a det iteration (S = 7 prediction sets, B = 2, Q = 900 queries,
C = 20 classes, G = 32 padded ground truths; 10 % of the queries matched):
    box loss     ops.box_loss_sums (the default recipe's GIoU) next to ops.box_loss_sums_kind for giou / iou (three modes) /
                 diou / ciou: one launch writes both sums and both gradients
    match cost   ops.match_cost_batched next to ops.match_cost_batched_kind for giou / iou
    class loss   ops.sigmoid_focal_loss_sum next to ops.quality_focal_loss_sum
us per forward call (the backward of each is one broadcast multiply in torch, the same for every kind) from device events
around warmed-up, alternating rounds.  `python scripts/bench_det_iou.py [calls per window]`: a small window suits a
kernel-trace run, which gives the per-kernel times."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rscotr_amd import ops

dev = torch.device('cuda:0')
S, B, Q, C, G = 7, 2, 900, 20, 32
ROUNDS = 5
N = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def boxes(g, *shape):
    return torch.cat([torch.rand(*shape, 2, generator=g) * 0.8 + 0.1, torch.rand(*shape, 2, generator=g) * 0.3 + 0.02], -1)


def main():
    g = torch.Generator().manual_seed(0)
    pred, tgt = boxes(g, S, B, Q), boxes(g, S, B, Q)
    pos = torch.rand(S, B, Q, 1, generator=g) < 0.1
    tgt = torch.where(pos, pred + 0.02 * torch.randn(S, B, Q, 4, generator=g), torch.zeros_like(tgt))
    w = pos.float().expand(-1, -1, -1, 4).contiguous()
    fac = torch.tensor([[512., 512., 512., 512.], [400., 300., 400., 300.]])
    cls = torch.randn(S, B, Q, C, generator=g) * 2
    lab = torch.where(pos[..., 0], torch.randint(0, C, (S, B, Q), generator=g), torch.full((S, B, Q), C))
    gt = boxes(g, B, G)
    gt = torch.cat([gt[..., :2] - 0.5 * gt[..., 2:], gt[..., :2] + 0.5 * gt[..., 2:]], -1) * fac[:, None]
    gl = torch.randint(0, C, (B, G), generator=g)
    pred, tgt, w, fac, cls, lab, gt, gl = (x.to(dev) for x in (pred, tgt, w, fac, cls, lab, gt, gl))
    cost_args = (2.0, 5.0, 2.0, 0.25, 2.0, 1e-12)
    cls2, lab2, pred2, tgt2 = cls.view(S, B * Q, C), lab.view(S, B * Q), pred.view(S, B * Q, 4), tgt.view(S, B * Q, 4)
    fns = {'box_loss_sums (giou)': lambda: ops.box_loss_sums(pred, tgt, w, fac, 1e-6)}
    for kind, mode in (('giou', 'log'), ('iou', 'log'), ('iou', 'linear'), ('iou', 'square'), ('diou', 'log'), ('ciou', 'log')):
        fns[f'box_loss_sums_kind {kind}' + (f'/{mode}' if kind == 'iou' else '')] = \
            lambda kind=kind, mode=mode: ops.box_loss_sums_kind(pred, tgt, w, fac, kind, 1e-6, mode)
    fns['match_cost_batched (giou)'] = lambda: ops.match_cost_batched(cls, pred, gt, gl, fac, *cost_args)
    for m in ('giou', 'iou'):
        fns[f'match_cost_batched_kind {m}'] = lambda m=m: ops.match_cost_batched_kind(cls, pred, gt, gl, fac, *cost_args, m)
    fns['sigmoid_focal_loss_sum'] = lambda: ops.sigmoid_focal_loss_sum(cls2, lab2, 2.0, 0.25)
    fns['quality_focal_loss_sum'] = lambda: ops.quality_focal_loss_sum(cls2, lab2, pred2, tgt2, 2.0)
    print(f'device: {torch.cuda.get_device_name(0)}   S={S} B={B} Q={Q} C={C} G={G}   {ROUNDS} rounds x {N} calls', flush=True)
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(5):
                fn()
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):  # alternate the variants: clock and neighbours drift together
            for k, fn in fns.items():
                times[k].append(timed(fn, N))
    for k, v in times.items():
        print(f'  {k:32s} median {sorted(v)[len(v) // 2] * 1e3:8.1f} us   min {min(v) * 1e3:8.1f}   max {max(v) * 1e3:8.1f}', flush=True)


if __name__ == '__main__':
    main()
