"""High-precision reference of the Swin window-attention core: everything between the qkv Linear and the proj Linear of
mmdet ShiftWindowMSA / WindowMSA, i.e. what csrc/swin_attn.hip computes (pad, roll, 7x7 partition, q k^T / sqrt(32) +
relative-position bias [+ -100 shift mask], softmax, P v, window reverse, un-roll, crop).

Built from oracle.model's window_partition / window_reverse / rel_pos_index and the mask slices of shift_window_msa, so
that F.linear(core(F.linear(x, Wqkv, bqkv)), Wproj, bproj) restates oracle.model.shift_window_msa exactly
(tests/test_wattn_oracle_cpu.py).  Runs in autograd: the gradients of qkv, the qkv bias and the table come from
.backward()."""
import torch

from oracle.model import rel_pos_index, window_partition, window_reverse

LOG2E = 1.4426950408889634


def wattn_core(qkv, hw, qkv_bias, table, heads, shift, ws=7, exp='plain'):
    """qkv (B, H*W, 3C), qkv_bias (3C,) | None, table (169, heads) -> (B, H*W, C), in the dtype of the inputs.
    Pad tokens take q = k = v = qkv_bias (zeros without one): in mmdet the qkv Linear acts on the zero padding too.
    exp='plain': torch's softmax.  exp='expf': exp(x) as exp2(fl(x * log2 e)) in the working precision — what the kernel's
    __expf does — on the max-subtracted scores (softmax is invariant to the subtracted constant, so the gradient through the
    detached maximum is exact)."""
    assert exp in ('plain', 'expf')
    B, L, C3 = qkv.shape
    C = C3 // 3
    H, W = hw
    assert L == H * W and C % heads == 0
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    Hp, Wp = H + pad_b, W + pad_r
    padv = qkv_bias if qkv_bias is not None else torch.zeros(C3, dtype=qkv.dtype)
    x = torch.cat([qkv.view(B, H, W, C3), padv.expand(B, H, pad_r, C3)], 2)
    x = torch.cat([x, padv.expand(B, pad_b, Wp, C3)], 1)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        img_mask = torch.zeros((1, Hp, Wp, 1), dtype=qkv.dtype)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img_mask[:, hs, wsl, :] = cnt
                cnt += 1
        mw = window_partition(img_mask, ws).view(-1, ws * ws)
        am = mw.unsqueeze(1) - mw.unsqueeze(2)
        am = am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)
    else:
        am = None
    win = window_partition(x, ws).view(-1, ws * ws, C3)
    Bw, N, _ = win.shape
    hd = C // heads
    t = win.reshape(Bw, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * (hd ** -0.5), t[1], t[2]
    a = q @ k.transpose(-2, -1)
    a = a + table[rel_pos_index(ws).view(-1)].view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
    if am is not None:
        nW = am.shape[0]
        a = (a.view(Bw // nW, nW, heads, N, N) + am.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    if exp == 'expf':
        e = torch.exp2((a - a.amax(-1, keepdim=True).detach()) * LOG2E)
        p = e / e.sum(-1, keepdim=True)
    else:
        p = a.softmax(-1)
    o = (p @ v).transpose(1, 2).reshape(Bw, N, C)
    o = window_reverse(o.view(-1, ws, ws, C), Hp, Wp, ws)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o[:, :H, :W].reshape(B, H * W, C)


def wattn_eval(qkv, hw, qkv_bias, table, heads, shift, dout, dtype, exp='plain'):
    """One evaluation of the core and its backward with the incoming gradient `dout`, all in `dtype` on the CPU ->
    dict(out, dqkv, dqkv_bias (None without a bias), dtable) as float64 tensors."""
    qkv = qkv.detach().cpu().to(dtype).requires_grad_(True)
    qb = None if qkv_bias is None else qkv_bias.detach().cpu().to(dtype).requires_grad_(True)
    tb = table.detach().cpu().to(dtype).requires_grad_(True)
    o = wattn_core(qkv, hw, qb, tb, heads, shift, exp=exp)
    o.backward(dout.detach().cpu().to(dtype))
    return dict(out=o.detach().double(), dqkv=qkv.grad.double(), dqkv_bias=None if qb is None else qb.grad.double(),
                dtable=tb.grad.double())
