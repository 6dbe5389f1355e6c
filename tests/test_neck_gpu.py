"""Token-layout neck kernels (GroupNorm, 3x3/s2 im2col conv, patchify conv through the MFMA GEMM) vs
torch.nn.functional on NCHW maps (the layout the reference's ChannelMapper / PatchEmbed run in)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, ref):
    ref = ref.double()
    return float((a.detach().cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))


# csrc/neck.hip: gn_stats_grid (~32 tokens per workgroup, at most 128 chunks per image) and the grid caps of
# gn_apply_kernel (1024 workgroups of 256 float4 lanes) and of the im2col / col2im gathers (4096 workgroups of 256)
def _gn_stats_grid(L):
    chunks = max(1, min((L + 31) // 32, 128))
    tpb = (L + chunks - 1) // chunks
    return tpb, (L + tpb - 1) // tpb


GN_APPLY_CAP = 1024 * 256
GATHER_CAP = 4096 * 256


@pytest.mark.parametrize('B,L,C,G', [(2, 64, 256, 32), (1, 4096, 256, 32), (3, 17, 128, 16), (2, 300, 64, 8),
                                      (2, 1, 256, 32),
                                      (2, 50, 128, 32),    # 4 channels per group: one lane per group
                                      (2, 50, 256, 16),    # 16 per group
                                      (1, 40, 64, 2),      # 32 per group
                                      (2, 33, 64, 1),      # one group spanning the whole token row
                                      (1, 4100, 256, 32),  # chunks recomputed from tokens_per_block; gn_apply's stride loop repeats
                                      (1, 4100, 64, 8)])   # the same chunking with four token rows per wavefront step
def test_groupnorm_tokens(cuda, B, L, C, G):
    from rscotr_amd import ops
    if L > 4096:  # what the two long cases are there for
        assert _gn_stats_grid(L) == (33, 125) and L - 124 * 33 == 8
        assert (L * C // 4 > GN_APPLY_CAP) == (C == 256)
    if G == 1:
        assert (C // G) // 4 == C // 4
    g = torch.Generator().manual_seed(L + C)
    x = torch.randn(B, L, C, generator=g) * 2 + 0.5
    w, b, go = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, L, C, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.group_norm(xr.transpose(1, 2), G, wr, br, 1e-5).transpose(1, 2)
    (yr * go.double()).sum().backward()
    xd, wd, bd = (t.to(cuda).requires_grad_(True) for t in (x, w, b))
    y = ops.group_norm_tokens(xd, G, wd, bd)
    (y * go.to(cuda)).sum().backward()
    assert _rel(y, yr) < 1e-4
    assert _rel(xd.grad, xr.grad) < 1e-4
    assert _rel(wd.grad, wr.grad) < 1e-4
    assert _rel(bd.grad, br.grad) < 1e-4


def _gn_run(ops, cuda, x, w, b, G, go):
    """Forward + backward with the gradient tensor `go` handed to autograd as it is -> (y, dx, dweight, dbias)."""
    xd, wd, bd = (t.to(cuda).requires_grad_(True) for t in (x, w, b))
    y = ops.group_norm_tokens(xd, G, wd, bd)
    y.backward(go)
    return y.detach(), xd.grad, wd.grad, bd.grad


def _gn_bwd_calls(monkeypatch):
    """Records (dy pointer, dy batch stride) of every rscotr_groupnorm_tokens_bwd call."""
    from rscotr_amd._lib import lib
    calls, real = [], lib.call

    def spy(name, *args):
        if name == 'rscotr_groupnorm_tokens_bwd':
            calls.append((args[0], args[12]))
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', spy)
    return calls


def _gn_inputs(B, L, C, G):
    g = torch.Generator().manual_seed(L + C)
    x = torch.randn(B, L, C, generator=g) * 2 + 0.5
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g)


def _gn_check_fp64(x, w, b, G, go, got):
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.group_norm(xr.transpose(1, 2), G, wr, br, 1e-5).transpose(1, 2)
    yr.backward(go.cpu().double())
    for a, ref in zip(got, (yr, xr.grad, wr.grad, br.grad)):
        assert _rel(a, ref) < 1e-4


@pytest.mark.parametrize('C,G', [(256, 32), (64, 8)])
def test_groupnorm_tokens_strided_grad(cuda, monkeypatch, C, G):
    """The gradient of one level is a slice of the gradient over the concatenated levels: the backward kernels read it in
    place through a batch stride larger than L * C.  Same kernels, same summation order as on a dense copy: bit for bit."""
    from rscotr_amd import ops
    B, L, L2 = 2, 17, 64
    x, w, b = _gn_inputs(B, L, C, G)
    big = torch.randn(B, L2 + L, C, generator=torch.Generator().manual_seed(C)).to(cuda)
    go = big[:, L2:L2 + L]
    # the in-place conditions of _GroupNormTokens.backward: otherwise this test would quietly exercise the copy
    assert go.stride() == ((L2 + L) * C, C, 1) and go.stride(0) > L * C and go.stride(0) % 4 == 0
    assert go.storage_offset() != 0 and go.data_ptr() % 16 == 0 and not go.is_contiguous()
    calls = _gn_bwd_calls(monkeypatch)
    strided = _gn_run(ops, cuda, x, w, b, G, go)
    dense_go = go.contiguous()
    dense = _gn_run(ops, cuda, x, w, b, G, dense_go)
    assert calls == [(go.data_ptr(), (L2 + L) * C), (dense_go.data_ptr(), L * C)]
    for a, d in zip(strided, dense):
        assert torch.equal(a, d)
    _gn_check_fp64(x, w, b, G, go, strided)


def test_groupnorm_tokens_misaligned_grad(cuda, monkeypatch):
    """A gradient the kernels cannot read in place (not 16-byte aligned) goes through an aligned copy and still matches."""
    from rscotr_amd import ops
    B, L, C, G = 2, 17, 64, 8
    x, w, b = _gn_inputs(B, L, C, G)
    buf = torch.randn(B * L * C + 1, generator=torch.Generator().manual_seed(5)).to(cuda)
    go = buf[1:].view(B, L, C)
    assert go.data_ptr() % 16 != 0
    calls = _gn_bwd_calls(monkeypatch)
    got = _gn_run(ops, cuda, x, w, b, G, go)
    assert len(calls) == 1 and calls[0][0] != go.data_ptr() and calls[0][0] % 16 == 0 and calls[0][1] == L * C
    _gn_check_fp64(x, w, b, G, go, got)


@pytest.mark.parametrize('B,H,W,C,O', [(2, 16, 16, 768, 256), (1, 7, 5, 32, 8), (2, 13, 13, 64, 16), (1, 1, 1, 8, 4),
                                        (2, 23, 25, 1024, 8)])  # both gathers loop past their grid cap, odd H and W
def test_conv3x3s2_tokens(cuda, B, H, W, C, O):
    from rscotr_amd import ops
    if C == 1024:
        assert B * H * W * C > GATHER_CAP and B * ((H + 1) // 2) * ((W + 1) // 2) * C * 9 > GATHER_CAP
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B, H * W, C, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) * 0.1
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr.transpose(1, 2).reshape(B, C, H, W), wr, None, stride=2, padding=1)
    go = torch.randn(yr.shape, generator=g)
    (yr * go.double()).sum().backward()
    xd, wd = x.to(cuda).requires_grad_(True), w.to(cuda).requires_grad_(True)
    y, hw = ops.conv3x3s2_tokens(xd, (H, W), wd)
    assert hw == tuple(yr.shape[-2:])
    (y * go.flatten(2).transpose(1, 2).to(cuda)).sum().backward()
    assert _rel(y, yr.flatten(2).transpose(1, 2)) < 1e-5
    assert _rel(xd.grad, xr.grad) < 1e-5
    assert _rel(wd.grad, wr.grad) < 1e-5


@pytest.mark.parametrize('H,W', [(64, 64), (30, 22)])  # 30x22 needs the corner padding to a multiple of 4
def test_patch_embed(cuda, H, W):
    from rscotr_amd import ops
    g = torch.Generator().manual_seed(H)
    img = torch.randn(2, 3, H, W, generator=g)
    w, b = torch.randn(96, 3, 4, 4, generator=g) * 0.1, torch.randn(96, generator=g)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pad = F.pad(img.double(), (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4))
    yr = F.conv2d(pad, wr, br, stride=4)
    go = torch.randn(yr.shape, generator=g)
    (yr * go.double()).sum().backward()
    wd, bd = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    y, hw = ops.patch_embed(img.to(cuda), wd, bd, 4)
    assert hw == tuple(yr.shape[-2:])
    (y * go.flatten(2).transpose(1, 2).to(cuda)).sum().backward()
    assert _rel(y, yr.flatten(2).transpose(1, 2)) < 1e-5
    assert _rel(wd.grad, wr.grad) < 1e-5
    assert _rel(bd.grad, br.grad) < 1e-5
