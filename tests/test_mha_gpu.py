"""ops.mha (batched MFMA GEMMs + masked softmax kernels through the C ABI) against torch.nn.MultiheadAttention
on the CPU in fp64 — the primitive mmcv's MultiheadAttention wraps: output, input gradients and
all parameter gradients, for the three mask layouts of the co-training step.  Tolerance 1e-3 (north star);
observed ~1e-6."""
import functools

import pytest
import torch

import attn_mask_cases as amc

pytestmark = pytest.mark.gpu


def _rel(a, ref):
    ref = ref.double()
    return float((a.detach().cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize('B,Lq,Lk,mask_kind', [(2, 100, 100, None), (2, 100, 256, 'image'), (2, 830, 830, 'shared'),
                                               (2, 37, 1024, 'head'), (1, 5, 64, 'image'), (2, 100, 4096, 'image'),
                                               (2, 800, 800, 'shared'), (1, 16, 2048, 'image')])
@pytest.mark.parametrize('core', [True, False])  # the fused core (csrc/attn_core.hip, the default) | q k^T -> softmax -> P v
def test_mha_matches_torch(cuda, B, Lq, Lk, mask_kind, core):
    from rscotr_amd import ops
    with ops.STATE.override(attn_core=core):
        _mha_against_torch(cuda, B, Lq, Lk, mask_kind)


def _mha_against_torch(cuda, B, Lq, Lk, mask_kind):
    from rscotr_amd import ops
    C, H = 256, 8
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    ref = torch.nn.MultiheadAttention(C, H, 0.0).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=g).double() * 0.1)
    self_attn = Lq == Lk and mask_kind in (None, 'shared')
    q_in = torch.randn(B, Lq, C, generator=g)
    k_in = q_in if self_attn else torch.randn(B, Lk, C, generator=g)
    v_in = torch.randn(B, Lk, C, generator=g)
    ident = torch.randn(B, Lq, C, generator=g)
    mask = None
    if mask_kind == 'shared':
        mask = torch.rand(Lq, Lk, generator=g) < 0.4
        mask[:, 0] = False
        tmask = mask
    elif mask_kind == 'image':
        mask = torch.rand(B, Lq, Lk, generator=g) < 0.5
        mask[:, :, 3] = False
        tmask = mask[:, None].expand(-1, H, -1, -1).reshape(B * H, Lq, Lk)
    elif mask_kind == 'head':
        mask = torch.rand(B * H, Lq, Lk, generator=g) < 0.5
        mask[:, :, 1] = False
        tmask = mask
    gy = torch.randn(B, Lq, C, generator=g)
    # reference (sequence-first, fp64)
    qr, kr, vr, ir = (t.double().clone().requires_grad_(True) for t in (q_in, k_in, v_in, ident))
    out_ref = ref(qr.transpose(0, 1), kr.transpose(0, 1), vr.transpose(0, 1), attn_mask=None if mask is None else tmask)[0]
    out_ref = out_ref.transpose(0, 1) + ir
    out_ref.backward(gy.double())
    # product
    qd = q_in.to(cuda).requires_grad_(True)
    kd = qd if self_attn else k_in.to(cuda).requires_grad_(True)
    vd, idd = v_in.to(cuda).requires_grad_(True), ident.to(cuda).requires_grad_(True)
    P = {n: p.detach().float().to(cuda).requires_grad_(True) for n, p in ref.named_parameters()}
    out = ops.mha(qd, kd, vd, P['in_proj_weight'], P['in_proj_bias'], P['out_proj.weight'], P['out_proj.bias'], H,
                  None if mask is None else mask.to(cuda), identity=idd)
    out.backward(gy.to(cuda))
    assert _rel(out, out_ref) < 1e-4
    if self_attn:
        assert _rel(qd.grad, qr.grad + kr.grad) < 1e-4
    else:
        assert _rel(qd.grad, qr.grad) < 1e-4 and _rel(kd.grad, kr.grad) < 1e-4
    assert _rel(vd.grad, vr.grad) < 1e-4 and _rel(idd.grad, ir.grad) < 1e-4
    for n, p in ref.named_parameters():
        assert _rel(P[n].grad, p.grad) < 1e-4, n

@pytest.mark.parametrize('B,H,Lq,Lk,mode', [(2, 8, 100, 4096, 2), (2, 8, 800, 800, 1), (1, 3, 45, 37, 3), (3, 2, 1, 1, 0),
                                            (1, 8, 33, 130, 2), (2, 4, 64, 1027, 0), (1, 8, 100, 16384, 2)])
def test_attn_core_against_fp64(cuda, B, H, Lq, Lk, mode):
    """rscotr_attn_core_fwd / _bwd through the C ABI against softmax(scale q k^T + mask) v in fp64 (strided q | k halves of one
    tensor, ragged lengths, every mask layout, key chunks, a fully blocked row -> zeros), twice: bit-identical results."""
    C = H * 32
    g = torch.Generator().manual_seed(B * 1000 + Lq * 7 + Lk)
    self_attn = Lq == Lk
    ldq = 2 * C if self_attn else C
    qk = torch.randn(B, Lq, ldq, generator=g)
    kx = None if self_attn else torch.randn(B, Lk, C, generator=g)
    v, do = torch.randn(B, Lk, C, generator=g), torch.randn(B, Lq, C, generator=g)
    mask = None
    if mode:
        shape = {1: (Lq, Lk), 2: (B, Lq, Lk), 3: (B * H, Lq, Lk)}[mode]
        mask = torch.rand(shape, generator=g) < 0.5
        mask[..., 0] = False
        if Lq > 2:
            mask[..., 2, :] = True  # a fully blocked row: output 0, no gradient through it
    q, k = (qk[..., :C], qk[..., C:]) if self_attn else (qk, kx)
    ref = amc.attn_reference(q, k, v, do, mask, mode, B, H)
    out = _attn_core_check(cuda, B, H, Lq, Lk, mode, self_attn, qk, kx, v, do, mask, ref)[0]
    if mode and Lq > 2:
        assert float(out[:, 2].abs().max()) == 0.0


def _attn_core_workspace(cuda, B, H, Lq, Lk):
    """(bytes, workspace tensor, key chunks of the launch): the chunk count read back from the size the library asks for —
    D = rowsum(dO * O) rounded to 256 bytes, then 1088 floats per (image, head, query block, chunk) when chunked."""
    from rscotr_amd._lib import lib
    nws = int(lib.rscotr_attn_core_workspace(B, H, Lq, Lk))
    nqb = (Lq + 31) // 32
    extra = nws - (B * H * Lq * 4 + 255) // 256 * 256
    assert extra >= 0 and extra % (B * H * nqb * 1088 * 4) == 0
    nch = extra // (B * H * nqb * 1088 * 4) or 1
    return nws, torch.empty(max(nws, 16) // 4, dtype=torch.float32, device=cuda), nch


def _misaligned_copy(t, cuda):
    """A device copy of a bool / uint8 tensor that starts one byte into a larger buffer: its pointer is not 4-byte aligned."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=cuda)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    return view


def _attn_core_check(cuda, B, H, Lq, Lk, mode, self_attn, qk, kx, v, do, mask, ref, misaligned_mask=False, label=None):
    """One case of rscotr_attn_core_fwd / _bwd through the C ABI against the fp64 reference `ref` (attn_mask_cases.attn_reference)
    at the tolerances of this kernel: out 2e-6, gradients 2e-5 (relative to the largest reference value, floor 0.1), lse 1e-5;
    NaN-filled exact-size outputs, two runs with bit-identical results, +inf lse / zero output / zero dq on every fully blocked
    row.  -> (out, lse, dq, dk, dv) of the first run."""
    from rscotr_amd._lib import lib
    hd, C = 32, H * 32
    ldq = 2 * C if self_attn else C
    scale = hd ** -0.5
    dev = lambda t: t.contiguous().to(cuda)
    qk_d = dev(qk)
    k_d = None if self_attn else dev(kx)
    v_d, do_d = dev(v), dev(do)
    m_d = None if mask is None else (_misaligned_copy(mask, cuda) if misaligned_mask else dev(mask))
    nws, ws, _ = _attn_core_workspace(cuda, B, H, Lq, Lk)
    st = torch.cuda.current_stream().cuda_stream
    kp = qk_d.data_ptr() + 4 * C if self_attn else k_d.data_ptr()
    runs = []
    for _ in range(2):
        out = torch.full((B, Lq, C), float('nan'), device=cuda)
        lse = torch.empty(B, H, Lq, device=cuda)
        dqk = torch.full((B, Lq, ldq), float('nan'), device=cuda)
        dk = None if self_attn else torch.full((B, Lk, C), float('nan'), device=cuda)
        dv = torch.full((B, Lk, C), float('nan'), device=cuda)
        mp = 0 if m_d is None else m_d.data_ptr()
        lib.call('rscotr_attn_core_fwd', qk_d.data_ptr(), kp, v_d.data_ptr(), mp, mode, out.data_ptr(), lse.data_ptr(), B, H, Lq,
                 Lk, hd, ldq, ldq, C, C, scale, ws.data_ptr(), nws, st)
        dkp = dqk.data_ptr() + 4 * C if self_attn else dk.data_ptr()
        lib.call('rscotr_attn_core_bwd', qk_d.data_ptr(), kp, v_d.data_ptr(), mp, mode, out.data_ptr(), do_d.data_ptr(),
                 lse.data_ptr(), dqk.data_ptr(), dkp, dv.data_ptr(), B, H, Lq, Lk, hd, ldq, ldq, C, C, ldq, ldq, C, scale,
                 ws.data_ptr(), nws, st)
        torch.cuda.synchronize()
        runs.append((out, lse, dqk, dv) + (() if self_attn else (dk,)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    out, lse, dqk, dv = runs[0][:4]
    dq_p = dqk[..., :C]
    dk_p = dqk[..., C:] if self_attn else runs[0][4]
    def rel(a, ref):  # (a single key: dq = dk = 0 exactly in the reference, rounding noise here -> floor on the denominator)
        return float((a.cpu().double() - ref).abs().max() / max(float(ref.abs().max()), 1e-1))
    lse_ref = ref['lse']
    finite = torch.isfinite(lse_ref)
    err = dict(out=rel(out, ref['out']), dq=rel(dq_p, ref['dq']), dk=rel(dk_p, ref['dk']), dv=rel(dv, ref['dv']),
               lse=float((lse.cpu().double() - lse_ref)[finite].abs().max()))
    if label is not None:
        print(f'[attn_core] {label}: ' + ' '.join(f'{n} {e:.3g}' for n, e in err.items()))
    assert err['out'] < 2e-6
    assert err['dq'] < 2e-5 and err['dk'] < 2e-5 and err['dv'] < 2e-5
    assert torch.equal(torch.isfinite(lse.cpu()), finite)  # (+inf marks a fully blocked row)
    assert err['lse'] < 1e-5
    dead = (~finite).nonzero().tolist()
    if dead:  # a fully blocked row: lse +inf, output exactly 0, no gradient through it
        bi, hi, ri = (torch.tensor(ix) for ix in zip(*dead))
        cols = (hi * 32)[:, None] + torch.arange(32)[None, :]
        lse_c, out_c, dq_c = lse.cpu(), out.cpu(), dq_p.cpu()
        assert bool((lse_c[bi, hi, ri] == float('inf')).all())
        assert float(out_c[bi[:, None], ri[:, None], cols].abs().max()) == 0.0
        assert float(dq_c[bi[:, None], ri[:, None], cols].abs().max()) == 0.0
    return out, lse, dq_p, dk_p, dv


_CORE_CASES = ['dino192', 'dino190', 'dino224', 'region_img', 'region_img_open', 'region_head', 'band_chunked', 'own_plain', 'own_region']


def _run_core_case(cuda, name, **kw):
    c = amc.CASES[name]
    qk, kx, v, do = amc.case_inputs(name)
    return _attn_core_check(cuda, c['B'], c['H'], c['Lq'], c['Lk'], c['mode'], c['self_attn'], qk, kx, v, do, amc.case_mask(name),
                            amc.case_reference(name), label=name + (' (misaligned mask)' if kw.get('misaligned_mask') else ''), **kw)


@pytest.mark.parametrize('name', _CORE_CASES)
def test_attn_core_structured_masks(cuda, name):
    """The fused core on block-structured masks (tests/attn_mask_cases.py; their tile census is asserted by
    test_attn_mask_cases_cpu.py): DINO's denoising mask with interior and ragged tiles (vector / scalar mask reads), region
    masks and a band against chunked keys (a whole chunk blocked, the first tile of every wavefront blocked, a fully blocked
    row), and the key-block-per-wavefront key-side pass with ragged keys — all at the tolerances of the random-mask test."""
    c = amc.CASES[name]
    B, H, Lq, Lk = c['B'], c['H'], c['Lq'], c['Lk']
    nch = _attn_core_workspace(cuda, B, H, Lq, Lk)[2]
    ntiles, nqb, nkb = (Lk + 31) // 32, (Lq + 31) // 32, (Lk + 31) // 32
    if 'chunk_tiles' in c:  # the census of this case was laid out for these chunks: the launch must really be chunked that way
        assert nch > 1 and (ntiles + nch - 1) // nch == c['chunk_tiles']
    if name.startswith('own'):  # the condition under which rscotr_attn_core_bwd gives every wavefront a key block of its own,
        assert nqb <= 8 and (nkb + 3) // 4 * B * H >= 128  # with one live wavefront of 6 keys in the last workgroup
        assert nkb % 4 == 1 and Lk - (nkb - 1) * 32 == 6
    _run_core_case(cuda, name)


def test_attn_core_misaligned_mask_is_bit_identical(cuda):
    """Lk % 4 == 0 with a mask pointer off 4-byte alignment takes the scalar mask reads on interior tiles: same bits as the
    vector reads of the aligned mask, and within tolerance of fp64."""
    aligned = _run_core_case(cuda, 'dino192')
    shifted = _run_core_case(cuda, 'dino192', misaligned_mask=True)
    for a, b in zip(aligned, shifted):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name,misaligned', [('dino192', False), ('dino192', True), ('dino190', False), ('region_img', False),
                                             ('region_img', True)])
def test_softmax_fallback_structured_masks(cuda, name, misaligned):
    """rscotr_softmax_mask_fwd / rscotr_softmax_bwd (the path without the fused core) on the structured masks against the fp64
    softmax and its Jacobian product; a fully blocked row gives zeros.  Tolerance: the 1e-4 test_mha_matches_torch applies."""
    from rscotr_amd._lib import lib
    c = amc.CASES[name]
    B, H, Lq, Lk, mode = c['B'], c['H'], c['Lq'], c['Lk'], c['mode']
    mask = amc.case_mask(name)
    g = torch.Generator().manual_seed(Lq + Lk)
    S, dP = torch.randn(B, H, Lq, Lk, generator=g) * 3, torch.randn(B, H, Lq, Lk, generator=g)
    scale = 32 ** -0.5
    p_ref, ds_ref = amc.softmax_reference(S, mask, mode, B, H, scale, dP)
    m_d = _misaligned_copy(mask, cuda) if misaligned else mask.to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    P, d = S.to(cuda), dP.to(cuda)
    lib.call('rscotr_softmax_mask_fwd', P.data_ptr(), m_d.data_ptr(), mode, B, H, Lq, Lk, scale, st)
    lib.call('rscotr_softmax_bwd', P.data_ptr(), d.data_ptr(), B * H * Lq, Lk, scale, st)
    torch.cuda.synchronize()
    print(f'[softmax] {name} misaligned={misaligned}: P {_rel(P, p_ref):.3g} dS {_rel(d, ds_ref):.3g}')
    assert _rel(P, p_ref) < 1e-4 and _rel(d, ds_ref) < 1e-4
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(d).all())
    blocked = mask.reshape(-1, Lq, Lk).all(-1)  # (blocks, Lq)
    assert int(blocked.sum()) == len(c['blocked'])
    if c['blocked']:
        rows = blocked[0].expand(B, H, Lq) if mode == 1 else \
            (blocked[:, None].expand(B, H, Lq) if mode == 2 else blocked.reshape(B, H, Lq))
        assert float(P.cpu()[rows].abs().max()) == 0.0 and float(d.cpu()[rows].abs().max()) == 0.0


def test_attn_core_rejects_other_head_dims(cuda):
    from rscotr_amd._lib import lib
    t = torch.zeros(4096, device=cuda)
    with pytest.raises(RuntimeError, match='head dim'):
        lib.call('rscotr_attn_core_fwd', t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 0, t.data_ptr(), t.data_ptr(), 1, 1, 4, 4, 64,
                 64, 64, 64, 64, 0.125, 0, 0, torch.cuda.current_stream().cuda_stream)


def test_attn_core_argument_checks(cuda):
    """The error returns of rscotr_attn_core_fwd / _bwd: every call is refused by the argument checks, before any launch."""
    from rscotr_amd._lib import lib
    t = torch.zeros(1 << 16, device=cuda)
    m = torch.zeros(4096, dtype=torch.bool, device=cuda)
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream

    def fwd(q=p, mask=0, mode=0, B=1, H=1, Lq=4, Lk=4, ldq=32, ldk=32, ldv=32, ldo=32, ws=p, nws=1 << 18):
        lib.call('rscotr_attn_core_fwd', q, p, p, mask, mode, p, p, B, H, Lq, Lk, 32, ldq, ldk, ldv, ldo, 0.125, ws, nws, st)

    def bwd(nws, ws=p, B=1, H=1, Lq=4, Lk=4):
        lib.call('rscotr_attn_core_bwd', p, p, p, 0, 0, p, p, p, p, p, p, B, H, Lq, Lk, 32, 32, 32, 32, 32, 32, 32, 32, 0.125, ws, nws, st)

    with pytest.raises(RuntimeError, match='exceeds the grid'):
        fwd(B=8192, H=8, ldq=256, ldk=256, ldv=256, ldo=256)
    with pytest.raises(RuntimeError, match='row stride 32'):
        fwd(H=2, ldq=32, ldk=64, ldv=64, ldo=64)       # below heads * 32
    with pytest.raises(RuntimeError, match='row stride 34'):
        fwd(ldv=34)                                    # not a multiple of 4
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        fwd(q=p + 4)
    with pytest.raises(RuntimeError, match='mask_mode 4'):
        fwd(mask=m.data_ptr(), mode=4)
    with pytest.raises(RuntimeError, match='mask_mode 2'):
        fwd(mask=0, mode=2)
    need = int(lib.rscotr_attn_core_workspace(1, 1, 4, 4))
    assert 0 < need <= 1 << 18
    with pytest.raises(RuntimeError, match='workspace'):
        bwd(need - 1)
    # a chunked forward (one query block against 16 key tiles: two chunks) needs its workspace
    B, H, Lq, Lk = 1, 1, 4, 512
    assert int(lib.rscotr_attn_core_workspace(B, H, Lq, Lk)) > (B * H * Lq * 4 + 255) // 256 * 256
    with pytest.raises(RuntimeError, match='workspace'):
        fwd(Lq=Lq, Lk=Lk, ws=0, nws=0)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0  # nothing ran


@pytest.mark.parametrize('kind', ['self', 'self_const_pos', 'cross', 'cross_const_kpos', 'self_no_identity'])
def test_mha_positional_inputs_and_merged_gradients(cuda, kind):
    """The mmcv wrapper's positional adds and identity inside the node (ops.mha(x, kx, vx, ..., q_pos, k_pos, identity=x)):
    output and the gradients of x, q_pos, the key content and k_pos — merged in GEMM epilogues, no element-wise adds —
    against torch.nn.MultiheadAttention in fp64 with the adds written out."""
    from rscotr_amd import ops
    C, H, B, Lq, Lk = 256, 8, 2, 100, 320
    g = torch.Generator().manual_seed(11)
    ref = torch.nn.MultiheadAttention(C, H, 0.0).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=g).double() * 0.1)
    self_attn = kind.startswith('self')
    x, qp = torch.randn(B, Lq, C, generator=g), torch.randn(B, Lq, C, generator=g)
    kx, kp = torch.randn(B, Lk, C, generator=g), torch.randn(B, Lk, C, generator=g)
    gy = torch.randn(B, Lq, C, generator=g)
    qp_grad = kind != 'self_const_pos'
    kp_grad = kind == 'cross'
    with_id = kind != 'self_no_identity'
    xr, qpr, kxr, kpr = (t.double().clone().requires_grad_(True) for t in (x, qp, kx, kp))
    qq = xr + qpr
    kk, vv = (qq, xr) if self_attn else (kxr + kpr, kxr)
    out_ref = ref(qq.transpose(0, 1), kk.transpose(0, 1), vv.transpose(0, 1))[0].transpose(0, 1)
    if with_id:
        out_ref = out_ref + xr
    out_ref.backward(gy.double())
    xd = x.to(cuda).requires_grad_(True)
    qpd = qp.to(cuda).requires_grad_(qp_grad)
    kxd = kx.to(cuda).requires_grad_(True)
    kpd = kp.to(cuda).requires_grad_(kp_grad)
    P = {n: p.detach().float().to(cuda).requires_grad_(True) for n, p in ref.named_parameters()}
    w = (P['in_proj_weight'], P['in_proj_bias'], P['out_proj.weight'], P['out_proj.bias'])
    if self_attn:
        out = ops.mha(xd, xd, xd, *w, H, None, identity=xd if with_id else None, q_pos=qpd, k_pos=qpd)
    else:
        out = ops.mha(xd, kxd, kxd, *w, H, None, identity=xd, q_pos=qpd, k_pos=kpd)
    out.backward(gy.to(cuda))
    assert _rel(out, out_ref) < 1e-4
    assert _rel(xd.grad, xr.grad) < 1e-4
    if qp_grad:
        assert _rel(qpd.grad, qpr.grad) < 1e-4
    if not self_attn:
        assert _rel(kxd.grad, kxr.grad) < 1e-4
        if kp_grad:
            assert _rel(kpd.grad, kpr.grad) < 1e-4
    for n, p in ref.named_parameters():
        assert _rel(P[n].grad, p.grad) < 1e-4, n


# ----------------------------------------------------------------------------------------------------------------------
# gradient routing of _MHA.backward: which inputs / parameters want a gradient decides which products run and where the
# gradients that meet at x and at the key content are merged
# ----------------------------------------------------------------------------------------------------------------------
_ALL_SELF, _ALL_CROSS = ('x', 'qp', 'kp'), ('x', 'qp', 'kx', 'kp')
_ROUTES = {
    # self-attention with distinct q_pos / k_pos objects: separate q and k projections, d_x = dq_in + dk_in [+ g]
    'split_all': dict(attn='self_split', train=_ALL_SELF, ident='x'),
    'split_all_no_identity': dict(attn='self_split', train=_ALL_SELF, ident=None),
    'split_x_frozen': dict(attn='self_split', train=('qp', 'kp'), ident='x'),
    'split_x_frozen_no_identity': dict(attn='self_split', train=('qp', 'kp'), ident=None),
    # fused self-attention (one q | k projection)
    'fused_x_frozen': dict(attn='self_fused', train=('qp',), ident='x'),
    'fused_pos_frozen_no_identity': dict(attn='self_fused', train=('x',), ident=None),
    'fused_params_only': dict(attn='self_fused', train=(), ident='x'),
    'fused_bias_only': dict(attn='self_fused', train=('x', 'qp'), ident='x', params='bias'),
    # cross-attention
    'cross_key_content_frozen': dict(attn='cross', train=('x', 'qp', 'kp'), ident='x'),
    'cross_k_pos_frozen': dict(attn='cross', train=('x', 'qp', 'kx'), ident='x'),
    'cross_vx_trainable': dict(attn='cross', train=_ALL_CROSS + ('vx',), ident='x', vx=True),
    'cross_vx_frozen': dict(attn='cross', train=_ALL_CROSS, ident='x', vx=True),
    'cross_distinct_identity': dict(attn='cross', train=_ALL_CROSS + ('ident',), ident='other'),
    # parameters
    'cross_bias_only': dict(attn='cross', train=_ALL_CROSS, ident='x', params='bias'),
    'cross_weight_only': dict(attn='cross', train=_ALL_CROSS, ident='x', params='weight'),
    'cross_params_frozen': dict(attn='cross', train=_ALL_CROSS, ident='x', params='none'),
    # positional inputs together with a mask
    'fused_dino_mask': dict(attn='self_fused', train=('x', 'qp'), ident='x', mask='dino190', Lq=190),
    'cross_region_mask': dict(attn='cross', train=_ALL_CROSS, ident='x', mask='mha_region_img'),
}
_HEAD_DIM_ROUTES = {
    'hd64_self': dict(attn='self_fused', train=('x', 'qp'), ident='x', H=4),
    'hd64_cross': dict(attn='cross', train=_ALL_CROSS, ident='x', H=4),
    'hd16_cross_head_mask': dict(attn='cross', train=_ALL_CROSS, ident='x', H=16, mask='mha_region_head16'),
}


@functools.lru_cache(maxsize=None)
def _mha_route_reference(route):
    """Inputs of a route on the CPU and torch.nn.MultiheadAttention in fp64 on them, positional adds written out (computed once
    per route, shared by the attention paths)."""
    cfg = {**_ROUTES, **_HEAD_DIM_ROUTES}[route]
    C, B, H = 256, 2, cfg.get('H', 8)
    Lq = cfg.get('Lq', 70)
    attn, ident, sep_vx = cfg['attn'], cfg['ident'], cfg.get('vx', False)
    cross = attn == 'cross'
    Lk = 96 if cross else Lq
    g = torch.Generator().manual_seed(23)
    ref = torch.nn.MultiheadAttention(C, H, 0.0).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=g).double() * 0.1)
    cpu = dict(x=torch.randn(B, Lq, C, generator=g), qp=torch.randn(B, Lq, C, generator=g))
    if attn != 'self_fused':
        cpu['kp'] = torch.randn(B, Lk, C, generator=g)
    if cross:
        cpu['kx'] = torch.randn(B, Lk, C, generator=g)
        if sep_vx:
            cpu['vx'] = torch.randn(B, Lk, C, generator=g)
    if ident == 'other':
        cpu['ident'] = torch.randn(B, Lq, C, generator=g)
    gy = torch.randn(B, Lq, C, generator=g)
    mask = tmask = None
    if cfg.get('mask'):
        build, mLq, mLk = amc.MHA_MASKS[cfg['mask']]
        mask = build()
        assert (mLq, mLk) == (Lq, Lk)
        per_image = mask.dim() == 3 and mask.shape[0] == B
        assert mask.dim() == 2 or per_image or mask.shape[0] == B * H
        tmask = mask[:, None].expand(-1, H, -1, -1).reshape(B * H, Lq, Lk) if per_image else mask
    r = {n: t.double().clone().requires_grad_(True) for n, t in cpu.items()}
    qq = r['x'] + r['qp']
    if attn == 'self_fused':
        kk, vv = qq, r['x']
    elif attn == 'self_split':
        kk, vv = r['x'] + r['kp'], r['x']
    else:
        kk, vv = r['kx'] + r['kp'], r['vx'] if sep_vx else r['kx']
    out_ref = ref(qq.transpose(0, 1), kk.transpose(0, 1), vv.transpose(0, 1), attn_mask=tmask)[0].transpose(0, 1)
    if ident is not None:
        out_ref = out_ref + (r['x'] if ident == 'x' else r['ident'])
    out_ref.backward(gy.double())
    return cfg, cpu, gy, mask, ref, r, out_ref.detach()


def _mha_route(cuda, route, sums=False):
    """One configuration of ops.mha against its fp64 reference: the output and the gradient of everything trainable at 1e-4,
    `.grad is None` for everything frozen.  -> the product's output and gradients (for bit comparisons between two runs)."""
    from rscotr_amd import ops
    cfg, cpu, gy, mask, ref, r, out_ref = _mha_route_reference(route)
    H = cfg.get('H', 8)
    attn, train, ident, sep_vx, params = cfg['attn'], set(cfg['train']), cfg['ident'], cfg.get('vx', False), cfg.get('params', 'all')
    cross = attn == 'cross'
    assert train <= set(cpu), train - set(cpu)
    # product
    d = {n: t.to(cuda).requires_grad_(n in train) for n, t in cpu.items()}
    want = {'in_proj_weight': params in ('all', 'weight'), 'out_proj.weight': params in ('all', 'weight'),
            'in_proj_bias': params in ('all', 'bias'), 'out_proj.bias': params in ('all', 'bias')}
    P = {n: p.detach().float().to(cuda).requires_grad_(want[n]) for n, p in ref.named_parameters()}
    w = (P['in_proj_weight'], P['in_proj_bias'], P['out_proj.weight'], P['out_proj.bias'])
    idt = None if ident is None else (d['x'] if ident == 'x' else d['ident'])
    kw = dict(identity=idt, q_pos=d['qp'], mask_mode=None)
    if sums:
        kw['q_sum'] = (d['x'] + d['qp']).detach()
        if cross:
            kw['k_sum'] = (d['kx'] + d['kp']).detach()
    md = None if mask is None else mask.to(cuda)
    if attn == 'self_fused':
        out = ops.mha(d['x'], d['x'], d['x'], *w, H, md, k_pos=d['qp'], **kw)
    elif attn == 'self_split':
        out = ops.mha(d['x'], d['x'], d['x'], *w, H, md, k_pos=d['kp'], **kw)
    else:
        out = ops.mha(d['x'], d['kx'], d['vx'] if sep_vx else d['kx'], *w, H, md, k_pos=d['kp'], **kw)
    out.backward(gy.to(cuda))
    torch.cuda.synchronize()
    got = {'out': out.detach()}
    for n in cpu:
        if n in train:
            assert d[n].grad is not None, n
            got[n] = d[n].grad
        else:
            assert d[n].grad is None, n
    for n, p in ref.named_parameters():
        if want[n]:
            assert P[n].grad is not None, n
            got[n] = P[n].grad
        else:
            assert P[n].grad is None, n
    refs = {'out': out_ref, **{n: t.grad for n, t in r.items()}, **{n: p.grad for n, p in ref.named_parameters()}}
    err = {n: _rel(t, refs[n]) for n, t in got.items()}
    print(f'[mha_route] {route} core={ops.STATE.attn_core and 256 // H == 32} sums={sums}: worst {max(err, key=err.get)} {max(err.values()):.3g}')
    for n, e in err.items():
        assert e < 1e-4, (n, e)
    return got


@pytest.mark.parametrize('route', sorted(_ROUTES))
@pytest.mark.parametrize('core', [True, False])
def test_mha_gradient_routing(cuda, route, core):
    """_MHA.backward's branches on needs_input_grad / fused / v_is_kx / id_is_x / has_*pos that the decoders use and
    test_mha_positional_inputs_and_merged_gradients does not reach (the routing is the same Python for both attention paths:
    each sees every route once)."""
    from rscotr_amd import ops
    with ops.STATE.override(attn_core=core):
        _mha_route(cuda, route)


@pytest.mark.parametrize('route', ['fused_dino_mask', 'cross_region_mask', 'split_all'])
@pytest.mark.parametrize('core', [True, False])
def test_mha_precomputed_sums_are_bit_identical(cuda, route, core):
    """q_sum / k_sum = x + q_pos / kx + k_pos formed by the caller: plain data, the same output and gradients to the bit."""
    from rscotr_amd import ops
    with ops.STATE.override(attn_core=core):
        plain = _mha_route(cuda, route)
        summed = _mha_route(cuda, route, sums=True)
    assert plain.keys() == summed.keys()
    for n in plain:
        assert torch.equal(plain[n], summed[n]), n


@pytest.mark.parametrize('route', sorted(_HEAD_DIM_ROUTES))
def test_mha_other_head_dims_take_the_fallback(cuda, route):
    """C = 256 with 4 or 16 heads (head dim 64 / 16) with the fused core left switched on: _MHA routes to the masked-softmax
    path by itself, with correct results."""
    from rscotr_amd import ops
    assert ops.STATE.attn_core is True
    _mha_route(cuda, route)


def test_mask_logits_matches_einsum(cuda):
    """einsum('bqd,bdhw->bqhw') of the seg head on the batched MFMA GEMM (token layout), with both gradients."""
    from rscotr_amd import ops
    g = torch.Generator().manual_seed(6)
    B, Q, D, P = 2, 100, 256, 4096
    e, mf, go = torch.randn(B, Q, D, generator=g), torch.randn(B, P, D, generator=g), torch.randn(B, Q, P, generator=g)
    er, mr = e.double().requires_grad_(True), mf.double().requires_grad_(True)
    ref = torch.einsum('bqd,bpd->bqp', er, mr)
    (ref * go.double()).sum().backward()
    ed, md = e.to(cuda).requires_grad_(True), mf.to(cuda).requires_grad_(True)
    out = ops.mask_logits(ed, md)
    (out * go.to(cuda)).sum().backward()
    assert _rel(out, ref) < 1e-5 and _rel(ed.grad, er.grad) < 1e-5 and _rel(md.grad, mr.grad) < 1e-5
