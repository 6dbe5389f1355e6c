"""Matrix products of the step on the C ABI: `gemm` (rscotr_gemm_f32 and its split-product / weight-plane routes), `colsum`,
`gemm_batched` (attention products addressed in place), and the Linear / MLP autograd node built on them (`linear`, `mlp`,
`_linear_param_grad`).  The weight planes live in ops.planes, the deferred weight-gradient work in ops.deferred, the fused launches
in ops.fused."""
import torch
from torch.autograd import Function

from .core import (ACT_GELU, ACT_GELU_GRAD, ACT_NONE, ACT_RELU, ACT_RELU_BITS, ACT_RELU_GRAD, ACT_RELU_GRAD_BITS, _ACT, _WS, _Prof,
                   _chk, _f32c, _gemm_ws_bytes, _off_path, _ptr, _sink, _stream, lib)
from .deferred import _in_arena, _try_defer_dw
from .fused import FFN_FUSED, LIN_FUSED, RELU_BITS
from .planes import HPLANES, WPLANES
from .ranges import RANGES
from .state import STATE


def gemm(A, B, M, N, K, lda, ldb, a_kmajor, b_kmajor, out=None, bias=None, act=ACT_NONE, aux=None, pre=None,
         resid=None, accumulate=False, rowsum=None, rowsum_accumulate=False, rowscale=None, rows_per=0, kscale=None,
         krows_per=0, out2=None, amax_a=0, amax_b=0, amax_out=0, range_out=True):
    """C[m,n] = epilogue(sum_k Aop[m,k] Bop[n,k]) on the fp32 matrix cores (include/rscotr.h,
    rscotr_gemm_f32).  A, B, out are contiguous fp32 device tensors; out (M,N) is allocated here
    unless given.  `rowsum` (M,) (+)= sum_k Aop[m,k] (k-major A only: the bias gradient riding the dW
    contraction).  `out2` (M,N): second output out + resid, `out` itself then stays without the residual.
    Returns out."""
    _chk(A, B, out, bias, aux, pre, resid, rowsum, out2)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    elif not amax_out:
        # a caller's tensor is (re)written: whatever bound it carried no longer holds; a route below that commits a word tags it anew
        RANGES.untag(out)
    if not amax_out:
        RANGES.untag(out2)
    if (rowsum is None and kscale is None and STATE.profile is None
            and WPLANES.eligible(A, B, M, N, K, lda, ldb, a_kmajor, b_kmajor,
                                 gelu=act in (ACT_GELU, ACT_GELU_GRAD) or pre is not None)):
        # B is a parameter: multiply with its pre-split bf16 planes (written once per optimizer step)
        planes, npad = WPLANES.get(B, N, K, ldb, b_kmajor)
        nws = lib.rscotr_gemm_f32_wplanes_workspace(M, N, K)
        ws = _WS.get(nws, A.device).data_ptr() if nws else 0
        lib.call('rscotr_gemm_f32_wplanes', A.data_ptr(), planes, npad, out.data_ptr(), M, N, K, lda, N, _ptr(bias), int(act),
                 _ptr(aux), _ptr(pre), _ptr(resid), int(accumulate), _ptr(rowscale), int(rows_per), _ptr(out2), ws, nws,
                 _stream())
        return out
    key = (M, N, K, lib.rscotr_gemm_get_precision())  # the workspace a shape wants depends on the precision mode
    nws = _gemm_ws_bytes.get(key)
    if nws is None:
        nws = _gemm_ws_bytes[key] = lib.rscotr_gemm_f32_workspace(M, N, K)
    if (accumulate and a_kmajor and b_kmajor and bias is None and act == ACT_NONE and resid is None and pre is None
            and rowscale is None and (rowsum is None or rowsum_accumulate) and STATE.profile is None
            and _try_defer_dw(A, B, out, M, N, K, lda, ldb, rowsum, kscale, krows_per, nws)):
        return out
    ws = _WS.get(nws, A.device).data_ptr() if nws else 0
    if RANGES.enabled:
        if not (amax_a and amax_b) and RANGES.wanted(M, N, K, lda, ldb, a_kmajor, b_kmajor, act, pre is not None,
                                                     rowscale is not None, kscale is not None, nws):
            # the split kernels take this product: with the value ranges of both operands it runs as the fp16 split product
            amax_a = amax_a or (RANGES.of(A, K, M, lda) if a_kmajor else RANGES.of(A, M, K, lda))
            amax_b = amax_b or (RANGES.of(B, K, N, ldb) if b_kmajor else RANGES.of(B, N, K, ldb))
        if not amax_out and range_out and RANGE_OUT.enabled_for(out):
            # the range of what this product stores rides out of its epilogue: whoever multiplies with it next finds it
            amax_out = RANGES.new_slot(A.device)
            RANGES.tag(out, amax_out)
            if out2 is not None:
                RANGES.tag(out2, amax_out)
    args = (A.data_ptr(), B.data_ptr(), out.data_ptr(), M, N, K, lda, ldb, N, int(a_kmajor), int(b_kmajor),
            _ptr(bias), int(act), _ptr(aux), _ptr(pre), _ptr(resid), int(accumulate), _ptr(rowsum),
            int(rowsum_accumulate), _ptr(rowscale), int(rows_per), _ptr(kscale), int(krows_per), _ptr(out2), ws, nws,
            int(amax_a), int(amax_b), int(amax_out), _stream())
    entry = 'rscotr_gemm_f32_r'
    if (amax_a and amax_b and rowsum is None
            and HPLANES.eligible(B, M, N, K, lda, ldb, a_kmajor, b_kmajor, act, pre, rowscale, kscale, nws)):
        # B is a parameter and the interior pipelined 64 x 64 kernel takes the product: its pre-split fp16 planes ride along
        planes, rpad = HPLANES.get(B, N, K, ldb, b_kmajor, amax_b)
        args = args[:-1] + (planes, rpad, args[-1])
        entry = 'rscotr_gemm_f32_rb'
    if STATE.profile is None:
        lib.call(entry, *args)
    else:
        with _Prof('gemm', 2 * M * N * K, gemm_kernel_name(M, N, K, a_kmajor, b_kmajor),
                   shape=(M, N, K, int(a_kmajor), int(b_kmajor))):
            lib.call(entry, *args)
    return out


def gemm_kernel_name(M, N, K, a_kmajor, b_kmajor):
    """Name of the kernel instantiation rscotr_gemm_f32 launches for this problem (mirrors the tile
    choice in csrc/gemm.hip; used to label roofline samples so they can be matched with rocprof)."""
    if N <= 32:
        bm, bn, wm, wn = 128, 32, 4, 1
    elif N >= 1024 and M >= 4096 and M % 128 == 0:
        bm, bn, wm, wn = 128, 64, 2, 2
    else:
        bm, bn, wm, wn = 64, 64, 2, 2
    return f'rscotr::gemm_f32_kernel<{bm}, {bn}, {wm}, {wn}, {"true" if a_kmajor else "false"}, ' \
           f'{"true" if b_kmajor else "false"}, *>'


def colsum(X, M, N, out=None, accumulate=False):
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=X.device)
    nws = lib.rscotr_colsum_f32_workspace(M, N)
    ws = _WS.get(nws, X.device)
    lib.call('rscotr_colsum_f32', X.data_ptr(), out.data_ptr(), M, N, N, int(accumulate), ws.data_ptr(), nws,
             _stream())
    return out


class _RangeOut:
    """Which products leave the range word of their output (amax_out of rscotr_gemm_f32_r).  The commit is one atomic round trip at
    the end of every workgroup's life (~1 us per launch: profiles/r5_range_word_cost.txt), and only an output that a LATER product
    multiplies with needs the word: callers that know their consumer is a norm, an attention core, the sampling kernel or an
    element-wise merge pass `range_out=False` (ops.linear / ops.gemm).  A tensor that does reach a product without a word is
    measured there (rscotr_amax_f32: correct, one launch; RSCOTR_RANGES_STATS=1 lists them).  `all = True`: every product
    writes its word, as before."""

    def __init__(self):
        self.all = False
        self.skip_next = False  # set by ops.linear(range_out=False) for the forward of the node it creates

    def enabled_for(self, out):
        return not _in_arena(out)

    def want(self, flag):
        return True if self.all else bool(flag)


RANGE_OUT = _RangeOut()

def _attn_ksplits(M, N, K, nb):
    """Slices of the key axis for an attention product with few output tiles (P v, dS k): aim at >= 512
    workgroups, >= 128 keys per slice, K divisible."""
    tiles = ((M + 127) // 128) * nb if N <= 32 else ((M + 63) // 64) * ((N + 63) // 64) * nb
    sp = 1
    while tiles * sp < 512 and K % (sp * 2) == 0 and K // (sp * 2) >= 128 and (K // (sp * 2)) % 16 == 0:
        sp *= 2
    return sp


def gemm_batched(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, nb0, nb1, sA, sB, sC, offA=0, offB=0, offC=0,
                 accumulate=False, ksplit=False):
    """nb0*nb1 products of one shape addressed in place (rscotr_gemm_f32_batched); s? = (stride b0, stride b1)
    and off? = element offset of the first problem inside the tensor."""
    _chk(A, B, C)
    flops = 2 * M * N * K * nb0 * nb1
    sp = _attn_ksplits(M, N, K, nb0 * nb1) if (ksplit and not a_kmajor and b_kmajor and not accumulate and offC == 0) else 1
    ws = _WS.get(sp * C.numel() * 4, C.device).data_ptr() if sp > 1 else 0
    args = (A.data_ptr() + 4 * offA, B.data_ptr() + 4 * offB, C.data_ptr() + 4 * offC, M, N, K, lda, ldb, ldc,
            int(a_kmajor), int(b_kmajor), nb0, nb1, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], int(accumulate), sp, ws,
            C.numel(), _stream())
    if STATE.profile is None:
        lib.call('rscotr_gemm_f32_batched', *args)
    else:
        with _Prof('gemm_batched', flops, 'rscotr::gemm_f32_kernel (batched attention products)'):
            lib.call('rscotr_gemm_f32_batched', *args)
    return C


def _linear_param_grad(A, Bm, M, N, K, w_handle, b_handle, row0, want_w, want_b, lda=None, kscale=None, krows_per=0):
    """Parameter gradients of y = x W^T + b from A = dy (K rows, M columns as the k-major operand) and Bm = x:
    dW[row0:row0+M] (+)= A^T Bm, db[row0:row0+M] (+)= column sums of A (riding the dW contraction); straight into the
    gradient arena when the parameter is sunk (then nothing is returned for it).  `lda`: row stride of A when it is a column
    block of a wider tensor.  `kscale`: per-sample factor on the rows of A (runs of `krows_per` rows), folded into the contraction.
    Returns (gw, gb, sink_w, sink_b); the caller announces the sunk gradients (`grad_sink.grad_written`)."""
    dev = A.device
    skw = _sink(w_handle) if want_w else None
    skb = _sink(b_handle) if want_b else None
    gw = gb = None
    rs, rs_acc = None, False
    if want_b:
        if skb is not None:
            rs, rs_acc = skb[1][row0:row0 + M], True
        else:
            rs = gb = torch.empty(M, dtype=torch.float32, device=dev)
    if want_w:
        dw = lambda **out: gemm(A, Bm, M, N, K, lda or M, N, 1, 1, rowsum=rs, rowsum_accumulate=rs_acc, kscale=kscale,
                                krows_per=krows_per if kscale is not None else 0, **out)
        if skw is None:
            gw = dw()
        elif skb is not None or not want_b:  # everything lands in the arena: off the critical path
            _off_path(lambda: dw(out=skw[1][row0:row0 + M], accumulate=True), A, Bm, kscale)
        else:
            dw(out=skw[1][row0:row0 + M], accumulate=True)
    elif want_b:
        assert lda is None or lda == M
        if kscale is not None:
            raise RuntimeError('out_scale with a bias-only gradient is not supported')
        colsum(A, K, M, out=rs, accumulate=rs_acc)
    return gw, gb, skw, skb


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


class _MLP(Function):
    """y = L_n(act(L_{n-1}(... act(L_1(x))))) [+ identity], L_i(h) = h W_i^T + b_i: every Linear is
    one MFMA GEMM with bias/activation/residual fused in its epilogue; backward folds act' into the
    epilogue of the dX GEMM of the following layer (no separate element-wise passes).
    `out_scale` (B,) or None: per-sample factor on the last layer's output before the identity is added (the
    DropPath of a Swin block folded into its proj / fc2 Linear): forward rides the epilogue, backward the
    epilogue of dH and the operand staging of dW / db.
    `sum_with` (same shape as the output) or None: a second, non-differentiable output `y + sum_with` leaves the last
    epilogue (the `query + query_pos` of the attention that follows a positional MLP: ops.mha / ops.msda_attention take it as
    `q_sum`); only without identity / out_scale.
    args: x, identity (Tensor | None), act code, out_scale, sum_with, then W_1, b_1, ..., W_n, b_n (b may be None)."""

    @staticmethod
    def forward(ctx, x, identity, act, out_scale, sum_with, *wb):
        n = len(wb) // 2
        ws, bs = wb[0::2], wb[1::2]
        K0 = x.shape[-1]
        x2 = RANGES.carry(x, _f32c(x).reshape(-1, K0))
        M = x2.shape[0]
        id_is_x = identity is x  # mmcv FFN: identity defaults to the input itself
        rows_per = 0
        if out_scale is not None:
            out_scale = _f32c(out_scale)
            assert x.dim() == 3 and out_scale.numel() == x.shape[0]
            rows_per = x.shape[1]
        id2 = None if identity is None else (x2 if id_is_x else _f32c(identity).reshape(M, -1))
        s2 = y2 = None
        if sum_with is not None:
            assert identity is None and out_scale is None
            s2 = _f32c(sum_with).reshape(M, -1)
        hs, auxs = [x2], []
        h = x2
        # the last layer's range word: not for an output that takes a residual (a block output: the next reader is a norm) nor
        # where the caller said so (ops.linear(range_out=False): qkv of a window attention, ...)
        want_last = RANGE_OUT.want(not RANGE_OUT.skip_next and id2 is None)
        RANGE_OUT.skip_next = False
        ctx.fused = FFN_FUSED.ok(x2, ws, act, out_scale, sum_with)
        lz = getattr(x, '_lazy_ln', None)  # (the norm in front has not run yet: ops.layer_norm_fork(lazy=True))
        # ONE Linear, tall and narrow (ops.LIN_FUSED): the rows-resident launch instead of the tiled product
        ctx.lin = (n == 1 and act == ACT_NONE and sum_with is None and LIN_FUSED.ok(x2, ws[0], ws[0].shape[0], K0))
        if lz is not None and not lz.done and not ((ctx.fused and FFN_FUSED.ln_ok(lz, K0, act)) or (ctx.lin and LIN_FUSED.ln_ok(lz, K0))):
            lz.run()
        if lz is not None and lz.done:
            lz = None
        if ctx.lin:
            h = LIN_FUSED.run(x2, ws[0], bs[0], 0, id2, want_last, yscale=out_scale, rows_per=rows_per, ln=lz)
            n = 0
        if ctx.fused:
            W1 = _contig(ws[0])
            W2 = _contig(ws[1])
            if act == ACT_RELU:  # the gate as one bit per element
                aux = torch.empty(int(lib.rscotr_ffn_h3_bits_words(M, K0, W1.shape[0])), dtype=torch.int32, device=x2.device)
            else:  # GELU: the pre-activation
                aux = torch.empty((M, W1.shape[0]), dtype=torch.float32, device=x2.device)
            hid, h = FFN_FUSED.run(x2, W1, bs[0], W2, bs[1], act, aux, 0, id2, want_last, yscale=out_scale, rows_per=rows_per, ln=lz)
            hs.append(hid)
            auxs.append(aux)
            n = 0  # (the loop below has nothing left to do)
        for i in range(n):
            W = _contig(ws[i])
            N, K = W.shape
            last = i == n - 1
            pre, a_i = None, act
            if not last and act == ACT_GELU:
                pre = torch.empty((M, N), dtype=torch.float32, device=x2.device)
            elif not last and act == ACT_RELU and RELU_BITS.ok(M, N, K, ws[i + 1].shape[0]):
                # the gate leaves the forward epilogue as bits: the gated dH product of backward reads 1 / 32 of the bytes
                pre, a_i = torch.empty(M * N // 64, dtype=torch.int64, device=x2.device), ACT_RELU_BITS
            sc = out_scale if last else None
            if last and s2 is not None:  # out2 = y + sum_with, y itself stored without it (epilogue's second output)
                y2 = torch.empty((M, N), dtype=torch.float32, device=x2.device)
                h = gemm(h, W, M, N, K, K, K, 0, 0, bias=bs[i], act=ACT_NONE, resid=s2, out2=y2)
            else:
                h = gemm(h, W, M, N, K, K, K, 0, 0, bias=bs[i], act=ACT_NONE if last else a_i, pre=pre,
                         resid=id2 if last else None, rowscale=sc, rows_per=rows_per if sc is not None else 0,
                         range_out=want_last if last else True)
            if not last:
                hs.append(h)
                auxs.append(pre if pre is not None else h)  # (GELU: the pre-activation; ReLU: the gate bits, or h itself)
        n = len(ws)
        ctx.save_for_backward(*hs, *auxs, *ws)
        ctx.h_slots = [RANGES.saved(t) for t in hs]  # ((generation, slot) of the saved activations: the weight gradients want their ranges)
        ctx.out_scale, ctx.rows_per = out_scale, rows_per
        ctx.n, ctx.act, ctx.has_id, ctx.id_is_x = n, act, identity is not None, id_is_x
        ctx.has_bias = [b is not None for b in bs]
        ctx.biases = bs  # parameter handles only (for the gradient sink); not needed as saved tensors
        ctx.x_shape = x.shape
        ctx.id_shape = None if identity is None else identity.shape
        out = RANGES.carry(h, h.view(*x.shape[:-1], h.shape[-1]))
        if y2 is None:
            return out
        y2 = RANGES.carry(y2, y2.view(out.shape))
        ctx.mark_non_differentiable(y2)
        ctx.set_materialize_grads(False)
        ctx.two_outputs = True
        return out, y2

    @staticmethod
    def backward(ctx, dy, _dsum=None):
        if dy is None:  # (only the non-differentiable sum was used)
            return (None,) * (5 + 2 * ctx.n)
        n, act = ctx.n, ctx.act
        saved = ctx.saved_tensors
        hs, auxs, ws = saved[:n], saved[n:2 * n - 1], saved[2 * n - 1:]
        M = hs[0].shape[0]
        for t, sl in zip(hs, ctx.h_slots):
            RANGES.restore(t, sl)  # (only within the generation that wrote the word: a begin() since the forward voids it)
        g = RANGES.carry(dy, _f32c(dy).reshape(M, -1))
        g_out = g
        d_id = g.view(ctx.id_shape) if ctx.has_id and not ctx.id_is_x and ctx.needs_input_grad[1] else None
        grads_wb = [None] * (2 * n)
        gact = ACT_RELU_GRAD if act == ACT_RELU else ACT_GELU_GRAD
        dx = None
        def param_grads(i, g):
            """dW_i = g^T h_i and db_i (riding the contraction) into the arena / grads_wb; -> (W_i, scr of the layer)"""
            W = _contig(ws[i])
            N, K = W.shape
            # the last layer's upstream gradient is s_b * dy: folded into the three contractions that read it
            sc = ctx.out_scale if i == n - 1 else None
            scr = dict(rowscale=sc, rows_per=ctx.rows_per) if sc is not None else {}
            grads_wb[2 * i], grads_wb[2 * i + 1], skw, skb = _linear_param_grad(
                g, hs[i], N, K, M, ws[i], ctx.biases[i], 0, ctx.needs_input_grad[5 + 2 * i],
                ctx.has_bias[i] and ctx.needs_input_grad[6 + 2 * i], kscale=sc, krows_per=ctx.rows_per)
            for sk in (skw, skb):
                if sk is not None:
                    STATE.grad_sink.grad_written(sk[0])
            return W, scr

        if getattr(ctx, 'fused', False):
            # the mirrored pair dH = (g W2) * gate, dX = dH W1 (+ dy when the identity is the input) as ONE launch (ops.FFN_FUSED)
            W2, _ = param_grads(1, g)
            W1 = _contig(ws[0])
            # (a DropPath'ed block: the upstream gradient of both products is s_b * dy — the rows are scaled while they are staged)
            dH, dx = FFN_FUSED.run(g, W2, None, W1, None, act, auxs[0], 1, g_out if ctx.id_is_x else None, False,
                                   xscale=ctx.out_scale, rows_per=ctx.rows_per)
            param_grads(0, dH)
            dx = RANGES.carry(dx, dx.view(ctx.x_shape)) if ctx.needs_input_grad[0] else None
            return (dx, d_id, None, None, None, *grads_wb)
        for i in range(n - 1, -1, -1):
            W, scr = param_grads(i, g)
            N, K = W.shape
            if i > 0:
                ga = ACT_RELU_GRAD_BITS if (act == ACT_RELU and auxs[i - 1].dtype == torch.int64) else gact
                g = gemm(g, W, M, K, N, N, K, 0, 1, act=ga, aux=auxs[i - 1], **scr)  # dH = (g W) * act'
            elif ctx.needs_input_grad[0]:
                # identity == input: its gradient (dy) rides in this epilogue instead of a separate add
                # (the node's input gradient goes to a norm's backward, an attention backward or a merge: no later product
                #  multiplies with it directly)
                if n == 1 and getattr(ctx, 'lin', False) and LIN_FUSED.ok(g, W, K, N):
                    dx = LIN_FUSED.run(g, W, None, 1, g_out if ctx.id_is_x else None, RANGE_OUT.want(False),
                                       yscale=scr.get('rowscale'), rows_per=scr.get('rows_per', 0))
                else:
                    dx = gemm(g, W, M, K, N, N, K, 0, 1, resid=g_out if ctx.id_is_x else None, range_out=RANGE_OUT.want(False), **scr)
                dx = RANGES.carry(dx, dx.view(ctx.x_shape))
        return (dx, d_id, None, None, None, *grads_wb)


def mlp(x, layers, act='relu', identity=None, out_scale=None, sum_with=None, range_out=True):
    """layers: [(W, b), ...]; activation between layers, none after the last; `identity` (same shape
    as the output) is added in the last epilogue (mmcv FFN add_identity); `out_scale` (B,) multiplies the
    output per sample before that (DropPath).  With `sum_with` (shape of the output, values only): -> (y, y + sum_with), the
    sum without a gradient of its own."""
    flat = []
    for w, b in layers:
        flat += [w, b]
    RANGE_OUT.skip_next = not range_out  # (False: no later product multiplies with the output — RANGE_OUT)
    try:
        return _MLP.apply(x, identity, _ACT[act], out_scale, None if sum_with is None else sum_with.detach(), *flat)
    finally:
        RANGE_OUT.skip_next = False


def linear(x, w, b=None, act=None, resid=None, out_scale=None, range_out=True):
    """F.linear(x, w, b) [* out_scale per sample] (+ resid) on the matrix cores.  Activations belong to `mlp`.
    range_out=False: no later product multiplies with the output (RANGE_OUT)."""
    if act is not None:
        raise RuntimeError('ops.linear has no activation: use ops.mlp')
    RANGE_OUT.skip_next = not range_out
    try:
        return _MLP.apply(x, resid, ACT_NONE, out_scale, None, w, b)
    finally:
        RANGE_OUT.skip_next = False
