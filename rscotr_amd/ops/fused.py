"""The fused-launch gates and callers of the Linear / MLP node (ops.matmul._MLP): the ReLU gate as bits (`RELU_BITS`), a two-layer block
as one launch per direction (`FFN_FUSED`) and one tall, narrow Linear on the same machinery (`LIN_FUSED`)."""
import torch

from .core import ACT_GELU, ACT_RELU, _ptr, _stream, lib
from .planes import FPLANES
from .ranges import RANGES
from .state import STATE


class _ReluBits:
    """The ReLU gate of a wide FFN as one bit per element (include/rscotr.h, rscotr_gemm_relu_bits_ok): where BOTH the forward
    product h = relu(x W1^T + b) and the gated backward product dH = (g W2) * [h > 0] run on the interior 128 x 128
    split-product tiles, the forward leaves M * N / 8 bytes of gate words and the backward reads those instead of h."""

    def __init__(self):
        self.enabled = True
        self.cache = {}

    def ok(self, M, N, K, N_next):
        if not self.enabled or not RANGES.enabled:
            return False
        key = (M, N, K, N_next, lib.rscotr_gemm_get_precision())
        r = self.cache.get(key)
        if r is None:
            r = self.cache[key] = bool(lib.rscotr_gemm_relu_bits_ok(M, N, K, K, K, 0, 0)
                                       and lib.rscotr_gemm_relu_bits_ok(M, N, N_next, N_next, N, 0, 1))
        return r


RELU_BITS = _ReluBits()


class _FusedFFN:
    """A two-layer MLP block as ONE launch per direction (rscotr_ffn_h3, csrc/ffn.hip): the encoder FFN (Linear - ReLU - Linear,
    256 -> H -> 256) and the MLP of the Swin blocks of stages 1 and 2 (Linear - GELU - Linear with DropPath, C = 96 / 192):
    forward y = act(x W1^T + b1) W2^T + b2 [* out_scale] (+ identity) with the hidden tensor leaving the kernel for the weight
    gradients only; backward dH = (g W2) * act', dX = dH W1 (+ g) with the mirrored call.  Taken where both weights are
    parameters of the optimizer's arena (their planes and range words live there) and the value ranges are on."""

    MIN_ROWS = 1024
    MODE = {(ACT_RELU, 0): 0, (ACT_RELU, 1): 1, (ACT_GELU, 0): 2, (ACT_GELU, 1): 3}

    def __init__(self):
        self.enabled = True
        self.ln = True  # (the norm in front of a Swin MLP as the launch's prologue)
        self.calls = 0
        self.ln_calls = 0

    def ok(self, x2, ws, act, out_scale, sum_with):
        if not self.enabled or not RANGES.enabled or len(ws) != 2 or act not in (ACT_RELU, ACT_GELU) or sum_with is not None:
            return False
        sink = STATE.grad_sink
        (H, C), (C2, H2) = ws[0].shape, ws[1].shape
        M = x2.shape[0]
        if sink is None or STATE.profile is not None or C2 != C or H2 != H or M < self.MIN_ROWS or x2.data_ptr() % 16:
            return False
        if not (sink.is_param_ptr(ws[0].data_ptr()) and sink.is_param_ptr(ws[1].data_ptr())):
            return False
        return bool(lib.rscotr_ffn_h3_ok(M, C, H))

    def ln_ok(self, lz, C, act):
        """Can the forward launch take the LayerNorm in front of the block (a pending ops.norm.LazyNorm) as its prologue?"""
        sink = STATE.grad_sink
        return (self.ln and act == ACT_GELU and C in (96, 192, 384) and lz.w is not None and sink is not None
                and sink.is_param_ptr(lz.w.data_ptr()) and (lz.b is None or sink.is_param_ptr(lz.b.data_ptr())))

    def run(self, x2, W1, b1, W2, b2, act, aux, gate, resid, want_y_range, xscale=None, yscale=None, rows_per=0, ln=None):
        """gate = 0: (W1, W2) are the two Linear weights as stored, (out, in); gate = 1: the mirrored products, W1 := W2 and
        W2 := W1 of the forward, both taken transposed.  aux: the gate bits (ReLU) or the pre-activation (GELU), written by the
        forward call and read by the mirrored one.  ln: a pending LazyNorm whose output x2 is — the launch normalises ln.x2's rows
        itself and fills x2 and the norm's statistics (rscotr_ffn_h3_ln).  -> (hid, y)."""
        M, C = x2.shape
        H = W1.shape[1] if gate else W1.shape[0]
        dev = x2.device
        sink = STATE.grad_sink
        s_x = 0 if ln is not None else RANGES.of(x2, M, C, C)
        s_w1, s_w2 = RANGES.of(W1, W1.shape[0], W1.shape[1], W1.shape[1]), RANGES.of(W2, W2.shape[0], W2.shape[1], W2.shape[1])
        s_b1 = sink.amax_slot(b1.data_ptr()) if (b1 is not None and sink.is_param_ptr(b1.data_ptr())) else 0
        if b1 is not None and not s_b1:
            s_b1 = RANGES.of(b1.view(1, -1), 1, H, H)
        w1f, w2f = FPLANES.get(W1, gate, s_w1), FPLANES.get(W2, gate, s_w2)
        hid = torch.empty((M, H), dtype=torch.float32, device=dev)
        y = torch.empty((M, C), dtype=torch.float32, device=dev)
        s_h = RANGES.new_slot(dev)
        RANGES.tag(hid, s_h)
        s_y = 0
        if want_y_range:
            s_y = RANGES.new_slot(dev)
            RANGES.tag(y, s_y)
        relu = act == ACT_RELU
        splits = int(lib.rscotr_ffn_h3_splits(M, C, H))  # (few rows: partial sums over runs of the hidden width, combined by a second launch)
        ws = torch.empty(splits * M * C, dtype=torch.float32, device=dev) if splits > 1 else None
        if ln is not None:
            assert not gate and not relu and xscale is None and ln.y.data_ptr() == x2.data_ptr()
            lib.call('rscotr_ffn_h3_ln', ln.x2.data_ptr(), M, C, H, _ptr(ln.w), _ptr(ln.b), float(ln.eps), x2.data_ptr(),
                     ln.stats[0].data_ptr(), ln.stats[1].data_ptr(), w1f, _ptr(b1), w2f, _ptr(b2), aux.data_ptr(), hid.data_ptr(),
                     _ptr(resid), y.data_ptr(), _ptr(yscale), int(rows_per), sink.amax_slot(ln.w.data_ptr()),
                     0 if ln.b is None else sink.amax_slot(ln.b.data_ptr()), s_w1, s_w2, s_b1, ln.slot, s_h, s_y, _ptr(ws),
                     0 if ws is None else ws.numel() * 4, _stream())
            ln.done = True
            self.calls += 1
            self.ln_calls += 1
            return hid, y
        lib.call('rscotr_ffn_h3', x2.data_ptr(), M, C, H, w1f, _ptr(b1), w2f, _ptr(b2), self.MODE[(act, int(gate))],
                 aux.data_ptr() if relu else 0, 0 if relu else aux.data_ptr(), hid.data_ptr(), _ptr(resid), y.data_ptr(),
                 _ptr(xscale), _ptr(yscale), int(rows_per), s_x, s_w1, s_w2, s_b1, s_h, s_y, _ptr(ws),
                 0 if ws is None else ws.numel() * 4, _stream())
        self.calls += 1
        return hid, y


FFN_FUSED = _FusedFFN()


class _FusedLinear:
    """ONE Linear on the fused MLP kernel's machinery (rscotr_lin_h3, csrc/ffn.hip: the rows' planes staged once per workgroup, the
    weight as fragment-major planes) for the TALL, NARROW products — Swin stages 1 / 2: the qkv / proj Linears of the window attention,
    PatchMerging's reduction, and their input gradients: 32768 x 96 -> 288 and the like, 25-50 MB for ~1 GFLOP, where the tiled
    kernels re-stage the rows once per column tile.  Taken where the weight is a parameter of the optimizer's arena and the value
    ranges are on; the 256-wide 10880-row Linears of the encoder stay on the tiled kernel (measured: profiles/r6_ffn_lab.txt)."""

    MIN_ROWS = 8192
    MAX_NARROW = 192  # the smaller of (N, K) at most this
    FEW_K = (384, 768)

    def __init__(self):
        self.enabled = True
        self.calls = 0
        self.ln_calls = 0

    def ok(self, x2, W, N, K):
        M = x2.shape[0]
        sink = STATE.grad_sink
        if not self.enabled or not RANGES.enabled or sink is None or STATE.profile is not None or x2.data_ptr() % 16 or not W.is_contiguous():
            return False
        tall = M >= self.MIN_ROWS and min(N, K) <= self.MAX_NARROW and max(N, K) <= 576
        # FEW rows with a wide reduction (Swin stages 3 / 4: 2048 x 384 -> 1152 / 384, 512 x 768 -> 2304 / 768, the neck's 1x1
        # convolutions on them): one workgroup per (row tile, 256 columns), all of K staged once — 11 us against 17-27 for the tiled
        # kernels (fp32 pipe at 96-192 workgroups).  The decoders' K = 256 products stay where they are (measured: +1.35 ms per round)
        few = 512 <= M < self.MIN_ROWS and K in self.FEW_K and N <= 3 * K
        if not (tall or few):
            return False
        return sink.is_param_ptr(W.data_ptr()) and bool(lib.rscotr_lin_h3_ok(M, N, K))

    def ln_ok(self, lz, K):
        sink = STATE.grad_sink
        return (K in (96, 192, 384) and lz.w is not None and sink is not None and sink.is_param_ptr(lz.w.data_ptr())
                and (lz.b is None or sink.is_param_ptr(lz.b.data_ptr())))

    def run(self, x2, W, bias, tr, resid, want_y_range, xscale=None, yscale=None, rows_per=0, ln=None):
        """tr = 0: y = x W^T (W (N, K) as stored); tr = 1: y = x W (W (K, N): the input gradient of the Linear).  ln: a pending LazyNorm whose
        output x2 is (rscotr_lin_h3_ln).  -> y (M, N)."""
        M, K = x2.shape
        N = W.shape[1] if tr else W.shape[0]
        dev = x2.device
        sink = STATE.grad_sink
        s_x = 0 if ln is not None else RANGES.of(x2, M, K, K)
        s_w = RANGES.of(W, W.shape[0], W.shape[1], W.shape[1])
        wf = FPLANES.get(W, tr, s_w)
        y = torch.empty((M, N), dtype=torch.float32, device=dev)
        s_y = 0
        if want_y_range:
            s_y = RANGES.new_slot(dev)
            RANGES.tag(y, s_y)
        if ln is not None:
            assert xscale is None and ln.y.data_ptr() == x2.data_ptr()
            lib.call('rscotr_lin_h3_ln', ln.x2.data_ptr(), M, N, K, _ptr(ln.w), _ptr(ln.b), float(ln.eps), x2.data_ptr(),
                     ln.stats[0].data_ptr(), ln.stats[1].data_ptr(), wf, _ptr(bias), _ptr(resid), y.data_ptr(), _ptr(yscale),
                     int(rows_per), sink.amax_slot(ln.w.data_ptr()), 0 if ln.b is None else sink.amax_slot(ln.b.data_ptr()), s_w,
                     ln.slot, s_y, _stream())
            ln.done = True
            self.ln_calls += 1
        else:
            lib.call('rscotr_lin_h3', x2.data_ptr(), M, N, K, wf, _ptr(bias), _ptr(resid), y.data_ptr(), _ptr(xscale), _ptr(yscale),
                     int(rows_per), s_x, s_w, s_y, _stream())
        self.calls += 1
        return y


LIN_FUSED = _FusedLinear()
