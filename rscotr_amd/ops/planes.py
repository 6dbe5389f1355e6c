"""Pre-split planes of the parameters that serve as the weight operand of a product: `WPLANES` (bf16, the six-term route), `HPLANES`
(fp16, the interior pipelined split kernel) and `FPLANES` (fragment-major fp16, the fused FFN / Linear launches).  One life cycle
(`_PlaneCache`): a split kernel writes a set ONCE per optimizer step, every product until the next step reads it."""
import os

import numpy as np
import torch

from .core import _stream, lib
from .deferred import DEFER
from .ranges import RANGES
from .state import STATE


class _PlaneCache:
    """Plane sets keyed by (address, two extents, row stride, transposed) of the weight operand.  A parameter is recognised by its
    address inside the optimizer's flat arena (`STATE.grad_sink.is_param_ptr`); the sets a task uses are remembered under the
    task's name (`begin`), and the first product of an iteration that finds them stale re-splits ALL of them in one grouped launch
    (inside the per-task hipGraph when the iteration is replayed).  `bump()` = "the parameters have changed" (optimizer step,
    checkpoint load, snapshot restore).  `begin` / `reset` / `bump` act on all three caches, whichever one they are called on.

    A subclass states its `eligible` test and public `get`, the split kernel (`ENTRY`), how an entry is sized (`_size`) and, where it
    differs, the table row of an entry (`_row`)."""

    ENTRY = None

    def __init__(self):
        self.enabled = True
        self.version = 1
        self.entries, self.groups, self.tables = {}, {}, {}
        self.current = None

    def begin(self, group):
        for c in _CACHES:
            c.current = group

    def reset(self):
        """Forget every plane set (a new optimizer arena: addresses may be reused by other parameters)."""
        for c in _CACHES:
            c.entries, c.groups, c.tables = {}, {}, {}
            c.version += 1

    def bump(self, by_optimizer=False):
        """The parameters have changed.  by_optimizer: by the update kernel itself, which also rewrites their range words;
        any other writer (checkpoint / state-dict load, init_weights, a snapshot restore, a manual copy) leaves the words the
        optimizer keeps stale — a stale-small word overflows the fp16 planes — so they are recomputed on next use."""
        for c in _CACHES:
            c.version += 1
        if not by_optimizer and STATE.grad_sink is not None:
            STATE.grad_sink.params_changed()

    def _entry(self, key, device, **fixed):
        """-> the entry of `key`, fresh; `fixed`: what a new entry records besides its planes (the range word of the split)."""
        e = self.entries.get(key)
        if e is None:
            e = self.entries[key] = dict(self._size(key, device), version=0, **fixed)
        keys = self.groups.setdefault(self.current, [])
        if key not in keys:
            keys.append(key)
        if e['version'] != self.version:
            self._refresh(keys, device)
        return e

    def _refresh(self, keys, dev):
        stale = tuple(k for k in keys if self.entries[k]['version'] != self.version)
        hit = self.tables.get(stale)
        if hit is None:
            rows, first = [], 0
            for k in stale:
                rows.append(self._row(k, self.entries[k], first))
                first += self.entries[k]['blocks']
            # (a table first needed while a hipGraph is being captured — a parameter set no warm-up iteration touched — goes through
            #  the pinned staging buffers of the deferred-work tables: a pageable host-to-device copy is not capturable)
            hit = (DEFER._upload(np.asarray(rows, dtype=np.int64), dev), len(rows), first)
            if not (dev.type == 'cuda' and torch.cuda.is_current_stream_capturing()):
                self.tables[stale] = hit  # (a table built inside a capture lives in the graph's private pool: not for later eager calls)
        table, n, blocks = hit
        lib.call(self.ENTRY, table.data_ptr(), n, blocks, _stream())
        for k in stale:
            self.entries[k]['version'] = self.version

    @staticmethod
    def _planes(words, pad, blocks, device):
        return dict(planes=torch.empty(words, dtype=torch.int16, device=device), pad=pad, blocks=blocks)

    def _row(self, key, e, first):
        """{W, planes, rows of W, cols of W, ldw, padded rows, first block, transposed} of an operand B = key (ptr, N, K, ldb, tr): a
        row-major operand B (N, K) is W itself; a k-major one is the (K, N) matrix W whose TRANSPOSE is multiplied (planes of W^T)."""
        ptr, N, K, ldb, tr = key
        return (ptr, e['planes'].data_ptr(), K if tr else N, N if tr else K, ldb, e['pad'], first, tr)


class _WeightPlanes(_PlaneCache):
    """bf16 plane sets of the parameters that serve as the B operand of y = x W^T (and dx = dy W): rscotr_gemm_split_weights
    writes them and rscotr_gemm_f32_wplanes multiplies fp32 activations with them (include/rscotr.h)."""

    ENTRY = 'rscotr_gemm_split_weights'

    def __init__(self):
        super().__init__()
        # (round 5: with the fp16 split product on, the tiled kernels are as fast as the 128-row weight-plane kernel on its own
        # shapes — 10880 x 256 x 2048: 72 us against 70 — and need no plane sets: the route is only taken with RSCOTR_GEMM_H3=0)
        self.enabled = os.environ.get('RSCOTR_WPLANES', '1') != '0' and not RANGES.enabled
        self.shape_ok = {}

    def eligible(self, A, B, M, N, K, lda, ldb, a_kmajor, b_kmajor, gelu=False):
        if not self.enabled or a_kmajor or STATE.grad_sink is None or K % 16 or N < 64:
            return False
        if lda % 4 or A.data_ptr() % 16 or (b_kmajor and ldb % 4):
            return False
        if lib.rscotr_gemm_get_precision() != 3:
            return False
        # the shape: the 128-row weight-plane kernel's domain (the library decides: rscotr_gemm_f32_wplanes_ok)
        key = (M, N, K, bool(gelu))
        ok = self.shape_ok.get(key)
        if ok is None:
            ok = self.shape_ok[key] = bool(lib.rscotr_gemm_f32_wplanes_ok(M, N, K, int(bool(gelu))))
        return ok and STATE.grad_sink.is_param_ptr(B.data_ptr())

    def get(self, B, N, K, ldb, b_kmajor):
        """-> (planes pointer, npad) of the weight behind operand B (N output rows, reduction K), fresh."""
        e = self._entry((B.data_ptr(), N, K, ldb, int(b_kmajor)), B.device)
        return e['planes'].data_ptr(), e['pad']

    def _size(self, key, device):
        _, N, K, _, _ = key
        npad = (N + 255) // 256 * 256
        return self._planes(npad * K * 3, npad, (npad * (K // 16) + 255) // 256, device)


class _WeightPlanesH(_PlaneCache):
    """fp16 planes of the weights that serve as B operand of the interior pipelined 64 x 64 fp16 split kernel (round 5,
    rscotr_gemm_split_weights_h3 / rscotr_gemm_f32_rb): y = x W^T takes the planes of W, dx = dy W those of W^T.  A plane set
    carries the scale of the parameter's range word at the time of the split, and that word only changes in the optimizer step."""

    ENTRY = 'rscotr_gemm_split_weights_h3'

    def eligible(self, B, M, N, K, lda, ldb, a_kmajor, b_kmajor, act, pre, rowscale, kscale, nws):
        sink = STATE.grad_sink
        if not self.enabled or not RANGES.enabled or a_kmajor or sink is None or K % 32 or ldb % 4 or B.data_ptr() % 16:
            return False
        if not sink.is_param_ptr(B.data_ptr()):
            return False
        key = (M, N, K, lda, ldb, int(a_kmajor), int(b_kmajor), int(act), pre is not None, rowscale is not None, kscale is not None,
               nws, lib.rscotr_gemm_get_precision())
        r = RANGES.route2.get(key)
        if r is None:
            r = RANGES.route2[key] = lib.rscotr_gemm_f32_split_route(M, N, K, lda, ldb, int(a_kmajor), int(b_kmajor), int(act),
                                                                     int(pre is not None), int(rowscale is not None),
                                                                     int(kscale is not None), nws) == 2
        return r

    def get(self, B, N, K, ldb, b_kmajor, word):
        """-> (planes pointer, rpad) of the weight behind operand B (N plane rows, reduction K), fresh."""
        e = self._entry((B.data_ptr(), N, K, ldb, int(b_kmajor)), B.device, word=int(word))
        return e['planes'].data_ptr(), e['pad']

    def _size(self, key, device):
        _, N, K, _, _ = key
        rpad = (N + 63) // 64 * 64
        return self._planes(rpad * K * 2, rpad, (rpad * (K // 32) + 255) // 256, device)

    def _row(self, key, e, first):
        return super()._row(key, e, first) + (e['word'],)


class _WeightPlanesF(_PlaneCache):
    """FRAGMENT-MAJOR fp16 planes of the weights of a fused FFN (round 6, rscotr_gemm_split_weights_frag / rscotr_ffn_h3,
    csrc/ffn.hip): the weight operand of one wavefront's 16 x 16 x 32 MFMA as one contiguous 1 KB record.  Like HPLANES, a set carries
    the scale of the parameter's range word at the time of the split."""

    ENTRY = 'rscotr_gemm_split_weights_frag'

    def get(self, W, tr, word):
        """-> planes pointer for the operand Wop = W (tr = 0: plane rows = rows of W, reduction over its columns) or W^T (tr = 1);
        W: a contiguous matrix, a parameter or a row block of one."""
        wr, wc = W.shape
        return self._entry((W.data_ptr(), wr, wc, wc, int(tr)), W.device, word=int(word))['planes'].data_ptr()

    def _size(self, key, device):
        _, wr, wc, _, tr = key
        rows, red = (wc, wr) if tr else (wr, wc)
        assert rows % 16 == 0 and red % 32 == 0
        return self._planes(wr * wc * 2, 0, (wr * wc // 8 + 255) // 256, device)

    def _row(self, key, e, first):
        ptr, wr, wc, ldw, tr = key
        return (ptr, e['planes'].data_ptr(), wr, wc, ldw, 0, first, tr, e['word'])


WPLANES = _WeightPlanes()
HPLANES = _WeightPlanesH()
FPLANES = _WeightPlanesF()
_CACHES = (WPLANES, HPLANES, FPLANES)
