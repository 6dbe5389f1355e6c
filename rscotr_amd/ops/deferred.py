"""The deferred end-of-backward work (`DEFER`): split-K slabs of weight gradients, partial rows of the LayerNorm and window-attention
parameter gradients and the grouped small-output weight gradients wait in pending lists and are folded into the gradient arena by a few
launches of `flush_deferred()`.  The pending entries are the named tuples below; their field order IS the column order of the device
tables the flush kernels read (include/rscotr.h)."""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from .._lib import _TRACE
from .core import ACT_NONE, _ptr, _stream, lib
from .ranges import RANGES
from .state import STATE


class Slab(NamedTuple):
    """`splits` slabs of an (M, N) weight gradient (and of its M row sums: the bias gradient) for rscotr_splitk_flush.
    out == 0: row sums only."""
    slab: int
    rs_slab: int
    out: int
    rowsum: int
    M: int
    N: int
    ldc: int
    splits: int


class LnPart(NamedTuple):
    """`rows` partial rows of a LayerNorm's (dw | db) of width C for rscotr_layernorm_flush (ops.norm)."""
    part: int
    dw: int
    db: int
    rows: int
    C: int


class WattnPart(NamedTuple):
    """Partial rows of a window attention's bias-table / pad-token gradients for rscotr_swin_wattn_flush (ops.attention)."""
    part: int
    dtable: int
    dbias: int
    heads: int
    C: int
    rows: int


class GroupProblem(NamedTuple):
    """One dW = A^T B (+ row sums) of the grouped launch rscotr_gemm_dw_group; range_a / range_b: range slots of the operands | 0."""
    a: int
    b: int
    out: int
    rowsum: int
    kscale: int
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    krows_per: int
    range_a: int = 0
    range_b: int = 0


class _DeferredCombine:
    """Split-K weight-gradient contractions whose result is ACCUMULATED into the gradient arena leave their slabs in a
    private region and are combined by ONE launch at the end of the backward pass (`flush_deferred`, called by the
    runner / optimizer before anything reads the arena) instead of one combine launch each: ~450 launches per
    co-training round become ~10 (one per task, plus one per repeated use of a shared parameter).  The (slab, destination, shape) table of a pass is static across iterations (slab
    regions are handed out in call order, destinations are arena addresses), so its device copy is cached by content
    and a captured hipGraph replays the same flush."""

    BLOCK = 256 << 20
    MAX_TABLES = 64
    GROUP_MAX_OUT = 160000         # M * N of a grouped problem
    GROUP_MAX_OUT_SHORT = 2500000  # ... with a short reduction (K <= GROUP_SHORT_K)
    GROUP_SHORT_K = 4096
    GROUP_EDGE = 48                # members with min(M, N) >= this on the split product's 128 x 128 edge body
    GROUP_TARGET_WGS = 4608        # workgroups a grouped launch aims at

    def __init__(self):
        self.enabled = True
        self.blocks, self.cur, self.off = [], 0, 0
        self.entries, self.notify, self.cache = [], [], {}
        self.ln_entries, self.ln_cache = [], {}
        # flush tables are addressed by raw pointer from captured hipGraphs: a table that was looked up while a graph
        # was being warmed up / captured (`pin = True`, set by runner.GraphedTask) is never evicted; the others are
        # dropped oldest-first once more than MAX_TABLES signatures have been seen
        self.pin = False
        self.pinned = set()
        # weight gradients with small outputs are not launched one by one: their operands are kept alive and ONE grouped
        # launch at the end of backward computes them all (rscotr_gemm_dw_group), then the combine below folds the slabs
        self.group_enabled = True
        self.group_x6 = 1  # 0: every member on the fp32 pipe's 64 x 64 tiles
        self.group, self.group_keep, self.group_cache = [], [], {}
        self.group_amax, self.amax_cache = {}, {}  # operands of grouped problems whose value range is measured at the flush
        self.pinned_pool, self.pinned_live = [], []
        self.captured = []  # (cache, signature) of the tables built during the capture in progress
        self.wattn_entries, self.wattn_cache = [], {}

    def grouped_size(self, M, N, K):
        return M * N <= self.GROUP_MAX_OUT or (K <= self.GROUP_SHORT_K and M * N <= self.GROUP_MAX_OUT_SHORT)

    def split_member(self, M, N, K):
        """Is a grouped problem of this shape a member of the split-product launch (given aligned operands: `_plan_group`)?  Such a
        member wants the value ranges of its operands (`_try_defer_dw` collects them)."""
        return bool(self.group_x6 and K >= 512 and K % 16 == 0 and M % 4 == 0 and N % 4 == 0 and min(M, N) >= self.GROUP_EDGE)

    def _plan_group(self):
        """Slices and slab regions of the pending grouped problems -> ([(device table, problems, workgroups, variant, flops)],
        combine entries).  Members of the split-product launch run its 128 x 128 edge body — with both value ranges as the fp16 split
        product (variant 7), else as the six-term bf16 product (6) — the rest the fp32 pipe's 64 x 64 tiles (0): one launch each."""
        probs = [GroupProblem(*p) for p in self.group]  # (callers without value ranges append the first 11 fields)

        def kind(p):
            if not (self.split_member(p.M, p.N, p.K) and p.lda % 4 == 0 and p.ldb % 4 == 0 and p.a % 16 == 0 and p.b % 16 == 0):
                return 0
            # with the value range of both operands: the same body as the fp16 split product (whose k loop addresses a tile with
            # 32-bit offsets: leading dimensions below 2^26, csrc/gemm_split_body.h thread_offset)
            return 7 if p.range_a and p.range_b and RANGES.enabled and max(p.lda, p.ldb) < 1 << 26 else 6

        def row(m, first):
            """Table row of member m (None: a bundle's padding) whose bundle starts at workgroup `first`."""
            if m is None:
                return [0] * 12 + [first, 0, 0, 0]
            p = m['p']
            return [p.a, p.b, m['slab'], m['rs_slab'], p.kscale, p.M, p.N, p.K, p.lda, p.ldb, m['klen'], m['splits'], first,
                    max(p.krows_per, 1), m['ranges'], m['wgs']]

        kinds = [kind(p) for p in probs]
        tiles = [((p.M + 127) // 128) * ((p.N + 127) // 128) if k else ((p.M + 63) // 64) * ((p.N + 63) // 64)
                 for k, p in zip(kinds, probs)]
        # k-slices of about equal WORK per workgroup (a 128 x 128 tile does four times the work of a 64 x 64 one per k), per
        # LAUNCH: with one target for the whole pass the few fp32 64 x 64 members of a det backward (the 4- and 20-row
        # reg / cls branches over K = 10880) inherited the k-slice of the big bf16x6 launch and ran as 160 workgroups of
        # K = 3632 each: 260 us for 0.1 GFLOP
        dev = self.group_keep[0].device
        launches, ents = [], []
        for variant in (0, 6, 7):
            big = 4 if variant else 1
            klen_t = max(256, -(-sum(t * p.K * big for t, k, p in zip(tiles, kinds, probs) if k == variant) // self.GROUP_TARGET_WGS))
            kq = 32 if variant else 16  # (k-slices of whole steps of the body: the one-stage split loop takes 32 k per barrier pair, the fp32 body 16)
            members = []
            for t, k, p in zip(tiles, kinds, probs):
                if k != variant:
                    continue
                sp = max(1, -(-p.K // max(256, klen_t // big)))
                klen = -(-(-(-p.K // sp)) // kq) * kq
                sp = -(-p.K // klen)
                if sp == 1:
                    klen = p.K
                slab = self.reserve(sp * (p.M * p.N + p.M) * 4, dev)
                rs_slab = slab + sp * p.M * p.N * 4 if p.rowsum else 0
                rng = ((RANGES.index(p.range_a) + 1) << 32 | (RANGES.index(p.range_b) + 1)) if variant == 7 else 0
                members.append(dict(p=p, slab=slab, rs_slab=rs_slab, klen=klen, splits=sp, ranges=rng, wgs=t * sp))
                ents.append(Slab(slab, rs_slab, p.out, p.rowsum, p.M, p.N, p.N, sp))
            if members:
                # bundles of 8 problems of similar size, one problem per XCD (the kernel's id layout): largest first
                members.sort(key=lambda m: -m['wgs'])
                members += [None] * (-len(members) % 8)
                rows, first = [], 0
                for b0 in range(0, len(members), 8):
                    rows += [row(m, first) for m in members[b0:b0 + 8]]
                    first += 8 * members[b0]['wgs']
                flops = float(sum(2.0 * m['p'].M * m['p'].N * m['p'].K for m in members if m is not None))
                launches.append((self._upload(np.asarray(rows, dtype=np.int64), dev), len(rows), first, variant, flops))
        return launches, ents

    def prepare_capture(self, n=4):
        """Pinned staging buffers for tables that have to be built WHILE a hipGraph is being captured (the grouped launch's
        table holds activation addresses, which differ between the warm-up iterations and the capture): a pageable
        host-to-device copy is not capturable, a pinned one is — and the replayed copy node re-reads the pinned buffer,
        which therefore lives as long as the cache entry."""
        while len(self.pinned_pool) < n:
            self.pinned_pool.append(torch.empty((4096, 16), dtype=torch.int64).pin_memory())

    @staticmethod
    def _copy(arr, dev):
        return torch.from_numpy(arr).to(dev)

    def _upload(self, arr, dev):
        """Device copy of a table; while a hipGraph is being captured, through a pinned staging buffer (`prepare_capture`)."""
        if dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            assert arr.size <= 4096 * 16, f'a table of {arr.size} words does not fit a staging buffer'
            assert self.pinned_pool, ('no staging buffer left for a table built during a capture: the pool is exhausted '
                                      f'({len(self.pinned_live)} taken), or DEFER.prepare_capture() did not run')
            host = self.pinned_pool.pop()
            stage = host.view(-1)[:arr.size].view(arr.shape)  # (tables of any row width share the (4096, 16) staging buffers)
            stage.copy_(torch.from_numpy(arr))
            d = torch.empty(arr.shape, dtype=torch.int64, device=dev)
            d.copy_(stage, non_blocking=True)
            self.pinned_live.append(host)
            return d
        return self._copy(arr, dev)

    def forget_captured(self):
        """A capture was abandoned (a failed capture, or the ranks' agreement to fall back to the split form): the tables that
        were built while it was being recorded were to be filled by the graph's own copy nodes, which will never run —
        their cache entries must not be found by the next capture, whose private pool hands out the same addresses."""
        for cache, sig in self.captured:
            cache.pop(sig, None)
            self.pinned.discard(sig)
        self.captured = []

    def keep_captured(self):
        """The capture is kept: its tables are refilled by every replay."""
        self.captured = []

    def _remember(self, cache, sig, hit):
        if sig not in cache and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            self.captured.append((cache, sig))
        if self.pin:
            self.pinned.add(sig)
        if sig not in cache:
            cache[sig] = hit
            if len(cache) > self.MAX_TABLES:
                for k in list(cache):
                    if len(cache) <= self.MAX_TABLES:
                        break
                    if k not in self.pinned and k != sig:
                        del cache[k]

    def reserve(self, nbytes, device):
        nbytes = (nbytes + 255) // 256 * 256
        while True:
            if self.cur == len(self.blocks):
                self.blocks.append(torch.empty(max(self.BLOCK, nbytes) // 4, dtype=torch.float32, device=device))
            b = self.blocks[self.cur]
            if self.off + nbytes <= b.numel() * 4:
                ptr = b.data_ptr() + self.off
                self.off += nbytes
                return ptr
            self.cur, self.off = self.cur + 1, 0

    def pending(self):
        return bool(self.entries or self.ln_entries or self.group or self.wattn_entries)

    def drop(self):
        self.entries, self.notify, self.ln_entries = [], [], []
        self.group, self.group_keep = [], []
        self.group_amax = {}
        self.wattn_entries = []
        self.cur = self.off = 0

    @staticmethod
    def _rounds(entries, dests):
        """Entries that share a destination go to successive launches (the combine is a plain read-add-write)."""
        seen, rounds = {}, []
        for e in entries:
            ds = [d for d in dests(e) if d]
            k = max([seen.get(d, 0) for d in ds] or [0])
            for d in ds:
                seen[d] = k + 1
            while len(rounds) <= k:
                rounds.append([])
            rounds[k].append(e)
        return rounds

    def _flush_queue(self, entries, cache, kind, dests, plan, entry_point, upload):
        """Fold one queue of pending entries (tuples of type `kind`): rounds by destination (`_rounds`), per round the tables and
        scalar arguments `plan(round)` -> (arrays, scalars) states, uploaded and cached under the queue's content, one launch each."""
        sig = tuple(entries)
        hit = cache.get(sig)
        if hit is None:
            dev = self.blocks[0].device
            hit = []
            for ents in self._rounds([kind(*e) for e in entries], dests):
                arrays, scalars = plan(ents)
                hit.append((tuple(upload(a, dev) for a in arrays), scalars))
        self._remember(cache, sig, hit)
        for tabs, scalars in hit:
            lib.call(entry_point, *(t.data_ptr() for t in tabs), *scalars, _stream())

    @staticmethod
    def _workgroups(ents, count):
        """(entry, block) of every workgroup of a fold launch: count(e) blocks for entry e."""
        return np.asarray([(r, c) for r, e in enumerate(ents) for c in range(count(e))], dtype=np.int32)

    def _plan_ln(self, ents):
        wg = self._workgroups(ents, lambda e: (2 * e.C + 63) // 64)
        return (np.asarray(ents, dtype=np.int64), wg), (len(wg),)

    def _plan_wattn(self, ents):
        rows, first = [], 0
        for e in ents:
            rows.append(tuple(e) + (first,) + (0,) * 9)
            first += e.heads
        return (np.asarray(rows, dtype=np.int64),), (len(rows), first)

    def _plan_splitk(self, ents):
        wg = self._workgroups(ents, lambda e: (max(e.M * e.N // 4, e.M) + 255) // 256)
        nbytes = float(sum((e.splits + 2) * (e.M * e.N + e.M) * 4 for e in ents))  # slabs read, destination read + written
        return (np.asarray(ents, dtype=np.int64), wg), (len(wg), nbytes)

    def group_range(self, t, rows, cols, ld):
        """Range slot of an operand of a grouped problem: what the tensor carries / the optimizer keeps, else a fresh slot
        that ONE launch fills for all such operands right before the grouped product (`_flush_group`).  Such a slot is
        not handed on with the tensor: nothing may read it before the flush."""
        s = RANGES.slot_of(t)
        if s:
            return s
        sink = STATE.grad_sink
        if sink is not None and sink.is_param_ptr(t.data_ptr()):
            return RANGES.of(t, rows, cols, ld)
        key = (t.data_ptr(), rows, cols, ld)
        s = self.group_amax.get(key)
        if s is None:
            s = self.group_amax[key] = RANGES.new_slot(t.device)
            if _TRACE:
                import sys
                end = t.storage_offset() * 4 + ((rows - 1) * ld + cols) * 4
                print(f'[group_range] {tuple(t.shape)} rows={rows} cols={cols} ld={ld} last byte {end} of storage {t.untyped_storage().nbytes()}'
                      + ('  <-- OUT OF BOUNDS' if end > t.untyped_storage().nbytes() else ''), file=sys.stderr, flush=True)
        return s

    def _measure_group(self):
        sig = tuple(self.group_amax.items())
        hit = self.amax_cache.get(sig)
        if hit is None:
            rows_, first = [], 0
            for (ptr, rows, cols, ld), slot in self.group_amax.items():
                rows_.append((ptr, rows, cols, ld, slot, first))
                first += max(1, min(128, rows * cols // 65536))
            hit = (self._upload(np.asarray(rows_, dtype=np.int64), self.group_keep[0].device), len(rows_), first)
        self._remember(self.amax_cache, sig, hit)
        table, n, total = hit
        lib.call('rscotr_amax_group', table.data_ptr(), n, total, _stream())
        RANGES.stats['grouped'] = RANGES.stats.get('grouped', 0) + n
        self.group_amax = {}

    def _flush_group(self):
        if self.group_amax:
            self._measure_group()
        sig = (tuple(self.group), self.cur, self.off)  # (the slab regions continue where this pass's reserves stand)
        hit = self.group_cache.get(sig)
        if hit is None:
            hit = self._plan_group() + (self.cur, self.off)
        launches, ents, self.cur, self.off = hit
        self._remember(self.group_cache, sig, hit)
        for table, n, total, variant, flops in launches:
            lib.call('rscotr_gemm_dw_group', table.data_ptr(), n, total, variant, flops, RANGES.base if variant == 7 else 0,
                     _stream())
        self.entries.extend(ents)
        self.group, self.group_keep = [], []

    def flush(self):
        if self.group:
            self._flush_group()
        if self.ln_entries:
            self._flush_queue(self.ln_entries, self.ln_cache, LnPart, lambda e: (e.dw, e.db), self._plan_ln,
                              'rscotr_layernorm_flush', self._copy)
            self.ln_entries = []
        if self.wattn_entries:
            # (one fold launch, or one per round when a block's destinations are pending more than once: the same block twice in
            #  one pass, or passes accumulated without a flush in between)
            self._flush_queue(self.wattn_entries, self.wattn_cache, WattnPart, lambda e: (e.dtable, e.dbias), self._plan_wattn,
                              'rscotr_swin_wattn_flush', self._upload)
            self.wattn_entries = []
        if self.entries:
            # a parameter used several times in one pass (ref_point_head and the shared heads of the DINO decoder: 6-7
            # contractions into one destination) must not be combined by concurrent workgroups: entry k of a destination goes
            # to launch k (out == 0: row-sum partials only — the bias gradient of a split pass)
            self._flush_queue(self.entries, self.cache, Slab, lambda e: (e.out, e.rowsum), self._plan_splitk,
                              'rscotr_splitk_flush', self._copy)
        notify, self.notify = self.notify, []
        self.entries = []
        self.cur = self.off = 0
        if STATE.grad_sink is not None:
            for i in notify:
                STATE.grad_sink._on_ready(i)


DEFER = _DeferredCombine()


def _ranges_invalidated():
    """RANGES.begin() / a wrap of the slot buffer while grouped weight gradients are still pending (gradient accumulation, an
    evaluation forward between backward and the flush): the raw slot addresses they hold are zero words or someone else's now.
    The problems fall back to the member kind that needs no ranges (the six-term bf16 body), the to-be-measured list is dropped."""
    DEFER.group = [GroupProblem(*p)._replace(range_a=0, range_b=0) for p in DEFER.group]
    DEFER.group_amax = {}


RANGES.on_invalidate.append(_ranges_invalidated)


def flush_deferred():
    """Compute the grouped weight gradients and combine the pending split-K weight gradients / LayerNorm parameter
    gradients into the arena (no-op when nothing is pending)."""
    if DEFER.pending() or DEFER.notify:
        DEFER.flush()


def _in_arena(t):
    sink = STATE.grad_sink
    if sink is None or t is None:
        return False
    lo = sink.flat_g.data_ptr()
    return lo <= t.data_ptr() < lo + sink.flat_g.numel() * 4


def _try_defer_dw(A, B, out, M, N, K, lda, ldb, rowsum, kscale, krows_per, nws):
    """-> True if the contraction was issued as slabs for the deferred combine."""
    if not DEFER.enabled or STATE.side is not None or N % 4 or out.data_ptr() % 16 or not _in_arena(out):
        return False
    if DEFER.group_enabled and DEFER.grouped_size(M, N, K) and K >= 16:
        # small output: joins the grouped launch at the end of backward (operands stay alive until then)
        sa = sb = 0
        if DEFER.split_member(M, N, K) and RANGES.enabled:
            sa, sb = DEFER.group_range(A, K, M, lda), DEFER.group_range(B, K, N, ldb)
            lo_r, hi_r = RANGES.base, RANGES.base + 4 * RANGES.STRIDE
            if not (lo_r <= sa < hi_r and lo_r <= sb < hi_r):
                sa = sb = 0
        DEFER.group.append(GroupProblem(A.data_ptr(), B.data_ptr(), out.data_ptr(), _ptr(rowsum), _ptr(kscale), M, N, K, lda, ldb,
                                        int(krows_per), sa, sb))
        DEFER.group_keep.extend(t for t in (A, B, kscale) if t is not None)
        return True
    if nws == 0:
        return False
    ptr = DEFER.reserve(nws, A.device)
    splits = ctypes.c_int32(1)
    sa = sb = 0
    if RANGES.wanted(M, N, K, lda, ldb, 1, 1, ACT_NONE, False, False, kscale is not None, nws):
        sa, sb = RANGES.of(A, K, M, lda), RANGES.of(B, K, N, ldb)  # (the two k-major operands)
    lib.call('rscotr_gemm_f32_dw_slabs_r', A.data_ptr(), B.data_ptr(), out.data_ptr(), M, N, K, lda, ldb, N, _ptr(rowsum),
             _ptr(kscale), int(krows_per), ptr, nws, ctypes.byref(splits), sa, sb, _stream())
    sp = splits.value
    if sp > 1:
        DEFER.entries.append(Slab(ptr, ptr + sp * M * N * 4 if rowsum is not None else 0, out.data_ptr(), _ptr(rowsum), M, N, N, sp))
    return True
