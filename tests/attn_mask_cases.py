"""Block-structured attention masks for the dense-attention tests, with the evidence that they reach the kernel paths.

Plain torch / numpy, written from the definitions in the papers (DINO's contrastive denoising groups: Zhang et al. 2022,
section 3.3 and DN-DETR's attention mask; Mask2Former's masked attention: Cheng et al. 2022, section 3.2.1), not from the
library's mask-building code.  True = blocked, as torch.nn.MultiheadAttention reads a bool attn_mask.

The fused core (csrc/attn_core.hip) walks the score matrix in aligned 32 x 32 tiles: a tile whose mask block is all True is
skipped without a product, a tile without any True bit runs without mask arithmetic, and with few query tiles the keys are cut
into chunks merged by a second launch.  `tile_census` counts, on the CPU, the tiles of each kind a mask holds, so that
tests/test_attn_mask_cases_cpu.py can assert that every case below contains them; tests/test_mha_gpu.py imports the same cases.
"""
import functools

import numpy as np
import torch

TILE = 32
ALL_FALSE, MIXED, ALL_TRUE = 0, 1, 2


def dino_dn_mask(ngroups, gsize, nmatch):
    """(L, L) bool, L = ngroups * gsize + nmatch: the first `pad = ngroups * gsize` queries are the denoising groups, the rest the
    matching queries.  A matching row must not see any denoising column (they carry ground truth); a denoising group must not
    see another group's columns; the matching columns are visible to everyone."""
    pad = ngroups * gsize
    L = pad + nmatch
    mask = torch.zeros(L, L, dtype=torch.bool)
    mask[pad:, :pad] = True
    for i in range(ngroups):
        lo, hi = i * gsize, (i + 1) * gsize
        mask[lo:hi, :lo] = True
        mask[lo:hi, hi:pad] = True
    return mask


def region_mask(shape, regions, seed=0, rough=2, blocked_rows=()):
    """Masked-attention masks of rectangular visible regions.  `shape` = (Lq, Lk) or (nblk, Lq, Lk) (a block per image or per
    image and head); `regions` = [(blk | None, r0, r1, k0, k1)]: rows r0:r1 of block blk (None: every block) see the keys
    k0:k1 and nothing else.  The two vertical edges of every region are roughened per row: each moves INWARD by a seeded random
    0..rough keys, so what lies outside the rectangles stays blocked exactly.  Every row must be covered by a region wider than
    2 * rough (no row is fully blocked) unless it is listed in `blocked_rows` = [(blk, row)], which are blocked entirely."""
    lead = shape[:-2]
    Lq, Lk = shape[-2:]
    nblk = int(np.prod(lead)) if lead else 1
    rng = np.random.RandomState(seed)
    mask = np.ones((nblk, Lq, Lk), dtype=bool)
    for blk, r0, r1, k0, k1 in regions:
        assert 0 <= r0 < r1 <= Lq and 0 <= k0 < k1 <= Lk and k1 - k0 > 2 * rough
        for b in (range(nblk) if blk is None else (blk,)):
            left = k0 + rng.randint(0, rough + 1, size=r1 - r0)
            right = k1 - rng.randint(0, rough + 1, size=r1 - r0)
            for i, r in enumerate(range(r0, r1)):
                mask[b, r, left[i]:right[i]] = False
    assert not mask.all(-1).any(), 'a row outside every region'
    for b, r in blocked_rows:
        mask[b, r] = True
    return torch.from_numpy(mask.reshape(tuple(shape)))


def band_mask(Lq, Lk, step, width):
    """(Lq, Lk) bool: row i sees the keys step * i .. step * i + width - 1 (a sliding band)."""
    i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
    return ~((j >= step * i) & (j < step * i + width))


def tile_census(mask, Lq, Lk):
    """Census of a mask over its flattened leading block dim.  The aligned 32 x 32 tiles are classified as the kernels classify
    them, with everything past the ragged edge (rows >= Lq, keys >= Lk) counted as blocked: `codes` (nblk, ceil(Lq/32),
    ceil(Lk/32)) holds ALL_FALSE / MIXED / ALL_TRUE, `all_true` / `all_false` / `mixed` their counts, `blocked_rows` the number
    of rows without a visible key."""
    m = mask.reshape(-1, Lq, Lk).numpy()
    nblk, nqb, nkb = m.shape[0], -(-Lq // TILE), -(-Lk // TILE)
    pad = np.ones((nblk, nqb * TILE, nkb * TILE), dtype=bool)
    pad[:, :Lq, :Lk] = m
    t = pad.reshape(nblk, nqb, TILE, nkb, TILE)
    codes = np.full((nblk, nqb, nkb), MIXED, dtype=np.int64)
    codes[t.all(axis=(2, 4))] = ALL_TRUE
    codes[~t.any(axis=(2, 4))] = ALL_FALSE
    return dict(codes=codes, all_true=int((codes == ALL_TRUE).sum()), all_false=int((codes == ALL_FALSE).sum()),
                mixed=int((codes == MIXED).sum()), blocked_rows=int(m.all(-1).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# the cases of the kernel-level tests.  mode: 0 none, 1 (Lq, Lk), 2 (B, Lq, Lk), 3 (B * H, Lq, Lk).  `blocked` = the fully
# blocked rows the case declares ((block, row) pairs of the mask).  `chunk_tiles`: key tiles per chunk the census of a chunked
# case was laid out for (the GPU test reads the chunk count back from the library and compares).
# ----------------------------------------------------------------------------------------------------------------------
def _chunk_regions(nblk):
    """Lq = 32 against Lk = 1024 in 4 chunks of 8 key tiles (a wavefront w of 4 walks the tiles t0 + w, t0 + w + 4 of a chunk):
    chunk 0 (keys 0..255): a region with all-False tiles inside, mixed tiles at its edges, all-True tiles behind it;
    chunk 1 (256..511): blocked for all 32 queries (the chunk leaves M = -big, L = 0 to the merge);
    chunk 2 (512..767): its first four tiles blocked — the first tile of every wavefront's walk — the rest visible;
    chunk 3 (768..1023): rows 0..15 see a region, rows 16..31 nothing."""
    reg = []
    for b in range(nblk):
        reg += [(b, 0, 32, 3 + b, 100 + 2 * b), (b, 0, 32, 640 + b, 768 - b), (b, 0, 16, 800 + 3 * b, 900 + b)]
    return reg


def _own_regions(B):
    """Lq = 40 against Lk = 1030 (33 key blocks, the last of 6 keys): a region with all-False tiles, the ragged tail visible
    (a mixed last tile), keys 500..599 visible to the second query tile only (the key-side walk over the query tiles skips its
    first tile, then meets a live one), everything else blocked for all queries (key blocks the key-side pass skips entirely)."""
    reg = []
    for b in range(B):
        reg += [(b, 0, 40, 40 + 5 * b, 200 + b), (b, 8, 40, 1000 - 3 * b, 1030), (b, 32, 40, 500 + b, 600)]
    return reg


CASES = {
    # DINO denoising mask, self-attention (q | k the strided halves of one tensor)
    'dino192': dict(B=2, H=8, Lq=192, Lk=192, mode=1, self_attn=True, blocked=(),
                    mask=lambda: dino_dn_mask(3, 40, 72),
                    expect={(0, 2): ALL_TRUE, (4, 0): ALL_TRUE, (0, 0): ALL_FALSE, (1, 1): MIXED}),
    'dino190': dict(B=2, H=8, Lq=190, Lk=190, mode=1, self_attn=True, blocked=(),
                    mask=lambda: dino_dn_mask(3, 40, 70),
                    expect={(0, 2): ALL_TRUE, (4, 0): ALL_TRUE, (0, 0): ALL_FALSE, (1, 1): MIXED}),
    # five denoising groups, seven query tiles: the key-side pass (a wavefront walks the query tiles w, w + 4) meets, for the keys
    # of the last group (key block 5), skipped tiles first and a live tile after them
    'dino224': dict(B=2, H=8, Lq=224, Lk=224, mode=1, self_attn=True, blocked=(),
                    mask=lambda: dino_dn_mask(5, 40, 24),
                    expect={(0, 5): ALL_TRUE, (1, 5): ALL_TRUE, (2, 5): ALL_TRUE, (3, 5): ALL_TRUE, (4, 5): ALL_TRUE, (5, 5): ALL_FALSE,
                            (6, 5): MIXED, (5, 1): ALL_TRUE, (0, 0): ALL_FALSE}),
    # region masks against chunked keys, one fully blocked query row.  'region_img' is ONE image of ONE query tile: its fully
    # blocked row puts a True bit into every tile, so it cannot hold an all-False tile (`no_all_false`); 'region_img_open' is
    # the same layout without the blocked row and does
    'region_img': dict(B=1, H=8, Lq=32, Lk=1024, mode=2, self_attn=False, blocked=((0, 5),), chunk_tiles=8, blocked_chunk=1,
                       no_all_false=True,
                       mask=lambda: region_mask((1, 32, 1024), _chunk_regions(1), seed=21, blocked_rows=((0, 5),))),
    'region_img_open': dict(B=1, H=8, Lq=32, Lk=1024, mode=2, self_attn=False, blocked=(), chunk_tiles=8, blocked_chunk=1,
                            mask=lambda: region_mask((1, 32, 1024), _chunk_regions(1), seed=21)),
    'region_head': dict(B=1, H=8, Lq=32, Lk=1024, mode=3, self_attn=False, blocked=((3, 5),), chunk_tiles=8, blocked_chunk=1,
                        mask=lambda: region_mask((8, 32, 1024), _chunk_regions(8), seed=22, blocked_rows=((3, 5),))),
    # a shared (mode 1) mask at a chunked shape: rows 0..31 all see keys 248..399, chunk 3 is blocked for them
    'band_chunked': dict(B=1, H=8, Lq=40, Lk=1024, mode=1, self_attn=False, blocked=(), chunk_tiles=8, blocked_chunk=3,
                         mask=lambda: band_mask(40, 1024, 8, 400)),
    # few query tiles against many ragged keys: the key-side pass with a key block per wavefront
    'own_plain': dict(B=2, H=8, Lq=40, Lk=1030, mode=0, self_attn=False, blocked=(), mask=lambda: None),
    'own_region': dict(B=2, H=8, Lq=40, Lk=1030, mode=2, self_attn=False, blocked=(),
                       mask=lambda: region_mask((2, 40, 1030), _own_regions(2), seed=23)),
}


@functools.lru_cache(maxsize=None)
def case_mask(name):
    return CASES[name]['mask']()


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(qk, kx | None, v, do) of a case on the CPU in fp32: self-attention reads q | k as the column halves of one (B, L, 2C)
    tensor, cross-attention q (B, Lq, C) and k (B, Lk, C); C = H * 32."""
    c = CASES[name]
    B, H, Lq, Lk = c['B'], c['H'], c['Lq'], c['Lk']
    C = H * 32
    g = torch.Generator().manual_seed(B * 1000 + Lq * 7 + Lk + 17 * c['mode'])
    qk = torch.randn(B, Lq, 2 * C if c['self_attn'] else C, generator=g)
    kx = None if c['self_attn'] else torch.randn(B, Lk, C, generator=g)
    v, do = torch.randn(B, Lk, C, generator=g), torch.randn(B, Lq, C, generator=g)
    return qk, kx, v, do


def attn_reference(q, k, v, do, mask, mode, B, H):
    """softmax(scale q k^T + mask) v and its gradients in fp64 on (B, L, H * 32) tensors; a fully blocked row (softmax of all
    -inf: NaN) counts as zeros.  -> dict(out (B, Lq, C), dq, dk, dv, lse (B, H, Lq) with +inf on fully blocked rows)."""
    hd = 32
    C = H * hd
    Lq, Lk = q.shape[1], k.shape[1]
    q6, k6, v6 = (t.double().reshape(B, -1, H, hd).transpose(1, 2).clone().requires_grad_(True) for t in (q, k, v))
    s = (q6 @ k6.transpose(-1, -2)) * hd ** -0.5
    if mask is not None:
        m4 = mask[None, None] if mode == 1 else (mask[:, None] if mode == 2 else mask.reshape(B, H, Lq, Lk))
        s = s.masked_fill(m4, float('-inf'))
    p = torch.softmax(s, -1)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
    o6 = p @ v6
    o6.backward(do.double().reshape(B, Lq, H, hd).transpose(1, 2))
    unhead = lambda t, L: t.transpose(1, 2).reshape(B, L, C)
    return dict(out=unhead(o6.detach(), Lq), dq=unhead(q6.grad, Lq), dk=unhead(k6.grad, Lk), dv=unhead(v6.grad, Lk),
                lse=torch.logsumexp(s.detach(), -1))


@functools.lru_cache(maxsize=None)
def case_reference(name):
    c = CASES[name]
    qk, kx, v, do = case_inputs(name)
    C = c['H'] * 32
    q, k = (qk[..., :C], qk[..., C:]) if c['self_attn'] else (qk, kx)
    return attn_reference(q, k, v, do, case_mask(name), c['mode'], c['B'], c['H'])


def softmax_reference(S, mask, mode, B, H, scale, dP):
    """P = softmax(scale S + mask) over the keys in fp64 (fully blocked rows -> zeros) and dS = scale P (dP - sum_k P_k dP_k),
    the product of dP with the softmax Jacobian, for S, dP (B, H, Lq, Lk)."""
    Lq, Lk = S.shape[-2:]
    s = S.double() * scale
    if mask is not None:
        m4 = mask[None, None] if mode == 1 else (mask[:, None] if mode == 2 else mask.reshape(B, H, Lq, Lk))
        s = s.masked_fill(m4, float('-inf'))
    p = torch.softmax(s, -1)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
    d = dP.double()
    return p, scale * p * (d - (p * d).sum(-1, keepdim=True))


# masks of the _MHA routing matrix that combine a mask with positional inputs / other head dims (census asserted as well)
def mha_region_img_mask():
    """(2, 70, 96) per-image regions for cross-attention (Lq = 70, Lk = 96)."""
    return region_mask((2, 70, 96), [(0, 0, 40, 2, 70), (0, 40, 70, 30, 96), (1, 0, 32, 34, 96), (1, 32, 70, 0, 60)], seed=31)


def mha_region_head_mask(H):
    """(2 * H, 70, 96) per-head regions for cross-attention."""
    reg = []
    for b in range(2 * H):
        reg += [(b, 0, 32, 32 + (b % 3), 96), (b, 32, 70, b % 5, 64 + (b % 7))]
    return region_mask((2 * H, 70, 96), reg, seed=32)


MHA_MASKS = {
    'dino190': (lambda: dino_dn_mask(3, 40, 70), 190, 190),
    'mha_region_img': (mha_region_img_mask, 70, 96),
    'mha_region_head16': (lambda: mha_region_head_mask(16), 70, 96),
}
