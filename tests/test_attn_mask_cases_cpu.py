"""The structured-mask cases of tests/test_mha_gpu.py reach the paths they are meant for: a CPU census of their 32 x 32 tiles
(all-True tiles the fused core skips, all-False tiles it runs without mask arithmetic, mixed tiles, a whole blocked chunk),
the fully blocked rows they declare, and a finite fp64 reference."""
import numpy as np
import pytest
import torch

import attn_mask_cases as amc
from attn_mask_cases import ALL_FALSE, ALL_TRUE, CASES, MHA_MASKS, MIXED


def test_dino_dn_mask_definition():
    m = amc.dino_dn_mask(3, 40, 70)
    pad, L = 120, 190
    assert m.shape == (L, L) and m.dtype == torch.bool
    assert bool(m[pad:, :pad].all())          # matching rows never see a denoising column
    assert not bool(m[:, pad:].any())         # matching columns are visible to everyone
    for gi in range(3):
        rows = slice(40 * gi, 40 * gi + 40)
        assert not bool(m[rows, rows].any())  # a group sees itself
        other = torch.ones(pad, dtype=torch.bool)
        other[rows] = False
        assert bool(m[rows, :pad][:, other].all())  # and no other group


def test_region_mask_definition():
    m = amc.region_mask((2, 40, 200), [(None, 0, 40, 50, 150)], seed=3, rough=2, blocked_rows=((1, 7),))
    assert m.shape == (2, 40, 200) and bool(m[..., :50].all()) and bool(m[..., 150:].all())
    assert not bool(m[0, :, 52:148].any())
    vis = (~m).sum(-1)
    assert int(vis[1, 7]) == 0 and int((vis == 0).sum()) == 1
    assert int(vis.max()) <= 100 and int(vis[0].min()) >= 96
    assert len(set(vis[0].tolist())) > 1  # the edges are roughened
    assert torch.equal(m, amc.region_mask((2, 40, 200), [(None, 0, 40, 50, 150)], seed=3, rough=2, blocked_rows=((1, 7),)))
    with pytest.raises(AssertionError):
        amc.region_mask((40, 200), [(None, 0, 39, 50, 150)])  # row 39 outside every region


def test_tile_census_counts_the_ragged_edge_as_blocked():
    m = torch.zeros(40, 70, dtype=torch.bool)
    m[:, 64:] = True
    m[33, :] = True
    c = amc.tile_census(m, 40, 70)
    assert c['codes'].shape == (1, 2, 3)
    # query block 0: two all-False tiles, keys 64..69 blocked + 70..95 out of range -> all-True
    assert c['codes'][0, 0].tolist() == [ALL_FALSE, ALL_FALSE, ALL_TRUE]
    # query block 1: rows 40..63 out of range -> mixed, the last still all-True
    assert c['codes'][0, 1].tolist() == [MIXED, MIXED, ALL_TRUE]
    assert (c['all_true'], c['all_false'], c['mixed'], c['blocked_rows']) == (2, 2, 2, 1)


@pytest.mark.parametrize('name', [n for n in CASES if CASES[n]['mode']])
def test_case_census(name):
    c = CASES[name]
    mask = amc.case_mask(name)
    shape = {1: (c['Lq'], c['Lk']), 2: (c['B'], c['Lq'], c['Lk']), 3: (c['B'] * c['H'], c['Lq'], c['Lk'])}[c['mode']]
    assert tuple(mask.shape) == shape and mask.dtype == torch.bool
    cen = amc.tile_census(mask, c['Lq'], c['Lk'])
    print(name, {k: v for k, v in cen.items() if k != 'codes'})
    assert cen['all_true'] >= 1 and cen['mixed'] >= 1
    if c.get('no_all_false'):
        assert cen['all_false'] == 0
    else:
        assert cen['all_false'] >= 1
    assert cen['blocked_rows'] == len(c['blocked'])
    rows = mask.reshape(-1, c['Lq'], c['Lk']).all(-1).nonzero().tolist()
    assert sorted(map(tuple, rows)) == sorted(c['blocked'])
    for (qb, kb), code in c.get('expect', {}).items():
        assert cen['codes'][0, qb, kb] == code, (qb, kb)
    if 'chunk_tiles' in c:
        per, ch = c['chunk_tiles'], c['blocked_chunk']
        chunk = cen['codes'][:, :, ch * per:(ch + 1) * per]
        assert chunk.shape[-1] == per
        assert bool((chunk == ALL_TRUE).all(-1).any()), 'no query block with a whole chunk of all-True tiles'


def test_chunk_cases_block_the_first_tile_of_every_wavefront_and_split_the_rows():
    for name in ('region_img', 'region_img_open', 'region_head'):
        codes = amc.tile_census(amc.case_mask(name), 32, 1024)['codes']
        assert bool((codes[:, 0, 16:20] == ALL_TRUE).all())      # chunk 2: tiles 16..19 = the first tile of wavefronts 0..3
        assert bool((codes[:, 0, 20:24] != ALL_TRUE).all())      # ... and their second tile is live
        m = amc.case_mask(name).reshape(-1, 32, 1024)
        sees = ~m[:, :, 768:].all(-1)  # chunk 3: rows 0..15 see it (but for the declared blocked row), rows 16..31 do not
        assert not bool(sees[:, 16:].any())
        for blk in range(m.shape[0]):
            dead = sorted(r for b, r in CASES[name]['blocked'] if b == blk)
            assert (~sees[blk, :16]).nonzero().flatten().tolist() == dead


@pytest.mark.parametrize('name', sorted(MHA_MASKS))
def test_mha_mask_census(name):
    build, Lq, Lk = MHA_MASKS[name]
    cen = amc.tile_census(build(), Lq, Lk)
    print(name, {k: v for k, v in cen.items() if k != 'codes'})
    assert cen['all_true'] >= 1 and cen['all_false'] >= 1 and cen['mixed'] >= 1 and cen['blocked_rows'] == 0


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_reference_is_finite(name):
    c = CASES[name]
    ref = amc.case_reference(name)
    for k in ('out', 'dq', 'dk', 'dv'):
        assert bool(torch.isfinite(ref[k]).all()), k
    inf = ~torch.isfinite(ref['lse'])
    assert int(inf.sum()) == len(c['blocked']) * (c['H'] if c['mode'] == 2 else 1)
    assert bool((ref['lse'][inf] == float('-inf')).all())  # (log of an empty sum; the kernel marks such a row with +inf)
    assert float(ref['out'].abs().max()) > 0 and float(ref['dk'].abs().max()) > 0


def test_softmax_reference_is_finite_and_normalised():
    mask = amc.case_mask('region_img')
    g = torch.Generator().manual_seed(5)
    S, dP = torch.randn(1, 8, 32, 1024, generator=g), torch.randn(1, 8, 32, 1024, generator=g)
    p, ds = amc.softmax_reference(S, mask, 2, 1, 8, 32 ** -0.5, dP)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(ds).all())
    sums = p.sum(-1)
    assert float((sums[:, :, 5]).abs().max()) == 0.0 and float(ds[:, :, 5].abs().max()) == 0.0
    live = np.ones(32, dtype=bool)
    live[5] = False
    assert float((sums[:, :, live] - 1).abs().max()) < 1e-12
