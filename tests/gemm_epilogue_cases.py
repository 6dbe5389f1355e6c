"""The epilogue forms of rscotr_gemm_f32* and the kernel routes they are tested on (tests/test_gemm_epilogue_routes_gpu.py; checked
on the host by tests/test_gemm_epilogue_cases_cpu.py): an fp64 reference of the formula at the head of csrc/gemm.hip, the argument
sets (FORMS) named after the epilogue code they select on a 64 x 64 tile, and the smallest shapes (ROUTES) that reach each kernel
instantiation behind plan_gemm."""
import collections
import math

import torch

ACT_NONE, ACT_RELU, ACT_GELU, ACT_RELU_GRAD, ACT_GELU_GRAD = 0, 1, 2, 3, 4


# ---- the fp64 reference ---------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad64(x):
    cdf = 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return cdf + x * pdf


def product64(A, B, ak, bk):
    """Aop Bop^T in fp64: Aop[m, k] = A[k, m] for a k-major A (stored (K, M)), A[m, k] otherwise; the same for B over n."""
    A, B = A.double(), B.double()
    return (A.t() if ak else A) @ (B if bk else B.t())


def reference(A, B, ak, bk, bias, act, aux, resid, c0, accumulate, rowscale, rows_per, want_out2, product=None):
    """-> (C, pre, C2 | None) in fp64; csrc/gemm.hip: v = Aop Bop^T + bias; pre = v; v = act(v) or v * act'(aux);
    v *= rowscale[m // rows_per]; then C = v + resid (+ c0 if accumulate) — or, with a second output, C = v (+ c0) and
    C2 = C + resid.  `product`: Aop Bop^T when the caller has it already (one fp64 product per shape)."""
    v = product64(A, B, ak, bk) if product is None else product.clone()
    if bias is not None:
        v = v + bias.double()
    pre = v.clone()
    if act == ACT_RELU:
        v = v.clamp(min=0)
    elif act == ACT_GELU:
        v = gelu64(v)
    elif act == ACT_RELU_GRAD:
        v = v * (aux > 0)
    elif act == ACT_GELU_GRAD:
        v = v * gelu_grad64(aux.double())
    else:
        assert act == ACT_NONE, act
    if rowscale is not None:
        M = v.shape[0]
        v = v * rowscale.double().repeat_interleave(rows_per)[:M, None]
    old = c0.double() if accumulate else 0.0
    r = resid.double() if resid is not None else 0.0
    if want_out2:
        C = v + old
        return C, pre, C + r
    return v + r + old, pre, None


# ---- the epilogue argument sets -------------------------------------------------------------------------------------
Form = collections.namedtuple('Form', 'bias act pre rowscale resid accumulate out2 selects')
FORMS = {
    'none':           Form(0, 0, 0, 0, 0, 0, 0, 'plain'),
    'bias':           Form(1, 0, 0, 0, 0, 0, 0, 'plain'),
    'bias_relu':      Form(1, 1, 0, 0, 0, 0, 0, 'noload'),
    'bias_gelu_pre':  Form(1, 2, 1, 0, 0, 0, 0, 'noload'),
    'resid':          Form(0, 0, 0, 0, 1, 0, 0, 'tile16_fast'),
    'bias_acc':       Form(1, 0, 0, 0, 0, 1, 0, 'tile16_fast'),
    'relu_grad':      Form(1, 3, 0, 0, 0, 0, 0, 'tile16_fast'),
    'gelu_grad':      Form(0, 4, 0, 0, 0, 0, 0, 'tile16_general'),
    'relu_resid':     Form(1, 1, 0, 0, 1, 0, 0, 'tile16_general'),
    'rowscale_resid': Form(0, 0, 0, 1, 1, 0, 0, 'tile16_general'),
    'pre_acc':        Form(1, 0, 1, 0, 0, 1, 0, 'tile16_general'),
    'rowscale':       Form(0, 0, 0, 1, 0, 0, 0, 'rows4'),
    'all':            Form(1, 4, 1, 1, 1, 1, 0, 'rows4'),
    'out2':           Form(0, 0, 0, 0, 0, 0, 1, 'rows4_c2'),
    'out2_all':       Form(1, 3, 0, 0, 1, 1, 1, 'rows4_c2'),
}


def selects(f, tile64=True):
    """The epilogue code a main kernel runs for these arguments: the predicates `plain`, `one_extra` and `noload` of
    csrc/gemm_split_body.h / csrc/gemm_tiled_body.h restated, in the order the kernels test them.  tile64 = False: the
    configurations without the 16-value batch (the 128-row tiles), where `one_extra` does not exist."""
    needs_aux = f.act in (ACT_RELU_GRAD, ACT_GELU_GRAD)
    plain = not f.pre and f.act == ACT_NONE and not f.resid and not f.accumulate and not f.rowscale and not f.out2
    one_extra = tile64 and not f.out2 and int(needs_aux) + int(bool(f.resid)) + int(bool(f.accumulate)) == 1
    noload = (not plain and f.act in (ACT_NONE, ACT_RELU, ACT_GELU) and not f.resid and not f.accumulate and not f.rowscale
              and not f.out2)
    if one_extra:  # epilogue_tile16: its fast inner path, or the general loop
        fast = not f.pre and not f.rowscale and f.act in (ACT_NONE, ACT_RELU_GRAD)
        return 'tile16_fast' if fast else 'tile16_general'
    if noload:
        return 'noload'
    if plain:
        return 'plain'
    return 'rows4_c2' if f.out2 else 'rows4'


def rows_per(M):
    """Rows per rowscale factor: the largest odd number <= (M - 1) // 3 — three samples of that many rows and a fourth of the one
    to six rows that are left.  Odd: every boundary (rows_per, 2 rows_per, 3 rows_per) falls inside a group of 4 rows and inside
    a 32-row accumulator tile; the last one, 3 rows_per >= M - 6, falls in the last 32 rows of every ragged M below — the ragged
    last tile of every tile height.  (M // 3 + 1 leaves its last boundary a third of M in front of that tile: 668 of 1000, 48
    of 70.)"""
    return ((M - 1) // 3 - 1) | 1


# ---- the route table ------------------------------------------------------------------------------------------------
# (M, N, K, a_kmajor, b_kmajor, precision mode) -> the launch name plan_name (csrc/gemm.hip) writes, what
# rscotr_gemm_f32_split_route answers, whether a combine launch follows (k-slices through slabs), and — for the rows of the
# small-product kernel — the name under a rowscale form, which small_gemm_ok refuses.  The name carries neither the loop form
# nor EDGE, the k-group count or the combine kernel: the comment of a row states the planner conditions its shape satisfies.
# No row had to move from the shape it was first derived at.
Route = collections.namedtuple('Route', 'M N K ak bk prec name split_route sliced rowscale_name')
_TF = ('false', 'true')


def _small(ak, bk):
    return f'rscotr::gemm_small_kernel<{_TF[ak]}, {_TF[bk]}, *>'


def _tiled(bm, bn, ak, bk):
    return f'rscotr::gemm_f32_kernel<{bm}, {bn}, {4 if bn == 32 else 2}, {1 if bn == 32 else 2}, {_TF[ak]}, {_TF[bk]}, *>'


def _dw(tm, tn):
    return f'rscotr::gemm_dw_direct_kernel<{tm}, {tn}>'


def _split(bm, ak, bk, fam='h3'):
    return f'rscotr::gemm_{fam}_kernel<{bm}, {bm}, {_TF[ak]}, {_TF[bk]}, *>'


COMBINE_NAME = 'rscotr::gemm_splitk_reduce_kernel'  # (the launch site's name of all three combine kernels)

ROUTES = [
    # the small-product kernel (small_gemm_ok: K % 8 == 0, 32 <= K <= 512, <= 512 tiles of 32 x 32; K / 8 octets -> 4, 8, 16 waves)
    Route(70, 45, 64, 0, 0, 3, _small(0, 0), 0, False, _tiled(64, 64, 0, 0)),     # 8 octets: 4 wavefronts
    Route(70, 45, 192, 0, 1, 3, _small(0, 1), 0, False, _tiled(64, 64, 0, 1)),    # 24 octets: 8 wavefronts
    Route(70, 45, 384, 1, 0, 3, _small(1, 0), 0, False, _tiled(64, 64, 1, 0)),    # 48 octets: 16 wavefronts
    Route(40, 45, 768, 0, 0, 3, _small(0, 0), 0, False, _tiled(64, 64, 0, 0)),    # K > 512: 4 tiles <= 8, 16 wavefronts
    # the fp32 tiled kernels (choose_cfg, choose_kgroups; K < 192 keeps mode 3 off the split route)
    Route(1280, 640, 48, 0, 0, 3, _tiled(64, 64, 0, 0), 0, False, None),          # 200 tiles, 3 k-tiles: one k-group, interior
    Route(640, 648, 100, 0, 0, 3, _tiled(64, 64, 0, 0), 0, False, None),          # 110 tiles, 7 k-tiles: two k-groups, EDGE (N, K)
    Route(1024, 1024, 192, 0, 0, 0, _tiled(64, 64, 0, 0), 0, False, None),        # mode 0; 256 tiles, 12 k-tiles: four k-groups
    Route(2000, 24, 100, 0, 1, 3, _tiled(128, 32, 0, 1), 0, False, None),         # N <= 32: 128 x 32, EDGE
    Route(4096, 1024, 128, 0, 0, 3, _tiled(128, 64, 0, 0), 0, False, None),       # N >= 1024, M >= 4096, M % 128 == 0: 128 x 64
    # fp32 tiled split-K (choose_cfg: fewer than 512 tiles, K >= 1024; 20 tiles of 64 are too few for choose_split6) and its combines
    Route(300, 200, 1024, 0, 0, 3, _tiled(64, 64, 0, 0), 0, True, None),          # 20 tiles: 4 slices of 256; reduce<true>
    Route(200, 260, 2056, 0, 0, 3, _tiled(64, 64, 0, 0), 0, True, None),          # 8 slices of 272, EDGE (K % 16); the sg combine
    Route(300, 202, 1024, 0, 0, 3, _tiled(64, 64, 0, 0), 0, True, None),          # N % 4 != 0: reduce<false>
    # the direct weight-gradient kernel (choose_dw_direct: both k-major, K >= 16384, 3 or 4 wave tiles); epilogue in the sg combine
    Route(288, 96, 16384, 1, 1, 3, _dw(3, 3), 0, True, None),                     # 3 tiles of 96 x 96, 86 slices
    Route(280, 92, 16392, 1, 1, 3, _dw(3, 3), 0, True, None),                     # ragged M, N and last slice
    Route(128, 200, 16384, 1, 1, 3, _dw(2, 4), 0, True, None),                    # 4 tiles of 64 x 128, 64 slices
    # the split product on 64 x 64 tiles (choose_split6: >= 256 tiles, 192 <= K <= 4096), as gemm_h3_kernel with both range words
    Route(1024, 1024, 192, 0, 0, 3, _split(64, 0, 0), 2, False, None),            # K % 32 == 0: pipelined loop, interior
    Route(1024, 1024, 208, 0, 1, 3, _split(64, 0, 1), 1, False, None),            # K % 32 != 0: two-stage loop, interior
    Route(1000, 1040, 196, 1, 0, 3, _split(64, 1, 0), 1, False, None),            # K % 16 != 0: two-stage loop, EDGE
    Route(1000, 1040, 224, 0, 0, 3, _split(64, 0, 0), 1, False, None),            # K % 32 == 0, ragged M / N: pipelined loop, EDGE
    # ... on 128 x 128 tiles (>= 512 of them, M and N % 128 == 0 or >= 1024)
    Route(2048, 4096, 192, 0, 0, 3, _split(128, 0, 0), 1, False, None),           # interior
    Route(2050, 4096, 200, 0, 1, 3, _split(128, 0, 1), 1, False, None),           # EDGE (M, K % 32)
    # ... k-sliced, the epilogue in the combine (96 <= tiles of 64 < 256 and K >= 1024; both k-major: 128-wide tiles from 24 of them)
    Route(512, 768, 1024, 0, 0, 3, _split(64, 0, 0), 2, True, None),              # 96 tiles: 4 slices of 256, interior; reduce<true>
    Route(512, 768, 1024, 0, 1, 3, _split(64, 0, 1), 2, True, None),
    Route(500, 780, 1040, 0, 0, 3, _split(64, 0, 0), 1, True, None),              # EDGE, 4 slices of 272 (two-stage loop)
    Route(512, 768, 2048, 1, 1, 3, _split(128, 1, 1), 1, True, None),             # 24 tiles of 128: 8 slices of 256; the sg combine
    Route(512, 768, 2080, 1, 1, 3, _split(128, 1, 1), 1, True, None),             # 8 slices of 288, the last one 64 long
]

# the six-term bf16 product (RSCOTR_GEMM_H3=0; here: no range words): the same tiles and loops as gemm_h3_kernel
SIX_TERM_ROUTES = [
    Route(1024, 1024, 192, 0, 0, 3, _split(64, 0, 0, 'bf16x6'), 2, False, None),
    Route(2050, 4096, 200, 0, 1, 3, _split(128, 0, 1, 'bf16x6'), 1, False, None),
]

# the scalar branches: epilogue_one in each of the three combine kernels (reduce<true>, the sg combine, reduce<false>) and a main
# kernel with unaligned rows of C
SCALAR_ROUTES = [ROUTES[9], ROUTES[10], ROUTES[11], ROUTES[15]]
SCALAR_FORMS = ('all', 'out2_all', 'relu_grad')


def route_id(r):
    return f'{r.M}x{r.N}x{r.K}-{r.ak}{r.bk}-p{r.prec}'


def skipped(r, form):
    """Both operands k-major and a row scale: the planner sends those to another route by design."""
    return bool(r.ak and r.bk and FORMS[form].rowscale)


def expected_name(r, form):
    return r.rowscale_name if (r.rowscale_name and FORMS[form].rowscale) else r.name


def cases(routes=None, forms=None):
    """(route, form name) in table order: all forms of a row are neighbours, so its inputs and fp64 product are made once."""
    return [(r, f) for r in (ROUTES if routes is None else routes) for f in (FORMS if forms is None else forms)
            if not skipped(r, f)]
