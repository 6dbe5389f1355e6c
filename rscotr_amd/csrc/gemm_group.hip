#include "gemm_tiled_body.h"
#include "gemm_split_body.h"

namespace rscotr {
// Grouped launch of deferred weight gradients (rscotr_gemm_dw_group): MANY dW = A^T B problems with small outputs (the
// 256 x 256 projections of the encoder / decoders, the Swin stage 1-2 Linears: ~110 launches of 8-40 us per co-training
// round, each a short grid that ramps up and drains alone) run as ONE launch.  Operands are the k-major activations /
// gradients kept alive until the end of backward; every problem is cut into 64 x 64 tiles x k-slices of about equal length
// (so few slices per problem: the slab traffic of 31-slice launches goes away), slabs + row-sum partials go to the deferred
// combine (rscotr_splitk_flush), which orders problems that share a destination.
// table: device (n, 16) int64 rows {A, B, slabs, rs_slabs | 0, kscale | 0, M, N, K, lda, ldb, ksplit_len, splits,
// first workgroup OF THE BUNDLE, krows_per, 0, workgroups of the problem = tiles * splits}, n a multiple of 8: rows come in
// bundles of 8 (padded with rows of 0 workgroups) that occupy 8 * max(workgroups of the bundle's rows) consecutive ids,
// row x of a bundle taking the ids = x mod 8 (see the kernel).
constexpr size_t GROUP_LDS_BYTES = 4 * (size_t)bf16x6_lds_words<128, 128, true, true, 0>();  // 24 KB (>= the fp32 body's 17 KB)
// VAR 0: fp32 matrix pipe on 64 x 64 tiles with bounds handling (any problem); VAR 6: the six-term bf16 split product on
// 128 x 128 tiles with edge handling (M, N, K multiples of 4, 16-byte aligned operands).  Separate instantiations rather than one
// kernel with both bodies: the 128 x 128 body's registers (114 + 64 accumulators) would halve the residency of the fp32 body's
// workgroups (measured: 950 -> 1500 us for the launch).  (Variants 2 / 3 / 4 of rounds 3-4 — interior-only 128 x 128, 64 x 64
// pipelined, fp32 on 128 x 128 — lost every A/B to variant 6 and left the library in round 5.)
// VAR 7 (round 5): the fp16 split product on the 128 x 128 edge body; table column 14 = (slot of A + 1) << 32 | slot of B + 1,
// indices into `amax_base` (the value-range words of the two operands); lda, ldb < 2^26 (the two-tile loop of the body addresses
// a tile with 32-bit offsets: the table's builder, ops/deferred.py, sends wider problems to variant 6).
template <int VAR>
__device__ __forceinline__ void gemm_group_dispatch(const int64_t* __restrict__ table, int n, const unsigned* __restrict__ amax_base) {
  extern __shared__ __attribute__((aligned(16))) float gemm_smem[];
  // the problem of this workgroup.  The table comes in BUNDLES of 8 rows that share the first-workgroup column: workgroup
  // first + 8 j + x is the j-th workgroup of the bundle's row x, so that (round-robin dispatch: XCD = id % 8) ALL tiles and
  // k-slices of a problem run on one XCD and its operands are fetched into that L2 once (with the tiles of a problem
  // spread over the XCDs a 256 x 256 x 10880 problem pulled its operands from HBM three times over).  Binary search over
  // the bundles (every thread, uniform: no static LDS in front of the dynamic region the body carves with 16-byte accesses)
  int lo = 0, hi = (n >> 3) - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)table[(long)mid * 8 * 16 + 12] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int rel = (int)blockIdx.x - (int)table[(long)lo * 8 * 16 + 12];
  const int64_t* t = table + ((long)lo * 8 + (rel & 7)) * 16;
  const int jwg = rel >> 3;
  if (jwg >= (int)t[15]) return;  // (rows of a bundle differ in size; empty rows have 0 workgroups)
  GemmParams p;
  p.A = reinterpret_cast<const float*>(t[0]);
  p.B = reinterpret_cast<const float*>(t[1]);
  p.slabs = reinterpret_cast<float*>(t[2]);
  p.rs_slabs = reinterpret_cast<float*>(t[3]);
  p.kscale = reinterpret_cast<const float*>(t[4]);
  p.M = (int)t[5]; p.N = (int)t[6]; p.K = (int)t[7]; p.lda = (int)t[8]; p.ldb = (int)t[9];
  p.ksplit_len = (int)t[10]; p.splits = (int)t[11];
  p.krows_per = (int)t[13];
  p.C = nullptr; p.C2 = nullptr; p.bias = nullptr; p.aux = nullptr; p.pre = nullptr; p.resid = nullptr; p.rowscale = nullptr;
  p.ldc = p.N; p.act = ACT_NONE; p.accumulate = 0; p.rows_per = 1; p.rowsum_acc = 0;
  p.rowsum = p.rs_slabs;  // non-null = the row sums are wanted (they go to rs_slabs)
  p.vecA = ((t[0] & 15) == 0) && (p.lda % 4 == 0);
  p.vecB = ((t[1] & 15) == 0) && (p.ldb % 4 == 0);
  p.vecC = 0;
  p.nb1 = 0; p.nb2 = 1;
  if constexpr (VAR == 7) {
    p.amax_a = amax_base + (unsigned)((uint64_t)t[14] >> 32) - 1;
    p.amax_b = amax_base + (unsigned)((uint64_t)t[14] & 0xffffffffu) - 1;
  }
  p.tiles = (VAR == 6 || VAR == 7) ? ((p.M + 127) / 128) * ((p.N + 127) / 128) : ((p.M + 63) / 64) * ((p.N + 63) / 64);
  // the bodies decode (tile, k-slice) from a workgroup id laid out for XCD runs (x = id & 7 owns a run of tiles, id >> 3 =
  // slice * run + position in the run): build the id whose decoding is (tile = jwg % tiles, slice = jwg / tiles)
  const int tl_ = jwg % p.tiles, sl_ = jwg / p.tiles;
  const int q_ = p.tiles >> 3, r_ = p.tiles & 7, run_ = q_ + (r_ ? 1 : 0);
  int x_, pos_;
  if (tl_ < r_ * (q_ + 1)) { x_ = tl_ / (q_ + 1); pos_ = tl_ - x_ * (q_ + 1); }
  else { const int u_ = tl_ - r_ * (q_ + 1); x_ = r_ + u_ / q_; pos_ = u_ - (x_ - r_) * q_; }
  const int bx = 8 * (sl_ * run_ + pos_) + x_;
  const int gx = p.splits > 1 ? 8 * run_ * p.splits : p.tiles;  // (one k-slice: the single-slice tile order, result still as slab 0)
  if constexpr (VAR == 6) {
    // bf16x6 on 128 x 128 tiles with edge handling: every member with min(M, N) >= 48 — interior or ragged (Swin stage 1 / 2:
    // 96, 192, 288, 576 rows or columns); on the fp32 pipe of variant 0 the ragged ones ran at 41 TFLOP/s
    gemm_bf16x6_body<128, 128, true, true, 0, true, true>(p, bx, gx, reinterpret_cast<unsigned*>(gemm_smem));
  } else if constexpr (VAR == 7) {
    gemm_bf16x6_body<128, 128, true, true, 0, true, true, true>(p, bx, gx, reinterpret_cast<unsigned*>(gemm_smem));
  } else {
    gemm_f32_body<64, 64, 2, 2, true, true, true, 1, true>(p, bx, gx, 0);
  }
}

template <int VAR>
__global__ __launch_bounds__(256) void gemm_f32_group_kernel(const int64_t* __restrict__ table, int n) {
  gemm_group_dispatch<VAR>(table, n, nullptr);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_h3_group_kernel(
    const int64_t* __restrict__ table, int n, const unsigned* __restrict__ amax_base) {
  gemm_group_dispatch<7>(table, n, amax_base);
}
}  // namespace rscotr
using namespace rscotr;

// Grouped launch of deferred weight gradients: see gemm_f32_group_kernel.  table: device (n, 16) int64 (layout there),
// total_wgs = sum of the problems' workgroup counts; flops = sum of 2 M N K over the problems (the table lives on the device:
// the caller, who built it, states the algorithmic work of the launch for the launch-site profiler; 0 = not stated).
extern "C" int rscotr_gemm_dw_group(const int64_t* table, int n, int total_wgs, int variant, double flops,
                                    const uint32_t* amax_base, void* stream) {
  if (n < 0 || total_wgs < 0) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_dw_group: negative count");
  if (n == 0 || total_wgs == 0) return RSCOTR_OK;
  if (!table) return fail(RSCOTR_E_ARG, "rscotr_gemm_dw_group: null table");
  ProfScope prof(PROF_GEMM, flops, (hipStream_t)stream, variant == 7 ? "rscotr::gemm_h3_group_kernel" : "rscotr::gemm_f32_group_kernel<%d>", variant);  // (2 / 3 / 6: bf16x6 bodies)
  if (variant == 7) {
    if (!amax_base) return fail(RSCOTR_E_ARG, "rscotr_gemm_dw_group: variant 7 needs the value-range words (amax_base)");
    gemm_h3_group_kernel<<<dim3((unsigned)total_wgs), 256, GROUP_LDS_BYTES, (hipStream_t)stream>>>(table, n, amax_base);
  } else if (variant == 0) {
    gemm_f32_group_kernel<0><<<dim3((unsigned)total_wgs), 256, gemm_lds_bytes<64, 64, 1>(), (hipStream_t)stream>>>(table, n);
  } else if (variant == 6) {
    gemm_f32_group_kernel<6><<<dim3((unsigned)total_wgs), 256, GROUP_LDS_BYTES, (hipStream_t)stream>>>(table, n);
  } else {
    return fail(RSCOTR_E_ARG, "rscotr_gemm_dw_group: variant must be 0 (fp32 matrix pipe, 64 x 64 tiles, any problem), 6 (six-term bf16 split product, 128 x 128 tiles with edges) or 7 (fp16 split product on the same tiles)");
  }
  return check_launch("rscotr_gemm_dw_group");
}
