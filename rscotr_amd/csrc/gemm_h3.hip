#include "gemm_split_body.h"
#include "gemm_plan.h"

namespace rscotr {
// OCC: wavefronts per SIMD the register allocation is held to (1: the compiler's own choice).  The interior pipelined 64 x 64
// kernels with a row-major A take 134 / 146 registers on their own and 126 / 128 without a spill when asked: four workgroups
// per CU instead of three
template <int BM, int BN, bool AKM, bool BKM, int PIPE, bool EDGE = false, int OCC = 1, bool BPL = false>
__global__ __launch_bounds__(256, OCC) void gemm_h3_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned lds[bf16x6_lds_words<BM, BN, AKM, BKM, PIPE, true>()];
  gemm_bf16x6_body<BM, BN, AKM, BKM, PIPE, false, EDGE, true, BPL>(p, blockIdx.x, gridDim.x, lds);
}
// 128 x 128 tiles: two accumulator sets are 128 registers; held to two wavefronts per SIMD (256 registers in all) so that
// two workgroups per CU cover each other's staging phases in the one-stage loop
// ONESET: the one-set loop also where the body would alternate two register sets (both operands k-major; h3_two_tiles)
template <bool AKM, bool BKM, bool EDGE = false, bool ONESET = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_h3_128_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned lds[bf16x6_lds_words<128, 128, AKM, BKM, 0, true>()];
  gemm_bf16x6_body<128, 128, AKM, BKM, 0, false, EDGE, true, false, ONESET>(p, blockIdx.x, gridDim.x, lds);
}

void launch_h3(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
  if (pl.b_from_planes) {  // no conversion of B in the loop (p.B = the plane set, p.ldb = its padded row count)
    gemm_h3_kernel<64, 64, false, false, 2, false, 4, true><<<dim3(pl.nwg), 256, 0, s>>>(p);
    return;
  }
  with_split_cfg(pl, [&](auto bm, auto pipe, auto edge) {
    with_layout(pl.a_kmajor, pl.b_kmajor, [&](auto ak, auto bk) {
      constexpr int BM = decltype(bm)::value, PIPE = decltype(pipe)::value;
      constexpr bool EDGE = decltype(edge)::value, AK = decltype(ak)::value, BK = decltype(bk)::value;
      if constexpr (BM == 128) {
        // (the two-set loop of the k-major layout addresses a tile with 32-bit offsets: SplitOperand::thread_offset)
        if (AK && BK && (p.lda >= (1 << 26) || p.ldb >= (1 << 26))) gemm_h3_128_kernel<AK, BK, EDGE, AK && BK><<<dim3(pl.nwg), 256, 0, s>>>(p);
        else gemm_h3_128_kernel<AK, BK, EDGE><<<dim3(pl.nwg), 256, 0, s>>>(p);
      } else if (PIPE == 2 && !EDGE && !AK) {
        // (the interior pipelined 64 x 64 kernels with a row-major A: the 128-register instantiations, four workgroups per CU —
        // 33.84 against 34.00 ms per round, bit-identical results.  A plain `if`: their OCC = 1 forms stay instantiated)
        gemm_h3_kernel<64, 64, false, BK, 2, false, 4><<<dim3(pl.nwg), 256, 0, s>>>(p);
      } else {
        gemm_h3_kernel<BM, BM, AK, BK, PIPE, EDGE><<<dim3(pl.nwg), 256, 0, s>>>(p);
      }
    });
  });
}
}  // namespace rscotr
