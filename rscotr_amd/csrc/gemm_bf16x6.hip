#include "gemm_split_body.h"
#include "gemm_plan.h"

namespace rscotr {
template <int BM, int BN, bool AKM, bool BKM, int PIPE, bool EDGE = false>
__global__ __launch_bounds__(256) void gemm_bf16x6_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned lds[bf16x6_lds_words<BM, BN, AKM, BKM, PIPE>()];
  gemm_bf16x6_body<BM, BN, AKM, BKM, PIPE, false, EDGE>(p, blockIdx.x, gridDim.x, lds);
}

void launch_bf16x6(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
  with_split_cfg(pl, [&](auto bm, auto pipe, auto edge) {
    with_layout(pl.a_kmajor, pl.b_kmajor, [&](auto ak, auto bk) {
      constexpr int BM = decltype(bm)::value;
      gemm_bf16x6_kernel<BM, BM, decltype(ak)::value, decltype(bk)::value, decltype(pipe)::value, decltype(edge)::value><<<dim3(pl.nwg), 256, 0, s>>>(p);
    });
  });
}
}  // namespace rscotr
