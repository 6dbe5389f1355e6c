// The route of one product: decided once by plan_gemm (gemm.hip), launched by the family files (each __global__ template is
// instantiated in exactly one of them), reported by the host views (rscotr_gemm_f32_split_route, rscotr_gemm_relu_bits_ok).
#pragma once
#include "gemm_common.h"
#include <type_traits>

namespace rscotr {
enum { ROUTE_SMALL = 0, ROUTE_DW_DIRECT = 1, ROUTE_SPLIT = 2, ROUTE_TILED = 3, ROUTE_WPLANES = 4 };
struct GemmPlan {
  int route;
  int bm, bn;          // block tile (ROUTE_WPLANES: 128 x bn)
  int tm, tn;          // ROUTE_DW_DIRECT: the wave tile in units of 32 rows / columns
  int pipe;            // ROUTE_SPLIT: loop form of gemm_bf16x6_body (0 one LDS stage, 1 two stages, 2 software-pipelined)
  bool edge;           // ROUTE_SPLIT: ragged M / N / K -> the EDGE instantiations
  bool h3;             // ROUTE_SPLIT: the fp16 split product (both ranges given, mode on) instead of the six-term bf16 one
  bool b_from_planes;  // ROUTE_SPLIT: B comes as pre-split fp16 planes (the interior pipelined 64 x 64 fp16 kernel only)
  int a_kmajor, b_kmajor;  // layouts as the kernel (and its profile name) sees them: b_from_planes makes B row-major
  int splits, klen;    // k-slices through slabs (1: none) and their length
  int tiles;           // output tiles (GemmParams::tiles)
  int kgroups;         // ROUTE_TILED: wavefront groups per workgroup sharing the k loop (1, 2, 4)
  int nw;              // ROUTE_SMALL: wavefronts per workgroup splitting K (4, 8, 16)
  unsigned nwg, nbatch;  // grid (x, y)
};

// The two runtime layout flags as compile-time booleans: f(std::bool_constant<a_kmajor>, std::bool_constant<b_kmajor>).
template <typename F>
static inline void with_layout(int a_kmajor, int b_kmajor, F&& f) {
  if (!a_kmajor && !b_kmajor) f(std::false_type{}, std::false_type{});
  else if (!a_kmajor) f(std::false_type{}, std::true_type{});
  else if (!b_kmajor) f(std::true_type{}, std::false_type{});
  else f(std::true_type{}, std::true_type{});
}

// Tile, loop form and edge handling of a ROUTE_SPLIT plan as compile-time values: f(BM, PIPE, EDGE) as integral constants.
template <typename F>
static inline void with_split_cfg(const GemmPlan& pl, F&& f) {
  auto go = [&](auto bm, auto pipe) {
    if (pl.edge) f(bm, pipe, std::true_type{});
    else f(bm, pipe, std::false_type{});
  };
  if (pl.bm == 128) go(std::integral_constant<int, 128>{}, std::integral_constant<int, 0>{});
  else if (pl.pipe == 2) go(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 64>{}, std::integral_constant<int, 1>{});
}

void launch_small(const GemmParams& p, const GemmPlan& pl, hipStream_t s);      // gemm_tiled.hip
void launch_dw_direct(const GemmParams& p, const GemmPlan& pl, hipStream_t s);  // gemm_tiled.hip
void launch_tiled(const GemmParams& p, const GemmPlan& pl, hipStream_t s);      // gemm_tiled.hip
void launch_bf16x6(const GemmParams& p, const GemmPlan& pl, hipStream_t s);     // gemm_bf16x6.hip
void launch_h3(const GemmParams& p, const GemmPlan& pl, hipStream_t s);         // gemm_h3.hip
void launch_wplanes(const GemmParams& p, const GemmPlan& pl, const unsigned short* planes, int npad, hipStream_t s);  // gemm_planes.hip (planes: rscotr_gemm_split_weights, npad rows per k-step)
void launch_slab_sum(const float* slabs, float* out, long n4, int splits, hipStream_t s);  // gemm_reduce.hip: out[i] = sum_s slabs[s][i], n4 float4s per slab
}  // namespace rscotr
