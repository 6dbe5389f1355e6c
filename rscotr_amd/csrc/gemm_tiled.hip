// The fp32 matrix-pipe kernels (tiled: body in gemm_tiled_body.h; small; direct dW) and their launches of a GemmPlan.
#include "gemm_tiled_body.h"
#include "gemm_plan.h"
#include <mutex>
#include <set>

namespace rscotr {
// (holding the k-group instantiations — 512 / 1024 threads, 68-72 registers — to 64 registers so that two 1024-thread workgroups
// fit a CU measured nothing: 33.80 against 33.79 ms per round)
template <int BM, int BN, int WM, int WN, bool AK, bool BK_, bool EDGE, int KG>
__global__ __launch_bounds__(256 * KG) void gemm_f32_kernel(GemmParams p) {
  gemm_f32_body<BM, BN, WM, WN, AK, BK_, EDGE, KG, false>(p, blockIdx.x, gridDim.x, blockIdx.y);
}

// Low-latency kernel for the decoders' small products (M x N <= ~1M outputs, K <= 512: the per-layer Linears and
// weight gradients of the DINO / Mask2Former decoders, a few hundred launches per round).  On such shapes the tiled
// kernel (gemm_f32_body) is a chain of dependent memory round trips (k-tile -> LDS -> barrier, 4-16 times) on a fraction of the
// CUs: 11-18 us per launch for microseconds of MFMA work.  Here
//   * the output tile is 32 x 32 (4x the workgroups of a 64 x 64 tiling: M = 200 -> 56, M = 1600 -> 400);
//   * the NW wavefronts of a workgroup split K (each takes a contiguous run of 8-element "octets", <= 32 elements per
//     pass), so the reduction runs on all four SIMDs of the CU at once;
//   * MFMA operand fragments are loaded straight from global memory into registers, all loads of a pass in flight
//     together: ONE memory round trip per pass, no LDS staging, no barrier in the k loop.  A row-major operand is read
//     as float4 = 4 consecutive k per lane (lane half h takes k = 8*octet + 4*h + j for MFMA j: the k order inside an
//     octet is permuted identically for both operands, which a contraction does not see); a k-major operand as
//     128-byte coalesced rows;
//   * partial accumulators meet in LDS in fixed order (deterministic); wavefront q < 4 finishes rows 8q..8q+3 (+4h)
//     of the tile through the staged epilogue.
// Requires K % 8 == 0 and 16-byte loads legal on row-major operands (host-checked); rows past M / N are clamped reads
// whose results are never stored.
template <bool AK, bool BKM, int NW>
__global__ __launch_bounds__(64 * NW) void gemm_small_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) float gemm_smem[];  // [NW][16][64] partial accumulators
  __shared__ float s_rs[NW][32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 31, h = lane >> 5;
  const int tiles_n = (p.N + 31) >> 5;
  const int tile = blockIdx.x;
  const int m0 = (tile / tiles_n) * 32, n0 = (tile % tiles_n) * 32;
  const int ar = min(m0 + fr, p.M - 1), br = min(n0 + fr, p.N - 1);
  const int no = p.K >> 3;
  const int o0 = (int)((long)w * no / NW), o1 = (int)((long)(w + 1) * no / NW);
  const bool do_rs = AK && p.rowsum && n0 == 0;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float rs = 0.f;
  const float* Ab = AK ? p.A + ar : p.A + (long)ar * p.lda;
  const float* Bb = BKM ? p.B + br : p.B + (long)br * p.ldb;
  for (int oc = o0; oc < o1; oc += 4) {
    const int nt = min(4, o1 - oc);  // wave-uniform
    float a[4][4], b[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
        const int k = (oc + t) * 8 + h * 4;
        if (AK) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[t][j] = Ab[(long)(k + j) * p.lda];
        } else {
          const float4 q = *reinterpret_cast<const float4*>(Ab + k);
          a[t][0] = q.x; a[t][1] = q.y; a[t][2] = q.z; a[t][3] = q.w;
        }
        if (BKM) {
#pragma unroll
          for (int j = 0; j < 4; ++j) b[t][j] = Bb[(long)(k + j) * p.ldb];
        } else {
          const float4 q = *reinterpret_cast<const float4*>(Bb + k);
          b[t][0] = q.x; b[t][1] = q.y; b[t][2] = q.z; b[t][3] = q.w;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (AK && do_rs) rs += a[t][j];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][j], b[t][j], acc, 0, 0, 0);
        }
      }
    }
  }

  // partial accumulators -> LDS ([wave][register][lane]: conflict-free), fixed-order sum by wavefronts 0..3
#pragma unroll
  for (int r = 0; r < 16; ++r) gemm_smem[(w * 16 + r) * 64 + lane] = acc[r];
  if (AK && do_rs) {
    rs += __shfl_xor(rs, 32, 64);
    if (h == 0) s_rs[w][fr] = rs;
  }
  __syncthreads();
  if (AK && do_rs && threadIdx.x < 32) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < NW; ++g) v += s_rs[g][threadIdx.x];
    const int m = m0 + threadIdx.x;
    if (m < p.M) p.rowsum[m] = p.rowsum_acc ? p.rowsum[m] + v : v;
  }
  if (w >= 4) return;
  const int n = n0 + fr;
  float amx = 0.f;
  if (n < p.N) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < NW; ++g) t += gemm_smem[(g * 16 + 4 * w + u) * 64 + lane];
      v[u] = t;
    }
    if (p.bias) {
      const float bv = p.bias[n];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] += bv;
    }
    epilogue_rows4<true>(p, v, m0 + 8 * w + 4 * h, n, amx);
  }
  amax_commit(p.amax_out, amx);
}

// Weight-gradient contractions with a SMALL output and a LONG reduction (dW = dY^T X over thousands of tokens: Swin
// stage 1-2 Linears, the 256-wide projections of the encoder): both operands k-major, so an MFMA fragment of k row
// `k` is a 128-byte coalesced load — no transposition, hence no LDS staging.  One wavefront owns a (32 TM) x (32 TN)
// block of the output (TM x TN accumulator tiles in AGPRs: TM + TN fragment loads feed TM * TN MFMAs per k pair, 3x3:
// 6 loads per 9 MFMAs) and streams its k range from global memory through two register buffers of 4 k pairs (the
// loads of block i+1 are in flight under the MFMAs of block i).  The 4 wavefronts of a workgroup take quarters of
// the workgroup's k slice and fold their accumulators through one LDS buffer in fixed order (3 -> 2 -> 1 -> 0), then
// the slice's slab is written for the split-K combine (deterministic).  Against the 64x64-tile kernel on
// M = 288, N = 96, K = 32768: no tile padding (320 x 128 -> 288 x 96), 75 MB instead of 167 MB of L2 -> CU operand
// traffic, no barrier in the k loop.
template <int TM, int TN, bool KS>
__global__ __launch_bounds__(256, 2) void gemm_dw_direct_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) float gemm_smem[];  // [TM*TN*16][64] + [TM][32]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 31, h = lane >> 5;
  const int tn = (p.N + 32 * TN - 1) / (32 * TN);
  const int tile = blockIdx.x % p.tiles, split = blockIdx.x / p.tiles;
  const int m0 = (tile / tn) * 32 * TM, n0 = (tile % tn) * 32 * TN;
  const int ks0 = split * p.ksplit_len, ks1 = min(p.K, ks0 + p.ksplit_len);
  const int q = (((ks1 - ks0 + 3) >> 2) + 1) & ~1;  // even quarter
  const int k0 = min(ks1, ks0 + w * q), k1 = min(ks1, k0 + q);
  int am[TM], bn[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) am[i] = min(m0 + 32 * i + fr, p.M - 1);  // clamped reads; those rows are never stored
#pragma unroll
  for (int j = 0; j < TN; ++j) bn[j] = min(n0 + 32 * j + fr, p.N - 1);
  const bool do_rs = p.rowsum && n0 == 0;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float rs[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) rs[i] = 0.f;

  // a fragment buffer: 4 k pairs of A / B fragments + the factor of each pair's A rows (0 past the k range, else the
  // per-sample scale).  Nothing is USED at load time, so no wait is placed between the loads; no predicated loads
  // either (they compile to divergent blocks with a wait after each): k past the range reads the last valid row.
  auto load = [&](int kb, float (&a)[4][TM], float (&b)[4][TN], float (&f)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kb + 2 * u + h;
      const int kc = min(k, p.K - 1);
      const float* ap = p.A + (long)kc * p.lda;
      const float* bp = p.B + (long)kc * p.ldb;
      f[u] = KS ? p.kscale[kc / p.krows_per] : 1.f;
      if (k >= k1) f[u] = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) a[u][i] = ap[am[i]];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[u][j] = bp[bn[j]];
    }
  };
  auto compute = [&](const float (&a)[4][TM], const float (&b)[4][TN], const float (&f)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float av = a[u][i] * f[u];
        rs[i] += av;
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][j], acc[i][j], 0, 0, 0);
      }
    }
  };
  float a0[4][TM], b0[4][TN], f0[4], a1[4][TM], b1[4][TN], f1[4];
  load(k0, a0, b0, f0);
  for (int kb = k0; kb < k1; kb += 16) {
    load(kb + 8, a1, b1, f1);
    compute(a0, b0, f0);
    load(kb + 16, a0, b0, f0);
    compute(a1, b1, f1);
  }

  // fold the 4 wavefronts' accumulators through LDS: 3 -> 2 -> 1 -> 0 (fixed order)
  float* s_rs = gemm_smem + TM * TN * 16 * 64;
#pragma unroll
  for (int i = 0; i < TM; ++i) rs[i] += __shfl_xor(rs[i], 32, 64);
  for (int g = 3; g >= 1; --g) {
    if (w == g) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) gemm_smem[(((i * TN + j) * 16) + r) * 64 + lane] = acc[i][j][r];
      if (h == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) s_rs[i * 32 + fr] = rs[i];
      }
    }
    __syncthreads();
    if (w == g - 1) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += gemm_smem[(((i * TN + j) * 16) + r) * 64 + lane];
#pragma unroll
      for (int i = 0; i < TM; ++i) rs[i] += s_rs[i * 32 + fr];
    }
    __syncthreads();
  }
  if (w != 0) return;
  float* slab = p.slabs + (long)split * p.M * p.N;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + 32 * j + fr;
      if (n >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < p.M) slab[(long)m * p.N + n] = acc[i][j][r];
      }
    }
  if (do_rs && h == 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + 32 * i + fr;
      if (m < p.M) p.rs_slabs[(long)split * p.M + m] = rs[i];
    }
  }
}

template <typename Kern>
static void launch_kernel(Kern kern, dim3 grid, int threads, size_t lds, hipStream_t s, const GemmParams& p) {
  if (lds > 48 * 1024) {  // opt in to more than the default dynamic LDS once per kernel (all instantiations share
    // this function: the template parameter is the pointer TYPE, so remember the pointers themselves)
    static std::mutex mu;
    static std::set<const void*> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (raised.insert(reinterpret_cast<const void*>(kern)).second)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  kern<<<grid, threads, lds, s>>>(p);
}

// pl.kgroups > 1 only for the one-tile-per-wavefront configurations and never together with rowsum
template <int BM, int BN, int WM, int WN>
static void launch_gemm_cfg(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
  const bool interior = p.M % BM == 0 && p.N % BN == 0 && p.K % GEMM_BK == 0 && p.ksplit_len % GEMM_BK == 0 && p.vecA && p.vecB;
  auto go = [&](auto kg, auto edge) {
    with_layout(pl.a_kmajor, pl.b_kmajor, [&](auto ak, auto bk) {
      constexpr int KG = decltype(kg)::value;
      launch_kernel(gemm_f32_kernel<BM, BN, WM, WN, decltype(ak)::value, decltype(bk)::value, decltype(edge)::value, KG>,
                    dim3(pl.nwg, pl.nbatch, 1), 256 * KG, gemm_lds_bytes<BM, BN, KG>(), s, p);
    });
  };
  auto groups = [&](auto kg) { interior ? go(kg, std::false_type{}) : go(kg, std::true_type{}); };
  if constexpr ((BM / WM == 32) && (BN / WN == 32)) {
    if (pl.kgroups == 4) return groups(std::integral_constant<int, 4>{});
    if (pl.kgroups == 2) return groups(std::integral_constant<int, 2>{});
  }
  groups(std::integral_constant<int, 1>{});
}

void launch_tiled(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
  if (pl.bm == 64) launch_gemm_cfg<64, 64, 2, 2>(p, pl, s);
  else if (pl.bn == 32) launch_gemm_cfg<128, 32, 4, 1>(p, pl, s);
  else launch_gemm_cfg<128, 64, 2, 2>(p, pl, s);
}

void launch_small(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
  auto go = [&](auto nw) {
    with_layout(pl.a_kmajor, pl.b_kmajor, [&](auto ak, auto bk) {
      constexpr int NW = decltype(nw)::value;
      launch_kernel(gemm_small_kernel<decltype(ak)::value, decltype(bk)::value, NW>, dim3(pl.nwg, pl.nbatch, 1), 64 * NW,
                    (size_t)NW * 16 * 64 * sizeof(float), s, p);
    });
  };
  if (pl.nw == 16) go(std::integral_constant<int, 16>{});
  else if (pl.nw == 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 4>{});
}

void launch_dw_direct(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
  auto go = [&](auto tm, auto tn) {
    constexpr int TM = decltype(tm)::value, TN = decltype(tn)::value;
    constexpr size_t lds = (size_t)(TM * TN * 16 * 64 + TM * 32) * sizeof(float);
    if (p.kscale) launch_kernel(gemm_dw_direct_kernel<TM, TN, true>, dim3(pl.nwg), 256, lds, s, p);
    else launch_kernel(gemm_dw_direct_kernel<TM, TN, false>, dim3(pl.nwg), 256, lds, s, p);
  };
  if (pl.tm == 3) go(std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{});
  else if (pl.tm == 2) go(std::integral_constant<int, 2>{}, std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{});
}
}  // namespace rscotr
