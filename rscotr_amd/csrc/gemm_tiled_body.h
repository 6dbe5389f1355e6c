// Device body of gemm_f32_kernel (gemm_tiled.hip) and of variant 0 of the grouped launch (gemm_group.hip).  Conventions: gemm.hip.
// Kernel shape (wave64, not a warp-shaped CUDA tiling): 256 threads = 4 wavefronts, one per SIMD;
// block tile BM x BN x 16; each wavefront owns a (BM/WM) x (BN/WN) sub-tile as MT x NT
// accumulators of 32x32 (16 VGPRs each).  Operand tiles are staged global -> VGPR -> LDS in
// K-MAJOR order ([k][m], [k][n]) so that an MFMA operand fragment (lane l: row l&31, k = l>>5) is
// one conflict-free ds_read_b32 of 32 consecutive floats per half-wave; LDS is double-buffered
// with one barrier per k-tile, the next tile's global loads are issued before the MFMAs of the
// current one.  Small grids on long reductions (the dW contractions) are split along K into
// fp32 slabs in a caller-provided workspace and combined in fixed order by a second kernel that applies
// the epilogue (deterministic: no atomics).  (Finishing a tile in the same launch by its last-arriving
// workgroup was tried: the device-scope fences it needs write back / invalidate the whole per-XCD L2 on
// every workgroup and made the step 2.5x slower.)
// A k-major A operand can also deliver its row sums over k (the bias gradient of the dW contraction).
#pragma once
#include "gemm_common.h"
#include <algorithm>

namespace rscotr {
// Load the (R rows x 16 k) operand tile at (row0, k0) into registers: NV float4 per thread.
template <int R, bool KMAJOR>
struct TileLoader {
  static constexpr int NV = (R * 4 + 255) / 256;
  float4 v[NV];

  __device__ __forceinline__ void load(const float* __restrict__ P, int ld, int rows, int kend, int row0,
                                       int k0, int vec, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < R * 4) {
        if (!KMAJOR) {
          const int row = row0 + (idx >> 2), k = k0 + (idx & 3) * 4;
          if (row < rows) {
            const float* src = P + (long)row * ld + k;
            if (vec && k + 3 < kend) {
              r = *reinterpret_cast<const float4*>(src);
            } else {
              if (k + 0 < kend) r.x = src[0];
              if (k + 1 < kend) r.y = src[1];
              if (k + 2 < kend) r.z = src[2];
              if (k + 3 < kend) r.w = src[3];
            }
          }
        } else {
          const int k = k0 + idx / (R / 4), row = row0 + (idx % (R / 4)) * 4;
          if (k < kend) {
            const float* src = P + (long)k * ld + row;
            if (vec && row + 3 < rows) {
              r = *reinterpret_cast<const float4*>(src);
            } else {
              if (row + 0 < rows) r.x = src[0];
              if (row + 1 < rows) r.y = src[1];
              if (row + 2 < rows) r.z = src[2];
              if (row + 3 < rows) r.w = src[3];
            }
          }
        }
      }
      v[i] = r;
    }
  }

  // whole tile in bounds, 16-byte loads legal
  __device__ __forceinline__ void load_fast(const float* __restrict__ P, int ld, int row0, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      if (R * 4 % 256 == 0 || idx < R * 4) {
        if (!KMAJOR)
          v[i] = *reinterpret_cast<const float4*>(P + (long)(row0 + (idx >> 2)) * ld + k0 + (idx & 3) * 4);
        else
          v[i] = *reinterpret_cast<const float4*>(P + (long)(k0 + idx / (R / 4)) * ld + row0 + (idx % (R / 4)) * 4);
      }
    }
  }

  // k-major tile: row k of the staged tile times ks[k / per]
  __device__ __forceinline__ void scale_k(const float* __restrict__ ks, int per, int k0, int kend, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      const int k = k0 + idx / (R / 4);
      if ((R * 4 % 256 == 0 || idx < R * 4) && k < kend) {
        const float f = ks[k / per];
        v[i].x *= f; v[i].y *= f; v[i].z *= f; v[i].w *= f;
      }
    }
  }

  // running sums over k of the columns this thread stages (k-major tiles: the thread's columns are fixed)
  __device__ __forceinline__ void accum(float4& a) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      a.x += v[i].x; a.y += v[i].y; a.z += v[i].z; a.w += v[i].w;
    }
  }

  // LDS image is always k-major: S[k][LD] with LD = R + 4.
  __device__ __forceinline__ void store(float* S, int tid) const {
    constexpr int LD = R + 4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      if (idx < R * 4) {
        if (!KMAJOR) {
          const int row = idx >> 2, kq = (idx & 3) * 4;
          S[(kq + 0) * LD + row] = v[i].x;
          S[(kq + 1) * LD + row] = v[i].y;
          S[(kq + 2) * LD + row] = v[i].z;
          S[(kq + 3) * LD + row] = v[i].w;
        } else {
          const int k = idx / (R / 4), c = (idx % (R / 4)) * 4;
          *reinterpret_cast<float4*>(S + k * LD + c) = v[i];
        }
      }
    }
  }
};

// EDGE = false: the host guarantees M % BM == 0, N % BN == 0, every k range a whole number of k-tiles and
// 16-byte vector loads legal on both operands — no bounds logic is compiled in (10-30 % faster on the
// step's forward shapes than the general kernel, which keeps both load paths and per-row store guards).
//
// KG > 1: KG groups of 4 wavefronts share one output tile and take the k-tiles round-robin (group g: k-tiles g,
// g+KG, ...), each with its own LDS double buffer; the partial accumulators meet in LDS at the end (fixed order).
// For launches with fewer workgroups than CUs the single-group loop runs at ~0.4 us per k-tile (LDS refill,
// barrier and fragment latency sit on the critical path with nothing to hide them): KG groups on the same CU
// interleave their chains.  No extra launch, no slabs in HBM.
//
// SLAB: always leave the result as split-K slabs / row-sum partials, also for a single k-slice (the grouped launch of
// deferred weight gradients: several problems may share a destination, the combine launch orders them).
template <int BM, int BN, int WM, int WN, bool AK, bool BK_, bool EDGE, int KG, bool SLAB>
__device__ __forceinline__ void gemm_f32_body(GemmParams& p, const int bx, const int gx, const int by) {
  static_assert(WM * WN == 4, "4 wavefronts per group");
  if (p.nb1 > 0) {  // batched: (b0, b1) = e.g. (image, head) of an attention product
    const int b01 = by / p.nb2, b2 = by - b01 * p.nb2;
    const int b0 = b01 / p.nb1, b1 = b01 - b0 * p.nb1;
    p.A += b0 * p.sA0 + b1 * p.sA1 + b2 * p.sA2;
    p.B += b0 * p.sB0 + b1 * p.sB1 + b2 * p.sB2;
    p.C += b0 * p.sC0 + b1 * p.sC1 + b2 * p.sC2;
  }
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MT = TM / 32, NT = TN / 32;
  constexpr int LDA = BM + 4, LDB = BN + 4;
  extern __shared__ __attribute__((aligned(16))) float gemm_smem[];
  const int grp = KG > 1 ? (int)(threadIdx.x >> 8) : 0;
  // (offsets, not a pointer array: a runtime-indexed array of pointers loses the LDS address space and the
  // accesses degrade to flat loads)
  // floats of LDS per k-group: two operand-tile pairs (k-major [16][LD])
  constexpr int GROUP_FLOATS = 2 * GEMM_BK * (LDA + LDB);
  constexpr int SA_FLOATS = GEMM_BK * LDA, SB_FLOATS = GEMM_BK * LDB;
  const int lds0 = grp * GROUP_FLOATS;
  float* const sA0 = gemm_smem + lds0;
  float* const sA1 = sA0 + SA_FLOATS;
  float* const sB0 = sA1 + SA_FLOATS;
  float* const sB1 = sB0 + SB_FLOATS;

  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (p.N + BN - 1) / BN;
  int tile, split = 0;
  if (p.splits == 1) {
    tile = xcd_swizzle(bx, gx);
  } else {
    // split-K: every XCD (workgroup id % 8) owns a contiguous run of tiles with ALL their splits, so the
    // slabs of a tile are written and summed through one L2; inside the run the order is split-major
    // (neighbouring workgroups = neighbouring tiles on the same k-slice share operand panels).
    const int x = bx & 7, j = bx >> 3;
    const int q = p.tiles >> 3, r = p.tiles & 7, run = q + (r ? 1 : 0);
    const int nt = q + (x < r ? 1 : 0);
    split = j / run;
    const int tl = j - split * run;
    if (tl >= nt) return;
    tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + tl;
  }
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int kbeg = split * p.ksplit_len;
  const int kend = min(p.K, kbeg + p.ksplit_len);
  const int nk = (kend - kbeg + GEMM_BK - 1) / GEMM_BK;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  TileLoader<BM, AK> la;
  TileLoader<BN, BK_> lb;
  // interior tiles (the common case) skip the per-element bounds logic
  const bool fastA = !EDGE || (p.vecA && (m0 + BM <= p.M)), fastB = !EDGE || (p.vecB && (n0 + BN <= p.N));
  auto load_tiles = [&](int k0) {
    if (!EDGE) {
      la.load_fast(p.A, p.lda, m0, k0, tid);
      lb.load_fast(p.B, p.ldb, n0, k0, tid);
    } else {
      const bool kfull = k0 + GEMM_BK <= kend;
      if (fastA && kfull) la.load_fast(p.A, p.lda, m0, k0, tid);
      else la.load(p.A, p.lda, p.M, kend, m0, k0, p.vecA, tid);
      if (fastB && kfull) lb.load_fast(p.B, p.ldb, n0, k0, tid);
      else lb.load(p.B, p.ldb, p.N, kend, n0, k0, p.vecB, tid);
    }
    if (AK && p.kscale) la.scale_k(p.kscale, p.krows_per, k0, kend, tid);
  };
  // bias gradient riding the dW contraction: workgroups of tile column 0 also sum their A tile over k
  const bool do_rs = AK && p.rowsum && n0 == 0;
  float4 rs = make_float4(0.f, 0.f, 0.f, 0.f);
  if (grp < nk) {
    load_tiles(kbeg + grp * GEMM_BK);
    if (AK && do_rs) la.accum(rs);
    la.store(sA0, tid);
    lb.store(sB0, tid);
  }
  __syncthreads();

  const int fr = lane & 31, fk = lane >> 5;
  const int nit = (nk + KG - 1) / KG;
  for (int it = 0; it < nit; ++it) {
    const int kt = it * KG + grp;
    const int cur = it & 1;
    const bool more = kt + KG < nk;
    if (more) load_tiles(kbeg + (kt + KG) * GEMM_BK);
    if (KG > 1 && kt >= nk) {  // this group has run out of k-tiles (wave-uniform)
      __syncthreads();
      continue;
    }
    {
      const float* a = (cur ? sA1 : sA0) + fk * LDA + wm * TM + fr;
      const float* b = (cur ? sB1 : sB0) + fk * LDB + wn * TN + fr;
      // operand fragments double-buffered in registers: the ds_reads of step kk+2 are in flight
      // while the MFMAs of step kk execute
      float af[2][MT], bf[2][NT];
  #pragma unroll
      for (int i = 0; i < MT; ++i) af[0][i] = a[i * 32];
  #pragma unroll
      for (int j = 0; j < NT; ++j) bf[0][j] = b[j * 32];
  #pragma unroll
      for (int kk = 0; kk < GEMM_BK; kk += 2) {
        const int c = (kk >> 1) & 1;
        if (kk + 2 < GEMM_BK) {
  #pragma unroll
          for (int i = 0; i < MT; ++i) af[c ^ 1][i] = a[(kk + 2) * LDA + i * 32];
  #pragma unroll
          for (int j = 0; j < NT; ++j) bf[c ^ 1][j] = b[(kk + 2) * LDB + j * 32];
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ahead of this step's MFMAs
  #pragma unroll
        for (int i = 0; i < MT; ++i)
  #pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][i], bf[c][j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) {
      if (AK && do_rs) la.accum(rs);
      la.store(cur ? sA0 : sA1, tid);
      lb.store(cur ? sB0 : sB1, tid);
    }
    __syncthreads();
  }

  if (AK && do_rs) {
    // thread t staged columns (t % (BM/4))*4.. of every k row it touched: fold the 256/(BM/4) k-lanes
    static_assert(!AK || 256 % (BM / 4) == 0, "row-sum fold needs fixed columns per thread");
    constexpr int CG = BM / 4, KL = 256 / CG;
    float4* red = reinterpret_cast<float4*>(sA0);  // KL x CG float4 = 4 KB <= one sA buffer (one per k-group)
    red[(tid / CG) * CG + (tid % CG)] = rs;
    __syncthreads();
    if (grp == 0 && tid < BM) {
      float v = 0.f;
#pragma unroll
      for (int g2 = 0; g2 < KG; ++g2) {
        const float* rf = gemm_smem + g2 * GROUP_FLOATS;
#pragma unroll
        for (int k = 0; k < KL; ++k) v += rf[k * BM + tid];
      }
      const int m = m0 + tid;
      if (m < p.M) {
        if (p.splits > 1 || SLAB) p.rs_slabs[(long)split * p.M + m] = v;
        else p.rowsum[m] = p.rowsum_acc ? p.rowsum[m] + v : v;
      }
    }
  }

  if (KG > 1) {
    if (AK && do_rs) __syncthreads();  // the row-sum fold above has finished reading the groups' LDS (uniform)
    // groups 1..KG-1 hand their accumulators to group 0 through LDS ([group][register][thread]: conflict-free)
    static_assert(KG == 1 || (MT == 1 && NT == 1), "in-workgroup k-groups are built for one 32x32 tile per wavefront");
    float* red = gemm_smem;
    if (grp > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((grp - 1) * 16 + r) * 256 + tid] = acc[0][0][r];
    }
    __syncthreads();
    if (grp > 0) return;
#pragma unroll
    for (int g2 = 0; g2 < KG - 1; ++g2)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][0][r] += red[(g2 * 16 + r) * 256 + tid];
  }

  // C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
  if (p.splits > 1 || SLAB) {
    float* slab = p.slabs + (long)split * p.M * p.N;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * TN + j * 32 + fr;
        if (EDGE && n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
          if (!EDGE || m < p.M) slab[(long)m * p.N + n] = acc[i][j][r];
        }
      }
    return;
  }
  const bool plain = !p.pre && p.act == ACT_NONE && !p.resid && !p.accumulate && !p.rowscale && !p.C2;
  // exactly one extra tensor read by the epilogue: its 16 values per 32 x 32 tile in one batch (epilogue_tile16; one-tile-per-
  // wavefront configurations only: the 128-row tiles keep their registers)
  const bool one_extra = MT == 1 && NT == 1 && !p.C2 &&
                         ((p.act == ACT_RELU_GRAD || p.act == ACT_GELU_GRAD) ? 1 : 0) + (p.resid ? 1 : 0) + (p.accumulate ? 1 : 0) == 1;
  // an activation (and / or the stored pre-activation) but no tensor to read: epilogue_noload16
  const bool noload = !plain && (p.act == ACT_NONE || p.act == ACT_RELU || p.act == ACT_GELU) && !p.resid && !p.accumulate &&
                      !p.rowscale && !p.C2;
  float amx = 0.f;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + wn * TN + j * 32 + fr;
      if (EDGE && n >= p.N) continue;
      const float bv = p.bias ? p.bias[n] : 0.f;
      const int mb = m0 + wm * TM + i * 32 + 4 * fk;
      float* crow = p.C + (long)mb * p.ldc + n;
      if (one_extra) {
        epilogue_tile16<EDGE>(p, acc[i][j], bv, mb, n, amx);
      } else if (noload) {
        epilogue_noload16<EDGE>(p, acc[i][j], bv, mb, n, amx);
      } else if (plain) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dm = (r & 3) + 8 * (r >> 2);
          if (!EDGE || mb + dm < p.M) {
            const float v = acc[i][j][r] + bv;
            crow[(long)dm * p.ldc] = v;
            amx = fmaxf(amx, fabsf(v));
          }
        }
      } else {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {  // rows 8 * g4 + {0..3} of this lane's 16 (C/D layout of the 32x32 MFMA)
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = acc[i][j][4 * g4 + u] + bv;
          epilogue_rows4<EDGE>(p, v, mb + 8 * g4, n, amx);
          __builtin_amdgcn_sched_barrier(0);  // keep the next group's loads from being hoisted across (registers)
        }
      }
    }
  amax_commit(p.amax_out, amx);
}

template <int BM, int BN, int KG>
constexpr size_t gemm_lds_bytes() {
  return sizeof(float) * std::max<size_t>((size_t)KG * (2 * GEMM_BK * (BM + 4 + BN + 4)), KG > 1 ? (size_t)(KG - 1) * 16 * 256 : 0);
}
}  // namespace rscotr
