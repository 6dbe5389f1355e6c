// The product on pre-split bf16 weight planes, and both plane splitters (the fp16 planes feed PlaneOperandH of gemm_h3.hip).
#include "gemm_plan.h"

namespace rscotr {
// bf16x6 with PRE-SPLIT WEIGHTS (rscotr_gemm_f32_wplanes; scripts/lab/planes_lab.hip is the stand-alone version).
// In y = x W^T and dx = dy W the B operand is a parameter: it changes once per optimizer step, yet the kernels of gemm_bf16x6.hip split it
// into bf16 planes again in every workgroup of every launch (a 10880 x 2048 x 256 product converts W 85 times).  Here the
// planes are written ONCE per step by rscotr_gemm_split_weights, in a k-step-major layout [K / 16][Npad][3 planes][16 k]
// bf16 (Npad = N rounded up to 128, zero rows behind N), so that the B stage of a workgroup is one contiguous run of
// 96-byte rows that goes global -> VGPR -> LDS with no VALU work at all; the transposed set (planes of W^T) serves
// dx = dy W.  Only A (the activation, fp32, row-major) is split while it is staged — once per 256 (128) output columns.
// Workgroup = 512 threads = 8 wavefronts; tile 128 x 256 (wave tile 64 x 64) or 128 x 128 (wave tile 32 x 64); two LDS
// stages, one barrier per 16-k step, three register sets of prefetch (tile t + 3 is requested at the top of step t), the
// split / pack / LDS writes of tile t + 1 interleaved with the MFMAs of tile t (sched_group_barrier).  Rows past M are
// clamped loads / guarded stores, columns past N are zero planes / guarded stores: any M, N; K % 16 == 0.
// Lab (MI355X, no epilogue): 10880 x 256 x 2048 in 3 k-slices 70 us against 105 for the in-kernel split, 32768 x 384 x 96
// 26 against 47, 8192 x 768 x 192 21 against 35, 2048 x 1536 x 384 22 against 30, 4096^3 207 TFLOP/s-equivalent against 174.
constexpr int WPL_LDR = 56;  // bf16 per LDS row: 3 planes x 16 k + 8 pad (112 bytes: conflict-free 16-byte fragment reads)

struct WplRegs {
  float4 a;
  uint4 b[3];
  __device__ __forceinline__ void load(const float* a_src, const unsigned short* b_src, long a_off, long b_off, bool b_active) {
    a = *reinterpret_cast<const float4*>(a_src + a_off);
    if (b_active) {
      const uint4* s = reinterpret_cast<const uint4*>(b_src + b_off);
      b[0] = s[0]; b[1] = s[1]; b[2] = s[2];
    }
  }
  __device__ __forceinline__ void store(unsigned* a_s, unsigned* b_s, int tid, bool b_active) const {
    __bf16 x[3], y[3], z[3], w[3];
    split_planes<3>(a.x, x); split_planes<3>(a.y, y); split_planes<3>(a.z, z); split_planes<3>(a.w, w);
    unsigned* dst = a_s + ((tid >> 2) * WPL_LDR + (tid & 3) * 4) / 2;
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(dst + p * 8) = make_uint2(pack_bf16(x[p], y[p]), pack_bf16(z[p], w[p]));
    if (b_active) {
      uint4* d4 = reinterpret_cast<uint4*>(b_s + ((tid >> 1) * WPL_LDR + (tid & 1) * 24) / 2);
      d4[0] = b[0]; d4[1] = b[1]; d4[2] = b[2];
    }
  }
};

template <int BN> constexpr size_t wplanes_lds_bytes() { return 2 * (size_t)(128 + BN) * WPL_LDR * 2; }

// p.B is unused; `planes` = the pre-split B, npad = its row count per k-step.  p.tiles = tiles_m * tiles_n, p.splits k-slices
// (k-steps divided evenly), slabs as in gemm_f32_body (gemm_tiled_body.h).
template <int BN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_wplanes_kernel(
    GemmParams p, const unsigned short* __restrict__ planes, int npad) {
  constexpr int BM = 128, DEPTH = 3;
  constexpr int WNW = BN / 64, WMW = 8 / WNW, MT = BM / WMW / 32, NT = 2;
  constexpr int A_WORDS = BM * WPL_LDR / 2, B_WORDS = BN * WPL_LDR / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned wpl_lds[];
  unsigned* sA[2] = {wpl_lds, wpl_lds + A_WORDS};
  unsigned* sB[2] = {wpl_lds + 2 * A_WORDS, wpl_lds + 2 * A_WORDS + B_WORDS};
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WNW, wn = wave % WNW;
  const int tiles_n = (p.N + BN - 1) / BN;
  // grid = tiles x k-slices EXACTLY: one (128 x 256) workgroup is resident per CU, so a grid padded past 256 workgroups
  // (the XCD-run mapping of gemm_f32_body / gemm_bf16x6_body) would leave a handful of them to a second round of the whole chip
  const int idx = xcd_swizzle(blockIdx.x, gridDim.x);
  const int split = idx / p.tiles, tile = idx - split * p.tiles;
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int nk_all = p.K / 16;
  const int kt0 = (int)((long)split * nk_all / p.splits), kt1 = (int)((long)(split + 1) * nk_all / p.splits);
  const int nk = kt1 - kt0;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  WplRegs sets[DEPTH];
  const float* a_src = p.A + (long)min(m0 + (tid >> 2), p.M - 1) * p.lda + (tid & 3) * 4;  // rows past M: clamped reads
  const bool b_active = BN == 256 || tid < 256;
  const unsigned short* b_src = planes + ((long)n0 + (tid >> 1)) * 48 + (tid & 1) * 24;      // (n0 + BN <= npad)
  const long b_step = (long)npad * 48;
  const int fr = lane & 31, g = lane >> 5;
  auto mma = [&](const unsigned* a_s, const unsigned* b_s) {
    bf16x8 af[MT][3], bf[NT][3];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const unsigned* q = a_s + ((wm * (BM / WMW) + i * 32 + fr) * WPL_LDR + 8 * g) / 2;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[i][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(q + pl * 8));
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const unsigned* q = b_s + ((wn * 64 + j * 32 + fr) * WPL_LDR + 8 * g) / 2;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bf[j][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(q + pl * 8));
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {  // small terms first
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], bf[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][2], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);
      }
  };
  constexpr int U = 2 * DEPTH;
  constexpr int NMFMA = MT * NT * 6;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    const int kt = kt0 + min(d, nk - 1);
    sets[d].load(a_src, b_src, (long)kt * 16, kt * b_step, b_active);
  }
  sets[0].store(sA[0], sB[0], tid, b_active);
  __syncthreads();
  for (int t0 = 0; t0 < nk; t0 += U) {
#pragma unroll
    for (int s = 0; s < U; ++s) {
      const int t = t0 + s;
      if (t < nk) {
        {
          const int kt = kt0 + min(t + DEPTH, nk - 1);
          sets[s % DEPTH].load(a_src, b_src, (long)kt * 16, kt * b_step, b_active);
        }
        mma(sA[s & 1], sB[s & 1]);
        sets[(s + 1) % DEPTH].store(sA[(s + 1) & 1], sB[(s + 1) & 1], tid, b_active);
#pragma unroll
        for (int i = 0; i < NMFMA; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // VALU
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS write
        }
        __syncthreads();
      }
    }
  }

  if (p.splits > 1) {
    float* slab = p.slabs + (long)split * p.M * p.N;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * 64 + j * 32 + fr;
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * (BM / WMW) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
          if (m < p.M) slab[(long)m * p.N + n] = acc[i][j][r];
        }
      }
    return;
  }
  float amx = 0.f;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + wn * 64 + j * 32 + fr;
      if (n >= p.N) continue;
      const float bv = p.bias ? p.bias[n] : 0.f;
      const int mb = m0 + wm * (BM / WMW) + i * 32 + 4 * g;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = acc[i][j][4 * g4 + u] + bv;
        epilogue_rows4<true>(p, v, mb + 8 * g4, n, amx);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
}

// Split weights into the plane layout above: table rows {W, planes, N, K, ldw, npad, first block, transposed} (int64 x 8);
// transposed = 0: planes of W (N rows, reduction over K: y = x W^T); 1: planes of W^T (rows = the K columns of W, reduction
// over N: dx = dy W), N % 16 == 0 then.  One thread per (row, k-step): 16 values, one 96-byte output row.
__global__ __launch_bounds__(256) void split_weights_kernel(const int64_t* __restrict__ table, int n_entries) {
  int e = 0;
  while (e + 1 < n_entries && (long)table[(long)(e + 1) * 8 + 6] <= (long)blockIdx.x) ++e;
  const int64_t* t = table + (long)e * 8;
  const float* W = reinterpret_cast<const float*>(t[0]);
  unsigned short* planes = reinterpret_cast<unsigned short*>(t[1]);
  const int N = (int)t[2], K = (int)t[3], ldw = (int)t[4], npad = (int)t[5], tr = (int)t[7];
  const int rows = tr ? K : N, red = tr ? N : K;  // output rows, reduction length
  const long idx = ((long)blockIdx.x - t[6]) * 256 + threadIdx.x;
  const int nkt = red / 16;
  // consecutive threads take consecutive k-steps of one row (tr = 0: contiguous 64-byte reads) or consecutive rows of one
  // k-step (tr = 1: W is read along its rows)
  const int row = tr ? (int)(idx % npad) : (int)(idx / nkt);
  const int kt = tr ? (int)(idx / npad) : (int)(idx % nkt);
  if (kt >= nkt || row >= npad) return;
  float v[16];
  if (row >= rows) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
  } else if (!tr) {
    const float4* src = reinterpret_cast<const float4*>(W + (long)row * ldw + kt * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float4 x = src[q]; v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w; }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = W[(long)(kt * 16 + i) * ldw + row];
  }
  unsigned out[3][8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    __bf16 a[3], b[3];
    split_planes<3>(v[2 * q], a);
    split_planes<3>(v[2 * q + 1], b);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) out[pl][q] = pack_bf16(a[pl], b[pl]);
  }
  uint4* dst = reinterpret_cast<uint4*>(planes + ((long)kt * npad + row) * 48);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    dst[pl * 2] = make_uint4(out[pl][0], out[pl][1], out[pl][2], out[pl][3]);
    dst[pl * 2 + 1] = make_uint4(out[pl][4], out[pl][5], out[pl][6], out[pl][7]);
  }
}

// Planes of weights for PlaneOperandH (rscotr_gemm_split_weights_h3): table rows {W, planes, rows of W, cols of W, ldw, rpad,
// first block, transposed, range word of the parameter} (int64 x 9).  transposed = 0: planes of W (plane rows = rows of W,
// reduction over its columns: y = x W^T); 1: planes of W^T (plane rows = columns of W, reduction over its rows: dx = dy W).
// The reduction length is a multiple of 32; rpad = plane rows rounded up to 64, the rows past the end are zeros.  One thread per
// (k-step, plane row): 32 values in, one 128-byte record {h[32], l[32]} out; an entry takes ceil(rpad * (reduction / 32) / 256)
// blocks.  Consecutive threads take consecutive plane rows of one k-step (the records of a k-step are contiguous; transposed
// reads run along the rows of W).
__global__ __launch_bounds__(256) void split_weights_h3_kernel(const int64_t* __restrict__ table, int n_entries) {
  int e = 0;
  while (e + 1 < n_entries && (long)table[(long)(e + 1) * 9 + 6] <= (long)blockIdx.x) ++e;
  const int64_t* t = table + (long)e * 9;
  const float* W = reinterpret_cast<const float*>(t[0]);
  uint4* planes = reinterpret_cast<uint4*>(t[1]);
  const int wrows = (int)t[2], wcols = (int)t[3], ldw = (int)t[4], rpad = (int)t[5], tr = (int)t[7];
  const int rows = tr ? wcols : wrows, red = tr ? wrows : wcols;
  const int se = h3_scale_exp(amax_read(reinterpret_cast<const unsigned*>(t[8])));
  const H3Scale hs{__uint_as_float((unsigned)se << 23), __uint_as_float((unsigned)(se + 11) << 23)};
  const long idx = ((long)blockIdx.x - t[6]) * 256 + threadIdx.x;
  const int nkt = red / 32;
  const int kt = (int)(idx / rpad), row = (int)(idx % rpad);
  if (kt >= nkt) return;
  float v[32];
  if (row >= rows) {
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = 0.f;
  } else if (!tr) {
    const float4* src = reinterpret_cast<const float4*>(W + (long)row * ldw + kt * 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) { const float4 x = src[q]; v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w; }
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = W[(long)(kt * 32 + i) * ldw + row];
  }
  unsigned h[16], l[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    unsigned o[3];
    split_pair_h(v[2 * q], v[2 * q + 1], hs, o);
    h[q] = o[0]; l[q] = o[1];
  }
  uint4* dst = planes + ((long)kt * rpad + row) * 8;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    dst[q] = make_uint4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
    dst[4 + q] = make_uint4(l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3]);
  }
}

void launch_wplanes(const GemmParams& p, const GemmPlan& pl, const unsigned short* planes, int npad, hipStream_t s) {
  static const bool attr_set = [] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_wplanes_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)wplanes_lds_bytes<256>());
    hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_wplanes_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)wplanes_lds_bytes<128>());
    return true;
  }();
  (void)attr_set;
  if (pl.bn == 256) gemm_wplanes_kernel<256><<<dim3(pl.nwg), 512, wplanes_lds_bytes<256>(), s>>>(p, planes, npad);
  else gemm_wplanes_kernel<128><<<dim3(pl.nwg), 512, wplanes_lds_bytes<128>(), s>>>(p, planes, npad);
}
}  // namespace rscotr
using namespace rscotr;

// Planes of weights for rscotr_gemm_f32_wplanes (layout: gemm_wplanes_kernel).  table: device (n, 8) int64 rows {W, planes, N,
// K, ldw, npad, first block, transposed}; an entry takes ceil(npad * (reduction / 16) / 256) blocks (npad = rows of the plane
// set rounded up to 256; reduction = K, or N when transposed); total_blocks = their sum.
extern "C" int rscotr_gemm_split_weights(const int64_t* table, int n, int total_blocks, void* stream) {
  if (n < 0 || total_blocks < 0) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_split_weights: negative count");
  if (n == 0 || total_blocks == 0) return RSCOTR_OK;
  if (!table) return fail(RSCOTR_E_ARG, "rscotr_gemm_split_weights: null table");
  split_weights_kernel<<<dim3((unsigned)total_blocks), 256, 0, (hipStream_t)stream>>>(table, n);
  return check_launch("rscotr_gemm_split_weights");
}

extern "C" int rscotr_gemm_split_weights_h3(const int64_t* table, int n, int total_blocks, void* stream) {
  if (n < 0 || total_blocks < 0) return fail(RSCOTR_E_SHAPE, "rscotr_gemm_split_weights_h3: negative count");
  if (n == 0 || total_blocks == 0) return RSCOTR_OK;
  if (!table) return fail(RSCOTR_E_ARG, "rscotr_gemm_split_weights_h3: null table");
  split_weights_h3_kernel<<<dim3((unsigned)total_blocks), 256, 0, (hipStream_t)stream>>>(table, n);
  return check_launch("rscotr_gemm_split_weights_h3");
}
