// Exact top-K selection of one workgroup over up to 36 864 32-bit keys in LDS, shared by det_select.hip (two-stage proposal
// selection) and det_eval.hip (box decoding at test time): MSD radix select for the K-th largest key, winners collected in
// index order (ties go to the lower index), bitonic sort of the (key, ~index) pairs into torch.topk(sorted=True) order.
#pragma once
#include "common.h"

namespace rscotr {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_MAX_N = 36864;  // keys in LDS: 144 KB
constexpr int SEL_MAX_K = 1024;

__device__ __forceinline__ unsigned order_key(float v) {  // larger float <-> larger unsigned; -0 < +0; NaN sorts high
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float order_key_value(unsigned k) {  // the float of a key
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// dynamic LDS of a kernel that selects among N keys: keys[N] (padded to 4) + cand[SEL_MAX_K]
inline size_t select_lds_bytes(int N) { return (size_t)((N + 3) & ~3) * 4 + (size_t)SEL_MAX_K * 8; }

// Called by all SEL_THREADS threads of a workgroup once keys[0 .. N) are written (no barrier needed before the call).  On
// return cand[0 .. K) holds (key << 32 | ~index) of the K largest keys in descending order (equal keys: ascending index),
// cand[K .. SEL_MAX_K) zeros, and every thread has passed a barrier.  1 <= K <= min(N, SEL_MAX_K), N <= SEL_MAX_N.
__device__ __forceinline__ void select_sort_topk(const unsigned* keys, unsigned long long* cand, int N, int K) {
  __shared__ int hist[256];
  __shared__ int wsum[16][2];
  __shared__ unsigned s_prefix;
  __shared__ int s_need, s_above;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { s_prefix = 0u; s_need = K; s_above = 0; }
  __syncthreads();

  // (2) radix select from the most significant byte down: after pass p the K-th largest key is known to start with
  // s_prefix (its top 8 (p + 1) bits), `s_above` keys are larger than anything with that prefix, `s_need` = K - s_above
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix, hmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int n = tid; n < N; n += SEL_THREADS) {
      const unsigned k = keys[n];
      if ((k & hmask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {  // (256 bins: a serial walk from the top costs nothing next to the passes over N)
      int need = s_need, bin = 255;
      for (; bin > 0; --bin) {
        if (hist[bin] >= need) break;
        need -= hist[bin];
      }
      s_above += s_need - need;
      s_need = need;
      s_prefix = prefix | ((unsigned)bin << shift);
    }
    __syncthreads();
  }
  const unsigned T = s_prefix;     // the K-th largest key
  const int need_eq = s_need;      // keys == T still to take (lowest indices first)
  const int n_above = s_above;     // keys > T

  // (3) winners in index order: positions [0, n_above) for keys > T, [n_above, K) for the first need_eq keys == T
  for (int i = tid; i < SEL_MAX_K; i += SEL_THREADS) cand[i] = 0ull;  // padding sorts last (key 0 < every real key)
  __syncthreads();
  int base_gt = 0, base_eq = 0;
  for (int n0 = 0; n0 < N; n0 += SEL_THREADS) {
    const int n = n0 + tid;
    const unsigned k = n < N ? keys[n] : 0u;
    const bool gt = n < N && k > T, eq = n < N && k == T;
    const unsigned long long mg = __ballot(gt), me = __ballot(eq);
    if (lane == 0) { wsum[wave][0] = __popcll(mg); wsum[wave][1] = __popcll(me); }
    __syncthreads();
    int og = 0, oe = 0, tg = 0, te = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int a = wsum[w][0], c = wsum[w][1];
      if (w < wave) { og += a; oe += c; }
      tg += a; te += c;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (gt) cand[base_gt + og + __popcll(mg & below)] = ((unsigned long long)k << 32) | (unsigned)(0xffffffffu - (unsigned)n);
    if (eq) {
      const int r = base_eq + oe + __popcll(me & below);
      if (r < need_eq) cand[n_above + r] = ((unsigned long long)k << 32) | (unsigned)(0xffffffffu - (unsigned)n);
    }
    base_gt += tg; base_eq += te;
    __syncthreads();
  }

  // (4) bitonic sort of 1024 pairs, descending (one element per thread)
  for (int size = 2; size <= SEL_MAX_K; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int partner = tid ^ stride;
      if (partner > tid) {
        const unsigned long long a = cand[tid], c = cand[partner];
        const bool desc = (tid & size) == 0;
        if (desc ? a < c : a > c) { cand[tid] = c; cand[partner] = a; }
      }
      __syncthreads();
    }
  }
}

}  // namespace rscotr
