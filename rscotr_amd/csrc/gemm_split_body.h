// Device body and operand stagers of gemm_bf16x6.hip, gemm_h3.hip and variants 6 / 7 of gemm_group.hip.  Conventions: gemm.hip.
#pragma once
#include "gemm_common.h"
#include <type_traits>

namespace rscotr {
// bf16x6: the fp32-ACCURATE split product (precision mode 3; scripts/lab/bf16x6_lab.hip is the stand-alone version).
// x = h + m + l with h = rne_bf16(x), m = rne_bf16(x - h), l = rne_bf16(x - h - m) — both subtractions exact in fp32, so the
// three bf16 planes carry all 24 significand bits and bf16 keeps the fp32 exponent (no range problem).  Per k-step of 16
// the product keeps the six plane pairs of order <= 2^-16 — l*h + h*l + m*m + m*h + h*m + h*h, small terms first, fp32
// accumulate (v_mfma_f32_32x32x16_bf16); what is dropped (m*l + l*m + l*l) is <= 2^-23 |a||b| per product, the rounding
// class of an fp32 FMA.  Measured against fp64 (lab, MI355X): 3.0e-7 of max|C| on M = 10880, N = 2048, K = 256 where the
// fp32 FMA chain has 4.4e-7 and the two-plane bf16x3 product 4.4e-6.  Six MFMAs of 32 cycles per 32x32x16 block against
// eight of 64 on the fp32 pipe: 2500 / 6 = 417 TFLOP/s-equivalent peak against 157.3.
// Structure: BK = 16 per stage; operands staged global -> VGPR -> (split, pack) -> LDS with the three planes of a row
// side by side (row-major source: 112-byte rows, one conflict-free 16-byte read per fragment and plane) or as k-pair
// dwords (k-major source: written as 16-byte rows, four dword reads per fragment); 128 x 128 tiles on one LDS stage with
// two barriers per k-tile (1-3 resident workgroups cover each other), 64 x 64 tiles double-buffered with one barrier.
// Interior shapes only (host-checked); split-K slabs, deferred combine, bias-gradient row sums, per-sample k scaling and
// the staged epilogue are shared with gemm_f32_body (gemm_tiled_body.h).
// The planes of TWO adjacent values as packed dwords (low half = a, high half = b): the same conversions and exact
// subtractions as split_planes, written on 2-vectors so that they compile to v_cvt_pk_bf16_f32 (two conversions and the
// pack in one instruction), one mask + one shift for the way back and v_pk_add_f32 for the two subtractions: 9 VALU
// instructions per pair against ~19 for two scalar splits + two packs (a VALU instruction occupies its SIMD's issue port
// for 4 cycles: the conversion was 41 % of the 4096^3 kernel's SIMD time next to 43 % of MFMA, profiles/r3_bf16x6_pmc.txt).
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
template <int NPL>
__device__ __forceinline__ void split_pair(float a, float b, unsigned (&out)[3]) {
  const f32x2_t x = {a, b};
  const bf16x2_t h = __builtin_convertvector(x, bf16x2_t);
  out[0] = __builtin_bit_cast(unsigned, h);
  const f32x2_t r1 = x - __builtin_convertvector(h, f32x2_t);
  const bf16x2_t m = __builtin_convertvector(r1, bf16x2_t);
  out[1] = __builtin_bit_cast(unsigned, m);
  if (NPL == 3) {
    const f32x2_t r2 = r1 - __builtin_convertvector(m, f32x2_t);
    out[2] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2_t));
  } else {
    out[2] = 0u;
  }
}

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  const f32x2_t x = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2_t));
}

// Planes of the pairs (e.x, o.x), (e.y, o.y), (e.z, o.z), (e.w, o.w) (low half = e): out[plane] = the four packed dwords.
template <int NPL>
__device__ __forceinline__ void split_rows4(const float4& e, const float4& o, uint4 (&out)[3]) {
  f32x2_t e01 = {e.x, e.y}, e23 = {e.z, e.w}, o01 = {o.x, o.y}, o23 = {o.z, o.w};
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl) {
    const unsigned h0 = cvt_pk_bf16(e01.x, o01.x), h1 = cvt_pk_bf16(e01.y, o01.y);
    const unsigned h2 = cvt_pk_bf16(e23.x, o23.x), h3 = cvt_pk_bf16(e23.y, o23.y);
    out[pl] = make_uint4(h0, h1, h2, h3);
    if (pl + 1 < NPL) {
      const f32x2_t fe01 = {__uint_as_float(h0 << 16), __uint_as_float(h1 << 16)};
      const f32x2_t fe23 = {__uint_as_float(h2 << 16), __uint_as_float(h3 << 16)};
      const f32x2_t fo01 = {__uint_as_float(h0 & 0xffff0000u), __uint_as_float(h1 & 0xffff0000u)};
      const f32x2_t fo23 = {__uint_as_float(h2 & 0xffff0000u), __uint_as_float(h3 & 0xffff0000u)};
      e01 -= fe01; e23 -= fe23; o01 -= fo01; o23 -= fo23;
    }
  }
}

// ---- fp16 split product ("h3", round 5): x 2^s = h + l 2^-11 with h = rne_f16(x 2^s), l = rne_f16((x 2^s - h) 2^11).  The
// subtraction is exact in fp32 and |x 2^s - h| <= 2^-12 |x 2^s|, so l keeps 11 of the remaining 13 bits: the two planes
// carry x to 2^-24 relative (the rounding class of fp32 itself) wherever fp16 is normal, i.e. down to 2^-26 of the tensor's
// amax with the scale of h3_scale_exp; below that the error is 2^-48 of amax absolute.  The product keeps three terms,
// h h into one accumulator and l h + h l into a second one that enters with 2^-11 at the end (fp32 accumulate; the dropped
// l l term is <= 2^-24 |a||b|): THREE v_mfma_f32_32x32x16_f16 per 16 k instead of six bf16 ones, two planes instead of three
// through the conversion and LDS.  7 VALU instructions per value pair (pk_mul, cvt_pk, 2 cvt, pk_mul, pk_fma, cvt_pk).
// (Measured and not kept, profiles/r5_h3_one_acc.txt: l UNSCALED and all three MFMAs into ONE accumulator set — 16 / 64 accumulator
// registers and one VALU instruction per value pair less, the 64 x 64 kernel at four workgroups per CU: 34.55 -> 33.86 ms per
// round with every product on it, 34.0 -> 33.7 with the forward-layout products only.  Its error is that of an fp32 FMA chain
// (4.3e-7 of max|C| against 2.5e-7 here), and elements more than 2^16 below the tensor's amax keep 11 bits only (fp16's 5-bit
// exponent; 2^27 with the scaled l).  The det step at 256^2, seed 4, then takes a ReLU gate of a decoder FFN on the other side
// — a coin toss for any fp32-class product, but outside the band tests/parity.py flips (3e-6 of the mean |pre-activation|)
// — and leaves the 1e-3 tier by 4e-3 on decoder layer 5.  Parity first: the two accumulator sets stay.)
// (f16x2_t / f16x8 / H3Scale / split_pair_h: gemm_common.h — shared with csrc/ffn.hip)
__device__ __forceinline__ void split_rows4_h(const float4& e, const float4& o, const H3Scale& k, uint4 (&out)[3]) {
  unsigned a[3], b[3], c[3], d[3];
  split_pair_h(e.x, o.x, k, a);
  split_pair_h(e.y, o.y, k, b);
  split_pair_h(e.z, o.z, k, c);
  split_pair_h(e.w, o.w, k, d);
  out[0] = make_uint4(a[0], b[0], c[0], d[0]);
  out[1] = make_uint4(a[1], b[1], c[1], d[1]);
}

template <int R, bool KM, int NPL, int SBK = 16, bool H16 = false>
struct SplitOperand {
  static_assert(!H16 || NPL == 2, "the fp16 split has two planes");
  static constexpr int LDR = SBK * NPL + 8;                         // bf16 per LDS row (row-major source): 112 / 208 bytes
  static constexpr int KP = SBK / 2;                                // k pairs per stage
  static constexpr int Q = SBK / 4;                                 // float4 per row per stage (row-major source)
  static constexpr int WORDS = KM ? NPL * KP * R : R * LDR / 2;     // dwords per stage
  static constexpr int ITEMS = KM ? KP * R / 4 : R * Q;             // float4 (pairs) per tile
  static constexpr int NV = (ITEMS + 255) / 256;
  float4 v[NV], w[NV];  // row-major: v; k-major: v = even k row, w = odd k row of a pair

  // EDGE instantiations (ragged M / N / K).  rlast: the last row a load may touch — rows - 1 of a row-major operand, rows - 4
  // of a k-major one (whose rows are read four at a time; rows % 4 == 0, host-checked): rows past it are CLAMPED reads, and
  // what they bring is multiplied into accumulator rows / columns that are never stored.  klim: the end of the reduction
  // (K % 4 == 0, host-checked): k positions past it are clamped reads replaced by ZEROS (they do enter the sums).
  template <bool EDGE = false>
  __device__ __forceinline__ void load(const float* __restrict__ P, int ld, int row0, int k0, int tid, int rlast = 0, int klim = 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      if (ITEMS % 256 == 0 || idx < ITEMS) {
        if (!KM) {
          const int row = EDGE ? min(row0 + idx / Q, rlast) : row0 + idx / Q;
          const int kk = k0 + (idx % Q) * 4;
          v[i] = *reinterpret_cast<const float4*>(P + (long)row * ld + (EDGE ? min(kk, klim - 4) : kk));
          if (EDGE && kk >= klim) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          const int kp = idx / (R / 4), r4 = (idx % (R / 4)) * 4;
          const int ka = k0 + 2 * kp, col = EDGE ? min(row0 + r4, rlast) : row0 + r4;
          if (!EDGE) {
            const float* src = P + (long)ka * ld + col;
            v[i] = *reinterpret_cast<const float4*>(src);
            w[i] = *reinterpret_cast<const float4*>(src + ld);
          } else {
            v[i] = *reinterpret_cast<const float4*>(P + (long)min(ka, klim - 1) * ld + col);
            w[i] = *reinterpret_cast<const float4*>(P + (long)min(ka + 1, klim - 1) * ld + col);
            if (ka >= klim) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ka + 1 >= klim) w[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
      }
    }
  }
  // k-major: the reads of load<EDGE, true>() as BUFFER loads.  One descriptor per read, built from uniform values in scalar
  // registers: it starts at the first k row of the read's item (k0 + 16 i + 0 | 1, for R = 128) and ends with row klim - 1, so a
  // row at or past klim is out of its range and reads as zeros — the zeros of load() without a select behind the load.  What
  // differs between threads is ONE 32-bit byte offset, the same for every read and every tile (thread_offset: the thread's k-pair
  // row inside the item and its four columns, clamped to rlast in the edge form): no 64-bit address per read in vector
  // registers.  ld < 2^26, so that the offset (< 15 rows + 1) fits 32 bits: launch_h3 sends wider operands to the one-set
  // kernel, the grouped launch's table builder (ops/deferred.py) to variant 6.
  __device__ __forceinline__ unsigned thread_offset(int ld, int row0, int tid, bool edge, int rlast) const {
    static_assert(!KM || ITEMS % 256 == 0, "whole items per thread");
    const int col = row0 + (tid % (R / 4)) * 4;
    return 4u * (unsigned)(2 * (tid / (R / 4)) * ld + (edge ? min(col, rlast) : col));
  }
  static __device__ __forceinline__ float4 load_row(const float* P, int ld, int krow, int klim, unsigned off) {
    typedef unsigned vec4u __attribute__((ext_vector_type(4)));
    const long left = 4l * ld * max(klim - krow, 0);  // bytes up to the end of row klim - 1
    const __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P + (long)krow * ld), 0,
                                                                        (int)(unsigned)min(left, 0xffffffffl), 0x00020000);
    const vec4u t = __builtin_amdgcn_raw_buffer_load_b128(d, (int)off, 0, 0);
    return make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
  }
  __device__ __forceinline__ void load_rows(const float* __restrict__ P, int ld, int k0, int klim, unsigned off) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int krow = k0 + i * (2 * 256 / (R / 4));
      v[i] = load_row(P, ld, krow, klim, off);
      w[i] = load_row(P, ld, krow + 1, klim, off);
    }
  }
  // k-major only: row k of the staged tile times ks[k / per]
  __device__ __forceinline__ void scale_k(const float* __restrict__ ks, int per, int k0, int tid, int klast = 0x7ffffffe) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      if (ITEMS % 256 == 0 || idx < ITEMS) {
        const int k = k0 + 2 * (idx / (R / 4));
        const float f0 = ks[min(k, klast) / per], f1 = ks[min(k + 1, klast) / per];  // (rows past K hold zeros: any factor)
        v[i].x *= f0; v[i].y *= f0; v[i].z *= f0; v[i].w *= f0;
        w[i].x *= f1; w[i].y *= f1; w[i].z *= f1; w[i].w *= f1;
      }
    }
  }
  // scale_k in two halves, R = 128: the factors are REQUESTED ahead and applied when the tile is staged — the same products as
  // scale_k, but no wait for the tile at the place of its request.  A wavefront stages four consecutive k rows per item (its two
  // half-waves one k pair each), so its factors are uniform: 4 NV SCALAR loads (f in scalar registers, the constant address
  // space: the vector says the same for the whole launch; their counter is not the operand tiles'), one division per item —
  // the next rows' quotients follow by counting.  wave: the wavefront's index, uniform (readfirstlane).
  __device__ __forceinline__ void scale_k_fetch(const float* __restrict__ ks, int per, int k0, int wave, int klast, float (&f)[4 * NV]) const {
    static_assert(!KM || R == 128, "two k pairs per wavefront");
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int kb = k0 + 4 * wave + i * (2 * 256 / (R / 4));
      int k = min(kb, klast), q = k / per, r = k - q * per;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kn = min(kb + j, klast);
        if (kn != k) {
          k = kn;
          if (++r == per) { r = 0; ++q; }
        }
        f[4 * i + j] = *(const __attribute__((address_space(4))) float*)(ks + q);
      }
    }
  }
  __device__ __forceinline__ void scale_k_apply(const float (&f)[4 * NV], int tid) {
    const bool hi = (tid / (R / 4)) & 1;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const float f0 = hi ? f[4 * i + 2] : f[4 * i], f1 = hi ? f[4 * i + 3] : f[4 * i + 1];
      v[i].x *= f0; v[i].y *= f0; v[i].z *= f0; v[i].w *= f0;
      w[i].x *= f1; w[i].y *= f1; w[i].z *= f1; w[i].w *= f1;
    }
  }
  // k-major only: running sums over k of the four rows this thread stages (r4 is the same for all its items: 256 is a
  // multiple of R / 4), times `f` (0 for a tile staged a second time at the end of the pipelined loop)
  __device__ __forceinline__ void accum(float4& a, int tid, float f = 1.f) const {
    static_assert(!KM || 256 % (R / 4) == 0, "row sums assume one row group per thread");
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (ITEMS % 256 == 0 || tid + i * 256 < ITEMS) {
        a.x = fmaf(f, v[i].x + w[i].x, a.x); a.y = fmaf(f, v[i].y + w[i].y, a.y);
        a.z = fmaf(f, v[i].z + w[i].z, a.z); a.w = fmaf(f, v[i].w + w[i].w, a.w);
      }
  }
  __device__ __forceinline__ void store(unsigned* S, int tid, const H3Scale& hs = H3Scale{1.f, 2048.f}) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      if (ITEMS % 256 == 0 || idx < ITEMS) {
        if (!KM) {
          const int row = idx / Q, kq = (idx % Q) * 4;
          unsigned ab[3], cd[3];
          if constexpr (H16) {
            split_pair_h(v[i].x, v[i].y, hs, ab);
            split_pair_h(v[i].z, v[i].w, hs, cd);
          } else {
            split_pair<NPL>(v[i].x, v[i].y, ab);
            split_pair<NPL>(v[i].z, v[i].w, cd);
          }
          unsigned* dst = S + (row * LDR + kq) / 2;
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
            uint2 q;
            q.x = ab[pl];
            q.y = cd[pl];
            *reinterpret_cast<uint2*>(dst + pl * (SBK / 2)) = q;
          }
        } else {
          const int kp = idx / (R / 4), r4 = (idx % (R / 4)) * 4;
          // (even k, odd k) pairs of the four rows: the conversions take one value of each row vector (v_cvt_pk_bf16_f32 has
          // two independent sources), the exact subtractions run on the rows' own register pairs (v_pk_add_f32)
          uint4 q[3];
          if constexpr (H16) split_rows4_h(v[i], w[i], hs, q);
          else split_rows4<NPL>(v[i], w[i], q);
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<uint4*>(S + (pl * KP + kp) * R + r4) = q[pl];
        }
      }
    }
  }
  // fragment of k-substep ks (16 k) of the stage
  static __device__ __forceinline__ void frag(const unsigned* S, int row, int g, int ks, bf16x8 (&f)[3]) {
    if (!KM) {
      const unsigned* q = S + (row * LDR + 16 * ks + 8 * g) / 2;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) f[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(q + pl * (SBK / 2)));
    } else {
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        const unsigned* q = S + (pl * KP + 8 * ks + 4 * g) * R + row;
        uint4 t;
        t.x = q[0]; t.y = q[R]; t.z = q[2 * R]; t.w = q[3 * R];
        f[pl] = __builtin_bit_cast(bf16x8, t);
      }
    }
  }
};

// B operand of the fp16 split product from PRE-SPLIT planes (round 5, rscotr_gemm_split_weights_h3): in y = x W^T and dx = dy W the
// B tile of a workgroup is a weight, which changes once per optimizer step, yet every one of the M / 64 row tiles of every launch
// converts it again — and the k loop of the 64 x 64 kernel is bound by exactly that conversion issue (78 VALU instructions per 6
// MFMAs and k-step, half of them B's: profiles/r5_h3_64_pmc.txt).  Plane layout [K / 32][rows padded to 64][h | l][32 k] fp16 (the
// planes of W for y = x W^T, of W^T for dx = dy W, so the kernel never sees a k-major B): the 64-row stage of a workgroup is ONE
// contiguous 8 KB run, 32 bytes per thread, written to the LDS rows of SplitOperand<R, false, 2, 32, true> as they are — no VALU
// work.  The planes carry the scale of the weight's range word at the time of the split; the consumer takes its 2^-s from the
// same word (the word only changes in the optimizer step, after which the planes are re-split).  (The same operand on the
// 128 x 128 one-stage kernels — four pieces per thread — measured nothing, 33.68 against 33.64 ms per round: those launches wait on
// memory, not on conversion issue.)
template <int R, int SBK>
struct PlaneOperandH {
  using Lay = SplitOperand<R, false, 2, SBK, true>;
  static_assert(R == 64 && SBK == 32, "one 32-byte piece per thread");
  static constexpr int WORDS = Lay::WORDS, KP = Lay::KP;
  typedef float vec4 __attribute__((ext_vector_type(4)));  // (a native vector: whole-struct copies of HIP's float4 / uint4 between
  vec4 v0, v1;                                             //  address spaces stay memcpys, and the register sets stayed in scratch)
  // P: the plane set (as const float* for the shared body), ld: its padded row count
  template <bool EDGE = false>
  __device__ __forceinline__ void load(const float* __restrict__ P, int ld, int row0, int k0, int tid, int = 0, int = 0) {
    const vec4* src = reinterpret_cast<const vec4*>(P) + ((long)(k0 / SBK) * ld + row0) * 8 + tid * 2;
    v0 = src[0];
    v1 = src[1];
  }
  __device__ __forceinline__ void store(unsigned* S, int tid, const H3Scale& = H3Scale{1.f, 2048.f}) const {
    vec4* dst = reinterpret_cast<vec4*>(S + (tid >> 2) * (Lay::LDR / 2) + (tid & 3) * 8);
    dst[0] = v0;
    dst[1] = v1;
  }
  static __device__ __forceinline__ void frag(const unsigned* S, int row, int g, int ks, bf16x8 (&f)[3]) { Lay::frag(S, row, g, ks, f); }
};

// PIPE: 0 = one LDS stage, two barriers per k-tile of 16; 1 = two LDS stages, one barrier, next tile's loads one step ahead;
// 2 = the software-pipelined loop (two LDS stages, one barrier): the loads of tile t + D are issued at the top of step t
// into the register set step t - 1 freed (D = 2 sets), and the split / pack / LDS writes of tile t + 1 are interleaved
// with the MFMAs of tile t inside the wavefront (sched_group_barrier: 1 MFMA : 4 VALU : 1 DS write) — the conversion runs in
// the shadow of the matrix pipe instead of in a phase of its own.  PIPE 2 stages 32 k per step (64 x 64 tiles: a row-major
// operand row is one whole 128-byte line per step; half as many barriers).  (A 128 x 128 form of the pipelined loop, 16 k
// per step, measured slower on every layout of the step: +0.65 ms per round.)
__device__ const float bf16x6_one = 1.f;
template <int PIPE> constexpr int bf16x6_bk() { return PIPE == 2 ? 32 : PIPE == 0 ? X6_BK0 : 16; }
constexpr int X6_D2 = 2, H3_VPM = 8, H3_DPM = 2;
template <int PIPE> constexpr int bf16x6_depth() { return PIPE == 2 ? X6_D2 : 1; }
// The one-stage loop of the 128 x 128 fp16 split body with two alternating register sets — EVERY OTHER tile two deep in flight
// as compiled today (see the loop's known shortfall) —, for the weight-gradient layout — both operands k-major: gemm_h3_128_kernel<true, true, *> and variant 7 of the grouped
// launch.  Those launches wait on memory: two workgroups of four wavefronts per CU, and with one register set a tile is requested
// one barrier and one MFMA phase before it is needed.  (The other layouts of gemm_h3_128_kernel stay on the one-set loop: with the
// row-major stager <true, false, *> and <false, true, true> do not fit 256 registers without scratch; <false, false, *> and
// <false, true, false> fit, but no launch of theirs was measured.  profiles/README.md, "two register sets".)
// REGISTERS ARE TIGHT: 246 / 248 / 249 of 256 with hipcc of ROCm 7.2, 7 - 10 to spare, held by the empty asm statements below.  A
// compiler update or an edit nearby can push the three kernels into scratch, which costs more than the loop gains: rscotr_amd/build.py
// compiles gemm_h3.hip and gemm_group.hip with the resource-usage remark and FAILS the build if one of them reports scratch.
// ONESET: the caller wants the one-set loop (a leading dimension of 2^26 or more: thread_offset is 32 bits).
template <int BM, int BN, bool AKM, bool BKM, int PIPE, bool EDGE, bool H16>
constexpr bool h3_two_tiles() { return H16 && PIPE == 0 && BM == 128 && BN == 128 && AKM && BKM; }

template <int BM, int BN, bool AKM, bool BKM, int PIPE, bool H16 = false>
constexpr int bf16x6_lds_words() {
  constexpr int NPL = H16 ? 2 : 3;
  return (PIPE ? 2 : 1) * (SplitOperand<BM, AKM, NPL, bf16x6_bk<PIPE>(), H16>::WORDS + SplitOperand<BN, BKM, NPL, bf16x6_bk<PIPE>(), H16>::WORDS);
}

// SLAB: leave the result as split-K slabs / row-sum partials also for a single k-slice (grouped launch, gemm_group.hip).
// lds: bf16x6_lds_words() dwords, 16-byte aligned.
// H16: the fp16 split product (split_pair_h above): operands scaled by powers of two from p.amax_a / p.amax_b (both
// required), three MFMAs per 16 k into two accumulator sets.
template <int BM, int BN, bool AKM, bool BKM, int PIPE, bool SLAB, bool EDGE = false, bool H16 = false, bool BPL = false, bool ONESET = false>
__device__ __forceinline__ void gemm_bf16x6_body(GemmParams& p, const int bx, const int gx, unsigned* lds) {
  constexpr bool TWO = !ONESET && h3_two_tiles<BM, BN, AKM, BKM, PIPE, EDGE, H16>();
  constexpr int NPL = H16 ? 2 : 3, SBK = bf16x6_bk<PIPE>(), D = TWO ? 2 : bf16x6_depth<PIPE>();
  constexpr int MT = BM / 64, NT = BN / 64;
  using OA = SplitOperand<BM, AKM, NPL, SBK, H16>;
  static_assert(!BPL || (H16 && !BKM && !EDGE && PIPE == 2), "B from planes: the interior pipelined fp16 kernel");
  using OB = typename std::conditional<BPL, PlaneOperandH<BN, SBK>, SplitOperand<BN, BKM, NPL, SBK, H16>>::type;
  H3Scale ha{1.f, 2048.f}, hb{1.f, 2048.f};
  float inva = 1.f, invb = 1.f;
  // The range words are REQUESTED here and reduced (h3_scales) only after the first operand tiles have been requested too:
  // the words are cold lines for this XCD's L2 — waiting for them first would put a full memory latency in front of every
  // workgroup's first tile (measured in the step: the split product's gain over the six-term one was gone).
  unsigned ra = 0u, rb = 0u;
  if constexpr (H16) {
    ra = p.amax_a[(long)(threadIdx.x & (kAmaxPlanes - 1)) * kAmaxStride];
    rb = p.amax_b[(long)(threadIdx.x & (kAmaxPlanes - 1)) * kAmaxStride];
  }
  auto h3_scales = [&]() {
    if constexpr (H16) {
      if constexpr (TWO) {  // (amax_fold_lane, common.h: the shuffle addresses do not stay in registers through the loop)
        int ln = (int)__lane_id();
        asm volatile("" : "+v"(ln));
        ra = amax_fold_lane(ra, ln); rb = amax_fold_lane(rb, ln);
      } else {
        ra = amax_fold(ra); rb = amax_fold(rb);
      }
      const int ea = h3_scale_exp(ra), eb = h3_scale_exp(rb);
      ha.sc = __uint_as_float((unsigned)ea << 23); ha.sc2 = __uint_as_float((unsigned)(ea + 11) << 23);
      hb.sc = __uint_as_float((unsigned)eb << 23); hb.sc2 = __uint_as_float((unsigned)(eb + 11) << 23);
      inva = __uint_as_float((unsigned)(254 - ea) << 23); invb = __uint_as_float((unsigned)(254 - eb) << 23);
    }
  };
  constexpr int NBUF = PIPE ? 2 : 1;
  unsigned* sA[2] = {lds, lds + (NBUF - 1) * OA::WORDS};
  unsigned* sB[2] = {lds + NBUF * OA::WORDS, lds + NBUF * OA::WORDS + (NBUF - 1) * OB::WORDS};
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // (not const: the two-tile loop derives them again behind itself)
  int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = EDGE ? (p.N + BN - 1) / BN : p.N / BN;
  const int alast = EDGE ? (AKM ? p.M - 4 : p.M - 1) : 0, blast = EDGE ? (BKM ? p.N - 4 : p.N - 1) : 0;
  int tile, split = 0;
  if (p.splits == 1) {
    tile = xcd_swizzle(bx, gx);
  } else {  // an XCD owns a run of tiles with all their splits (as gemm_f32_body, gemm_tiled_body.h)
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
  const int nk = EDGE ? (kend - kbeg + SBK - 1) / SBK : (kend - kbeg) / SBK;
  const int klast = EDGE ? p.K - 1 : 0x7ffffffe;

  f32x16 acc[MT][NT];
  f32x16 acc2[H16 ? MT : 1][H16 ? NT : 1];  // (fp16 split: the l h + h l terms, scaled by 2^11)
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[i][j][r] = 0.f;
        if constexpr (H16) acc2[i][j][r] = 0.f;
      }
  OA las[D];
  OB lbs[D];
  OA& la = las[0];
  OB& lb = lbs[0];
  const bool do_rs = AKM && p.rowsum && n0 == 0;  // bias gradient riding the dW contraction (tile column 0)
  float4 rs = make_float4(0.f, 0.f, 0.f, 0.f);
  int fr = lane & 31, g = lane >> 5;
  auto fetch = [&](int t) {
    la.template load<EDGE>(p.A, p.lda, m0, kbeg + t * SBK, tid, alast, p.K);
    lb.template load<EDGE>(p.B, p.ldb, n0, kbeg + t * SBK, tid, blast, p.K);
    if (AKM && p.kscale) la.scale_k(p.kscale, p.krows_per, kbeg + t * SBK, tid, klast);
  };
  auto stage = [&](unsigned* a_s, unsigned* b_s) {
    if (AKM && do_rs) la.accum(rs, tid);
    la.store(a_s, tid, ha);
    lb.store(b_s, tid, hb);
  };
  auto mma = [&](const unsigned* a_s, const unsigned* b_s) {
    int ra0 = wm * (BM / 2) + fr, rb0 = wn * (BN / 2) + fr;
    // (two tiles in flight: the fragment rows pass through an empty asm in every step, so that the sixteen LDS addresses of the
    // fragment reads — per operand, plane, substep and row half — are offsets of one register each inside the step and not
    // sixteen loop invariants held in registers across the loop: the second register set needs that room)
    if constexpr (TWO) asm volatile("" : "+v"(ra0), "+v"(rb0));
#pragma unroll
    for (int ks = 0; ks < SBK / 16; ++ks) {
      bf16x8 af[MT][3], bf[NT][3];
#pragma unroll
      for (int i = 0; i < MT; ++i) OA::frag(a_s, ra0 + i * 32, g, ks, af[i]);
#pragma unroll
      for (int j = 0; j < NT; ++j) OB::frag(b_s, rb0 + j * 32, g, ks, bf[j]);
      if constexpr (H16) {
        // l h, h l into the second accumulator set, h h into the first; term-major as below
#pragma unroll
        for (int tm = 0; tm < 3; ++tm)
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              const f16x8 a = __builtin_bit_cast(f16x8, af[i][tm == 0 ? 1 : 0]), b = __builtin_bit_cast(f16x8, bf[j][tm == 1 ? 1 : 0]);
              if (tm < 2) acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc2[i][j], 0, 0, 0);
              else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[i][j], 0, 0, 0);
            }
        continue;
      }
      // small terms first; term-major over the MT x NT accumulators (same sums, bit for bit): consecutive MFMAs write
      // DIFFERENT accumulators, so none waits for its predecessor's result (six back-to-back MFMAs on one accumulator are a
      // dependent chain)
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int tm = 0; tm < 6; ++tm)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][PA[tm]], bf[j][PB[tm]], acc[i][j], 0, 0, 0);
    }
  };
  if (PIPE == 2) {
    // Steady state without branches inside a step (the scheduler interleaves within one basic block): loads past the end
    // re-read the last tile, the last step stages it a second time into the idle LDS stage (its row sums times 0).
    constexpr int U = (D % 2 == 0) ? D : 2 * D;  // steps per unrolled round: register set and LDS stage indices static
    constexpr int NMFMA = MT * NT * (H16 ? 3 : 6) * (SBK / 16);
    constexpr int VPM = H16 ? H3_VPM : 4, DPM = H16 ? H3_DPM : 1;  // VALU / DS writes the scheduler places behind each MFMA
    // per-sample k scaling of a k-major A (weight gradients under DropPath / Mixup): always applied, so that a step stays
    // one basic block — without a scale vector every k reads the constant 1
    const float* ksp = (AKM && p.kscale) ? p.kscale : &bf16x6_one;
    const int ksper = (AKM && p.kscale) ? p.krows_per : 0x7fffffff;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int tt = min(d, nk - 1);
      las[d].template load<EDGE>(p.A, p.lda, m0, kbeg + tt * SBK, tid, alast, p.K);
      lbs[d].template load<EDGE>(p.B, p.ldb, n0, kbeg + tt * SBK, tid, blast, p.K);
    }
    h3_scales();
    if (AKM) las[0].scale_k(ksp, ksper, kbeg, tid, klast);
    if (AKM) las[0].accum(rs, tid);
    las[0].store(sA[0], tid, ha);
    lbs[0].store(sB[0], tid, hb);
    __syncthreads();
    for (int t0 = 0; t0 < nk; t0 += U) {
#pragma unroll
      for (int s = 0; s < U; ++s) {
        const int t = t0 + s;
        if (t < nk) {
          {  // tile t + D into the set tile t left (staged during step t - 1 / the prologue)
            const int tt = min(t + D, nk - 1);
            las[s % D].template load<EDGE>(p.A, p.lda, m0, kbeg + tt * SBK, tid, alast, p.K);
            lbs[s % D].template load<EDGE>(p.B, p.ldb, n0, kbeg + tt * SBK, tid, blast, p.K);
          }
          mma(sA[s & 1], sB[s & 1]);
          if (AKM) las[(s + 1) % D].scale_k(ksp, ksper, kbeg + min(t + 1, nk - 1) * SBK, tid, klast);
          if (AKM) las[(s + 1) % D].accum(rs, tid, t + 1 < nk ? 1.f : 0.f);
          las[(s + 1) % D].store(sA[(s + 1) & 1], tid, ha);
          lbs[(s + 1) % D].store(sB[(s + 1) & 1], tid, hb);
#pragma unroll
          for (int i = 0; i < NMFMA; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);  // VALU
            __builtin_amdgcn_sched_group_barrier(0x200, DPM, 0);  // DS write
          }
          __syncthreads();
        }
      }
    }
  } else if (PIPE) {
    fetch(0);
    h3_scales();
    stage(sA[0], sB[0]);
    if (nk > 1) fetch(1);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      const bool odd = t & 1;  // (selects, not a runtime-indexed pointer array: the accesses must stay LDS accesses)
      mma(odd ? sA[1] : sA[0], odd ? sB[1] : sB[0]);
      if (t + 1 < nk) {  // registers hold tile t+1: split / pack / write to the other stage, then fetch tile t+2
        stage(odd ? sA[0] : sA[1], odd ? sB[0] : sB[1]);
        if (t + 2 < nk) fetch(t + 2);
      }
      __syncthreads();
    }
  } else if constexpr (TWO) {
    // The one-stage loop with tile t + 2 requested before tile t + 1 is staged: two register sets that alternate (static indices:
    // two steps per round), one LDS stage, the same barriers.  Nothing READS a loaded register before the staging of its tile:
    // the zeros past K of the edge form come with the buffer loads themselves (load_rows), and the per-sample k scaling is
    // applied at staging from factors requested one step ahead (scalar loads into one set of scalar registers: scale_k_fetch) —
    // in the one-set loop below a select or a product right behind the loads makes the wavefront wait for the tile where it is
    // requested.  Values, their order into the row sums and the MFMA sequence are those of that loop, bit for bit.  Requests
    // are NOT predicated (a request under a branch leaves the set as a merge of old and new registers, which the compiler
    // resolves with copies — and waits — behind the loads): the descriptors end with the k-slice, so a request past it moves no
    // data.
    // Registers: 128 accumulators + 64 for the two sets leave 64 for everything else; the empty asm statements (mma, h3_scales,
    // behind the loop) keep loop invariants out of them that are cheaper to derive again (246 - 249 registers, no scratch).
    // Known shortfall (profiles/README.md): the register allocator still moves four registers of set 1 at the end of a round, behind
    // their loads, so the odd tiles are waited for there — one MFMA phase after their request, as in the one-set loop.
    float kf[4 * OA::NV];
    const unsigned offa = la.thread_offset(p.lda, m0, tid, EDGE, alast);
    const unsigned offb = lb.thread_offset(p.ldb, n0, tid, EDGE, blast);
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto factors = [&](int t) {
      if (p.kscale) la.scale_k_fetch(p.kscale, p.krows_per, kbeg + t * SBK, wave_u, klast, kf);
    };
    auto fetch2 = [&](auto set, int t) {
      constexpr int S = decltype(set)::value;
      // (readfirstlane: k0 is uniform anyway; behind the intrinsic the addresses are no function of the loop counter that the
      // compiler could turn into one running 64-bit pointer per read — sixteen register pairs for the two sets)
      const int k0 = __builtin_amdgcn_readfirstlane(kbeg + t * SBK);
      las[S].load_rows(p.A, p.lda, k0, kend, offa);
      lbs[S].load_rows(p.B, p.ldb, k0, kend, offb);
    };
    auto stage2 = [&](auto set) {
      constexpr int S = decltype(set)::value;
      // (the set passes through an empty asm: no use of a loaded register — the compiler pairs them up for the packed conversions
      // with moves — may be scheduled in front of this point, back into the step that requested the tile)
#pragma unroll
      for (int i = 0; i < OA::NV; ++i) {
        asm volatile("" : "+v"(las[S].v[i].x), "+v"(las[S].v[i].y), "+v"(las[S].v[i].z), "+v"(las[S].v[i].w));
        asm volatile("" : "+v"(las[S].w[i].x), "+v"(las[S].w[i].y), "+v"(las[S].w[i].z), "+v"(las[S].w[i].w));
        asm volatile("" : "+v"(lbs[S].v[i].x), "+v"(lbs[S].v[i].y), "+v"(lbs[S].v[i].z), "+v"(lbs[S].v[i].w));
        asm volatile("" : "+v"(lbs[S].w[i].x), "+v"(lbs[S].w[i].y), "+v"(lbs[S].w[i].z), "+v"(lbs[S].w[i].w));
      }
      if (p.kscale) las[S].scale_k_apply(kf, tid);
      if (do_rs) las[S].accum(rs, tid);
      las[S].store(sA[0], tid, ha);
      lbs[S].store(sB[0], tid, hb);
    };
    constexpr std::integral_constant<int, 0> s0{};
    constexpr std::integral_constant<int, 1> s1{};
    factors(0);
    fetch2(s0, 0);
    fetch2(s1, 1);
    h3_scales();
    for (int t = 0; t < nk; t += 2) {
      __syncthreads();  // the previous tile has been consumed
      stage2(s0);
      if (t + 1 < nk) factors(t + 1);
      fetch2(s0, t + 2);
      __syncthreads();
      mma(sA[0], sB[0]);
      if (t + 1 < nk) {
        __syncthreads();
        stage2(s1);
        if (t + 2 < nk) factors(t + 2);
        fetch2(s1, t + 3);
        __syncthreads();
        mma(sA[0], sB[0]);
      }
    }
  } else {
    fetch(0);
    h3_scales();
    for (int t = 0; t < nk; ++t) {
      __syncthreads();  // the previous tile has been consumed
      stage(sA[0], sB[0]);
      if (t + 1 < nk) fetch(t + 1);  // next tile's global loads: requested before the barrier, in flight under it and the MFMAs
      __syncthreads();
      mma(sA[0], sB[0]);
    }
  }

  if constexpr (TWO) {
    // what the epilogue derives from the thread index (output rows and columns, the row-sum fold's addresses) is derived AFTER the
    // loop: computed in front of it, a dozen values would sit in registers through the loop, which has none to spare
    asm volatile("" : "+v"(tid));
    lane = tid & 63; wave = tid >> 6; wm = wave >> 1; wn = wave & 1; fr = lane & 31; g = lane >> 5;
  }
  if (AKM && do_rs) {  // thread t summed rows (t % (BM/4)) * 4 .. + 3 over the k-pairs it staged: fold the 8 k-lanes
    __syncthreads();
    constexpr int KL = 256 / (BM / 4) < OA::KP ? 256 / (BM / 4) : OA::KP;  // distinct k-lanes among the threads (item i of a
    float4* red = reinterpret_cast<float4*>(lds);                            // thread has the same rows: 256 % (BM / 4) == 0)
    if (tid < KL * BM / 4) red[tid] = rs;  // [k-lane][BM / 4]
    __syncthreads();
    if (tid < BM) {
      const float* rf = reinterpret_cast<const float*>(lds);
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < KL; ++k) v += rf[k * BM + tid];
      const int m = m0 + tid;
      if (!EDGE || m < p.M) {
        if (p.splits > 1 || SLAB) p.rs_slabs[(long)split * p.M + m] = v;
        else p.rowsum[m] = p.rowsum_acc ? p.rowsum[m] + v : v;
      }
    }
  }

  if constexpr (H16) {  // C = (hh + (lh + hl) 2^-11) 2^-(sa + sb)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = fmaf(acc2[i][j][r], 0x1p-11f, acc[i][j][r]) * inva * invb;
  }
  if (p.splits > 1 || SLAB) {
    float* slab = p.slabs + (long)split * p.M * p.N;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 32 + fr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
          if (!EDGE || (m < p.M && n < p.N)) slab[(long)m * p.N + n] = acc[i][j][r];
        }
      }
    return;
  }
  if constexpr (BM == 128 && BN == 128 && !EDGE) {
    // the ReLU gate as one bit per element (ACT_RELU_BITS / ACT_RELU_GRAD_BITS, gemm_common.h): the forward product of an FFN leaves
    // 8 bytes per thread and tile next to its activation, and dH = (g W) * [h > 0] reads them back instead of the M x N activation
    // (10880 x 2048: 89 MB in 512-byte row segments at the end of every workgroup — what bounds that launch).  Host-checked: no pre /
    // residual / accumulate / row scale / second output with these codes.
    if (p.act == ACT_RELU_BITS || p.act == ACT_RELU_GRAD_BITS) {
      const bool fwd = p.act == ACT_RELU_BITS;
      const long widx = ((long)(m0 / 128) * (p.N / 128) + n0 / 128) * 256 + tid;
      unsigned long long bits = fwd ? 0ull : reinterpret_cast<const unsigned long long*>(p.aux)[widx];
      float amx = 0.f;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int n = n0 + wn * (BN / 2) + j * 32 + fr;
          const float bv = p.bias ? p.bias[n] : 0.f;
          float* crow = p.C + (long)(m0 + wm * (BM / 2) + i * 32 + 4 * g) * p.ldc + n;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int b = (i * NT + j) * 16 + r;
            float v = acc[i][j][r] + bv;
            if (fwd) {
              v = fmaxf(v, 0.f);
              bits |= (unsigned long long)(v > 0.f) << b;
            } else {
              v = ((bits >> b) & 1ull) ? v : 0.f;
            }
            crow[(long)((r & 3) + 8 * (r >> 2)) * p.ldc] = v;
            amx = fmaxf(amx, fabsf(v));
          }
        }
      if (fwd) reinterpret_cast<unsigned long long*>(p.pre)[widx] = bits;
      amax_commit(p.amax_out, amx);
      return;
    }
  }
  const bool plain = !p.pre && p.act == ACT_NONE && !p.resid && !p.accumulate && !p.rowscale && !p.C2;
  // exactly one extra tensor read by the epilogue (aux of act', residual, or old C): its 16 values per tile in one batch
  // (64 x 64 tiles only: on the 128 x 128 one-stage bf16 kernel the 16-register batch costs the third resident workgroup, and on
  // the fp16 one — measured cold, 10880 x 2048 x 256 + residual: 109.7 against 105.8 us — it buys nothing: those launches are
  // bound by the 190 MB their epilogue moves in 512-byte row segments 8 KB apart)
  // (Requesting the 16 values in the PROLOGUE instead, so that they wait in registers through the k loop, measured SLOWER in the
  // step: 34.27 against 34.11 ms per round on one box, two runs each — the in-order load counter makes the second k-step wait
  // for them, and 130 + 32 registers leave the scheduler no slack under the three-workgroup cap.)
  const bool one_extra = BM == 64 && !p.C2 &&
                         ((p.act == ACT_RELU_GRAD || p.act == ACT_GELU_GRAD) ? 1 : 0) + (p.resid ? 1 : 0) + (p.accumulate ? 1 : 0) == 1;
  // an activation (and / or the stored pre-activation) but no tensor to read: epilogue_noload16
  const bool noload = !plain && (p.act == ACT_NONE || p.act == ACT_RELU || p.act == ACT_GELU) && !p.resid && !p.accumulate &&
                      !p.rowscale && !p.C2;
  float amx = 0.f;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + wn * (BN / 2) + j * 32 + fr;
      if (EDGE && n >= p.N) continue;
      const float bv = p.bias ? p.bias[n] : 0.f;
      const int mb = m0 + wm * (BM / 2) + i * 32 + 4 * g;
      float* crow = p.C + (long)mb * p.ldc + n;
      if (one_extra) {
        epilogue_tile16<EDGE>(p, acc[i][j], bv, mb, n, amx);
        __builtin_amdgcn_sched_barrier(0);
      } else if (noload) {
        epilogue_noload16<EDGE>(p, acc[i][j], bv, mb, n, amx);
      } else if (plain) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!EDGE || mb + (r & 3) + 8 * (r >> 2) < p.M) {
            const float v = acc[i][j][r] + bv;
            crow[(long)((r & 3) + 8 * (r >> 2)) * p.ldc] = v;
            amx = fmaxf(amx, fabsf(v));
          }
      } else {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = acc[i][j][4 * g4 + u] + bv;
          epilogue_rows4<EDGE>(p, v, mb + 8 * g4, n, amx);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  amax_commit(p.amax_out, amx);
}
}  // namespace rscotr
