// MSDA forward for gfx950: msda_fwd_kernel, its launcher and the entries rscotr_msda_fwd, rscotr_msda_fused_ok,
// rscotr_msda_fwd_prep (msda_common.h: the operator and where the reference calls it).
//
// CDNA4 mapping (not a CUDA one-thread-per-channel translation):
//   * one (b, q-tile, head) per 256-thread workgroup; G = D/4 lanes hold the D channels of
//     one query as float4, so a wavefront covers 64/G queries and every tap is one 16-byte
//     load per lane = whole 128-byte lines per query (D = 32);
//   * blockIdx % H == head: with H = 8 heads and the dispatcher's round-robin over the
//     8 XCDs, each XCD's private 4 MiB L2 only ever sees ONE head's 128-byte slice of every
//     value token (680 KB per image at N = 5440), so the 16x4 tap re-reads are L2 hits;
//   * sampling locations / attention weights for the tile are staged once through LDS with
//     coalesced loads, set up once per sample and re-read as LDS broadcasts by the G lanes of a query
//     (DEDUP); a tile whose records pass 48 KB of LDS (D = 16 with L P >= 32), or element offsets past 2^31, take the
//     per-lane set-up instead;
//   * PREP: the softmax / location prologue of the attention module by the threads that stage the samples.
#include "msda_common.h"

namespace rscotr {

// PREP (rscotr_msda_fwd_prep; L * P == 16): the kernel does the element-wise prologue of the attention module itself — the softmax
// over the 16 logits of a (query, head) and the location arithmetic, by the 16 consecutive threads that stage its samples — and
// leaves loc / attn in global memory for the backward, instead of reading what msda_prep_fwd_kernel wrote a launch earlier.
struct MsdaPrepIn {
  const float* off;    // raw sampling offsets, row (b, q) at (b Nq + q) ld_off, head h at + h L P 2
  const float* logit;  // raw attention logits, row (b, q) at (b Nq + q) ld_logit, head h at + h L P
  const float* ref;    // reference points (B, Nq, ref_levels, refdim)
  const float* norm;   // (L, 2) = (W_l, H_l) for 2-d reference points
  float* loc;          // out (B, Nq, H, L, P, 2)
  float* attn;         // out (B, Nq, H, L, P)
  int ld_off, ld_logit, refdim, ref_levels;
};

template <int D, int P, bool DEDUP = true, bool PREP = false>
__global__ __launch_bounds__(256) void msda_fwd_kernel(
    const float* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ lsi, const float* __restrict__ loc,
    const float* __restrict__ attn, float* __restrict__ out, int Nk, int Nq, int H, int L,
    int ntiles, MsdaPrepIn pi = MsdaPrepIn{}) {
  static_assert(!PREP || DEDUP, "the prologue rides the record staging");
  constexpr int G = D / 4;        // lanes per (query, head)
  constexpr int QW = kWave / G;   // queries per wavefront
  constexpr int QB = 4 * QW;      // queries per workgroup
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int LP = L * P;

  const int bid = blockIdx.x;
  const int h = bid % H;
  const int t = bid / H;
  const int tile = t % ntiles;
  const int b = t / ntiles;
  const int q0 = tile * QB;
  const int tid = threadIdx.x;
  const int tok_stride = H * D;
  if constexpr (DEDUP) {
  MsdaSample* recs = reinterpret_cast<MsdaSample*>(smem);  // [QB][LP]
  // stage the tile's samples: locations + weights read in coalesced 128-byte rows, set up once, left as records
  for (int i = tid; i < QB * LP; i += 256) {
    const int r = i / LP, s_ = i - r * LP;
    const int q = q0 + r;
    MsdaSample m;
    m.aw = m.w1 = m.w2 = m.w3 = m.w4 = 0.f;
    m.e1 = m.ok = m.pad = 0;
    float2 xy = make_float2(0.f, 0.f);
    float aw_ = 0.f;
    const long e = (((long)b * Nq + q) * H + h) * LP + s_;
    const int l = s_ / P;
    if constexpr (PREP) {  // (msda_prep_fwd_kernel<16>'s arithmetic: whole 16-lane groups stay together for the shuffles)
      const bool in = q < Nq;
      const long bq = (long)b * Nq + (in ? q : 0);
      const float lg = in ? pi.logit[bq * pi.ld_logit + h * LP + s_] : -3.0e38f;
      if (in) {
        const float* rp = pi.ref + (bq * pi.ref_levels + (pi.ref_levels > 1 ? l : 0)) * pi.refdim;
        const float2 o = *reinterpret_cast<const float2*>(pi.off + bq * pi.ld_off + (h * LP + s_) * 2);
        xy = msda_location(rp, o, pi.norm, l, P, pi.refdim);
        reinterpret_cast<float2*>(pi.loc)[e] = xy;
      }
      const float mx = group_max<16>(lg);
      const float ex = in ? expf(lg - mx) : 0.f;
      const float sum = group_sum<16>(ex);
      if (in) { aw_ = ex / sum; pi.attn[e] = aw_; }
    } else if (q < Nq) {
      xy = *reinterpret_cast<const float2*>(loc + e * 2);
      aw_ = attn[e];
    }
    if (q < Nq) {
      const int Hl = (int)shapes[2 * l], Wl = (int)shapes[2 * l + 1];
      const Bilinear g = bilinear_setup(xy.x, xy.y, Hl, Wl);
      m.aw = aw_;
      m.w1 = g.hh * g.hw; m.w2 = g.hh * g.lw; m.w3 = g.lh * g.hw; m.w4 = g.lh * g.lw;
      m.e1 = ((int)lsi[l] + g.i1) * tok_stride;
      m.ok = (g.ok1 ? 1 : 0) | (g.ok2 ? 2 : 0) | (g.ok3 ? 4 : 0) | (g.ok4 ? 8 : 0);
    }
    recs[i] = m;
  }
  __syncthreads();

  const int lane = tid & 63, w = tid >> 6;
  const int r = w * QW + lane / G;
  const int sub = lane % G;
  const int q = q0 + r;
  if (q >= Nq) return;

  const float* vb = value + ((long)b * Nk * H + h) * D + sub * 4;  // + element offset of a token's channel row
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const MsdaSample* mine = recs + r * LP;
  for (int l = 0; l < L; ++l) {
    const int rowstep = (int)shapes[2 * l + 1] * tok_stride;
    float4 ra[P], rb[P];
    float4 v1[P], v2[P], v3[P], v4[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float4* rp = reinterpret_cast<const float4*>(mine + l * P + p);
      ra[p] = rp[0];
      rb[p] = rp[1];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int ok = __float_as_int(rb[p].z);
      const float* t1 = vb + __float_as_int(rb[p].y);
      v1[p] = ld4(t1, ok & 1);
      v2[p] = ld4(t1 + tok_stride, ok & 2);
      v3[p] = ld4(t1 + rowstep, ok & 4);
      v4[p] = ld4(t1 + rowstep + tok_stride, ok & 8);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float aw = ra[p].x, w1 = ra[p].y, w2 = ra[p].z, w3 = ra[p].w, w4 = rb[p].x;
      acc.x += aw * (w1 * v1[p].x + w2 * v2[p].x + w3 * v3[p].x + w4 * v4[p].x);
      acc.y += aw * (w1 * v1[p].y + w2 * v2[p].y + w3 * v3[p].y + w4 * v4[p].y);
      acc.z += aw * (w1 * v1[p].z + w2 * v2[p].z + w3 * v3[p].z + w4 * v4[p].z);
      acc.w += aw * (w1 * v1[p].w + w2 * v2[p].w + w3 * v3[p].w + w4 * v4[p].w);
    }
  }
  *reinterpret_cast<float4*>(out + (((long)b * Nq + q) * H + h) * D + sub * 4) = acc;
  } else {  // the per-lane set-up (records of a tile past 48 KB of LDS, or element offsets past 2^31)
  float* s_loc = smem;                // [QB][LP*2]
  float* s_attn = smem + QB * LP * 2;  // [QB][LP]

  // stage sampling locations + attention weights of the tile (coalesced 128-byte rows)
  for (int i = tid; i < QB * LP * 2; i += 256) {
    const int r = i / (LP * 2), c = i - r * (LP * 2);
    const int q = q0 + r;
    s_loc[i] = (q < Nq) ? loc[(((long)b * Nq + q) * H + h) * (LP * 2) + c] : 0.f;
  }
  for (int i = tid; i < QB * LP; i += 256) {
    const int r = i / LP, c = i - r * LP;
    const int q = q0 + r;
    s_attn[i] = (q < Nq) ? attn[(((long)b * Nq + q) * H + h) * LP + c] : 0.f;
  }
  __syncthreads();

  const int lane = tid & 63, w = tid >> 6;
  const int r = w * QW + lane / G;
  const int sub = lane % G;
  const int q = q0 + r;
  if (q >= Nq) return;

  const float* vb = value + ((long)b * Nk * H + h) * D + sub * 4;  // + token*H*D
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* my_loc = s_loc + r * LP * 2;
  const float* my_attn = s_attn + r * LP;

  for (int l = 0; l < L; ++l) {
    const int Hl = (int)shapes[2 * l], Wl = (int)shapes[2 * l + 1];
    const float* vl = vb + (long)lsi[l] * tok_stride;
    Bilinear g[P];
    float aw[P];
    float4 v1[P], v2[P], v3[P], v4[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float2 xy = *reinterpret_cast<const float2*>(my_loc + (l * P + p) * 2);
      aw[p] = my_attn[l * P + p];
      g[p] = bilinear_setup(xy.x, xy.y, Hl, Wl);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      v1[p] = ld4(vl + (long)g[p].i1 * tok_stride, g[p].ok1);
      v2[p] = ld4(vl + (long)g[p].i2 * tok_stride, g[p].ok2);
      v3[p] = ld4(vl + (long)g[p].i3 * tok_stride, g[p].ok3);
      v4[p] = ld4(vl + (long)g[p].i4 * tok_stride, g[p].ok4);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float w1 = g[p].hh * g[p].hw, w2 = g[p].hh * g[p].lw;
      const float w3 = g[p].lh * g[p].hw, w4 = g[p].lh * g[p].lw;
      acc.x += aw[p] * (w1 * v1[p].x + w2 * v2[p].x + w3 * v3[p].x + w4 * v4[p].x);
      acc.y += aw[p] * (w1 * v1[p].y + w2 * v2[p].y + w3 * v3[p].y + w4 * v4[p].y);
      acc.z += aw[p] * (w1 * v1[p].z + w2 * v2[p].z + w3 * v3[p].z + w4 * v4[p].z);
      acc.w += aw[p] * (w1 * v1[p].w + w2 * v2[p].w + w3 * v3[p].w + w4 * v4[p].w);
    }
  }
  *reinterpret_cast<float4*>(out + (((long)b * Nq + q) * H + h) * D + sub * 4) = acc;
  }
}

template <int D, int P>
static void launch_fwd(const float* value, const int64_t* shapes, const int64_t* lsi,
                       const float* loc, const float* attn, float* out, int B, int Nk, int Nq,
                       int H, int L, hipStream_t s, const MsdaPrepIn* prep = nullptr) {
  constexpr int QB = msda_qb(D);
  const int ntiles = (Nq + QB - 1) / QB;
  const size_t shm_rec = (size_t)QB * L * P * sizeof(MsdaSample);
  if (prep) {  // (rscotr_msda_fwd_prep checked rscotr_msda_fused_ok)
    msda_fwd_kernel<D, P, true, true><<<dim3((unsigned)((long)B * ntiles * H)), dim3(256), shm_rec, s>>>(
        value, shapes, lsi, nullptr, nullptr, out, Nk, Nq, H, L, ntiles, *prep);
    return;
  }
  if (shm_rec <= 48 * 1024 && (long)(Nk + 1) * H * D < (1l << 31)) {
    msda_fwd_kernel<D, P, true><<<dim3((unsigned)((long)B * ntiles * H)), dim3(256), shm_rec, s>>>(
        value, shapes, lsi, loc, attn, out, Nk, Nq, H, L, ntiles);
    return;
  }
  const size_t shm = (size_t)QB * L * P * 3 * sizeof(float);
  msda_fwd_kernel<D, P, false><<<dim3((unsigned)((long)B * ntiles * H)), dim3(256), shm, s>>>(
      value, shapes, lsi, loc, attn, out, Nk, Nq, H, L, ntiles);
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_msda_fwd(const float* value, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const float* loc,
                               const float* attn, float* out, int B, int Nk, int Nq, int H, int D,
                               int L, int P, void* stream) {
  if (int e = check_shape("rscotr_msda_fwd", B, Nk, Nq, H, D, L, P)) return e;
  if (B == 0 || Nq == 0) return RSCOTR_OK;  // empty query set: nothing to write
  if (!value || !spatial_shapes || !level_start_index || !loc || !attn || !out)
    return fail(RSCOTR_E_ARG, "rscotr_msda_fwd: null pointer");
  if (!aligned16(value) || !aligned16(out))
    return fail(RSCOTR_E_ALIGN, "rscotr_msda_fwd: value/out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: read value + loc + attn, write out
  ProfScope prof(PROF_MSDA_FWD, 4.0 * B * ((double)Nk * H * D + (double)Nq * H * L * P * 3 + (double)Nq * H * D), s,
                 "rscotr::msda_fwd_kernel<%d, %d>", D, P);
#define CALL(DD, PP) \
  launch_fwd<DD, PP>(value, spatial_shapes, level_start_index, loc, attn, out, B, Nk, Nq, H, L, s)
  RSCOTR_DISPATCH_DP(D, P, CALL)
#undef CALL
  return check_launch("rscotr_msda_fwd");
}

// 1 if the fused entries (rscotr_msda_fwd_prep / rscotr_msda_bwd_prep) take this geometry: 16 samples per (query, head) — the
// prologue's softmax is a 16-lane reduction of the threads that stage them —, a tile's sample records within 48 KB of LDS and
// element offsets within 2^31
extern "C" int rscotr_msda_fused_ok(int Nk, int H, int D, int L, int P) {
  if (!(D == 16 || D == 32 || D == 64) || !(P == 1 || P == 2 || P == 4 || P == 8) || L < 1 || L > MSDA_MAXL || L * P != 16) return 0;
  const int QB = msda_qb(D);
  return (size_t)QB * L * P * sizeof(MsdaSample) <= 48 * 1024 && (long)(Nk + 1) * H * D < (1l << 31);
}

extern "C" int rscotr_msda_fwd_prep(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                    const float* off, const float* logit, int ld_off, int ld_logit, const float* ref,
                                    const float* norm, int refdim, int ref_levels, float* loc, float* attn, float* out, int B,
                                    int Nk, int Nq, int H, int D, int L, int P, void* stream) {
  if (int e = check_shape("rscotr_msda_fwd_prep", B, Nk, Nq, H, D, L, P)) return e;
  if (B == 0 || Nq == 0) return RSCOTR_OK;
  if (!rscotr_msda_fused_ok(Nk, H, D, L, P))
    return fail(RSCOTR_E_SHAPE, "rscotr_msda_fwd_prep: geometry outside rscotr_msda_fused_ok (L * P = %d, D = %d)", L * P, D);
  if ((refdim != 2 && refdim != 4) || (ref_levels != 1 && ref_levels != L) || ld_off < H * L * P * 2 || (ld_off & 1) || ld_logit < H * L * P)
    return fail(RSCOTR_E_SHAPE, "rscotr_msda_fwd_prep: refdim 2 | 4, ref_levels 1 | L, ld_off >= 2 H L P (even), ld_logit >= H L P");
  if (!value || !spatial_shapes || !level_start_index || !off || !logit || !ref || !loc || !attn || !out || (refdim == 2 && !norm))
    return fail(RSCOTR_E_ARG, "rscotr_msda_fwd_prep: null pointer");
  if (!aligned16(value) || !aligned16(out) || ((uintptr_t)off & 7) || ((uintptr_t)loc & 7))
    return fail(RSCOTR_E_ALIGN, "rscotr_msda_fwd_prep: value / out 16-byte, off / loc 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  MsdaPrepIn pi{off, logit, ref, norm, loc, attn, ld_off, ld_logit, refdim, ref_levels};
  // algorithmic bytes: rscotr_msda_fwd's, with the raw offsets / logits read and loc / attn written instead of read
  ProfScope prof(PROF_MSDA_FWD, 4.0 * B * ((double)Nk * H * D + (double)Nq * H * L * P * 6 + (double)Nq * H * D), s,
                 "rscotr::msda_fwd_kernel<%d, %d>", D, P);
#define CALL(DD, PP) launch_fwd<DD, PP>(value, spatial_shapes, level_start_index, nullptr, nullptr, out, B, Nk, Nq, H, L, s, &pi)
  RSCOTR_DISPATCH_DP(D, P, CALL)
#undef CALL
  return check_launch("rscotr_msda_fwd_prep");
}
