// Class logits of the seg head's scheme 1 as one skinny product over the mask features (gfx950).
//
// Replaces models/multi/seg_head/mask2former_head.py:118-125 for the LAST prediction (the only one supervised or returned):
//   mask_pred = einsum('bqd,bdhw->bqhw', mask_embed(d), mask_feature)      (B,Q,h,w)   Q = 100
//   seg_mask  = einsum('bqc,bqhw->bchw', cls_pred, mask_pred)              (B,K,h,w)   K = num_classes + 1
// re-associated: with e = mask_embed(d) (B,Q,D) and the mask features in token layout mf (B,P,D), P = h*w,
//   seg[b,k,p] = sum_d M[b,k,d] mf[b,p,d],     M[b,k,d] = sum_q cls[b,q,k] e[b,q,d]       (the "mix", K*D floats per image)
// so the (B,Q,P) mask logits — 13 MB at 2 x 100 x 128^2 — are never formed and the Q = 100 product with its two backward
// products is gone.  What is left has K <= 32 output rows per pixel: far too skinny for the MFMA tiles, and bound by the one
// pass over mf (33.5 MB at 2 x 128^2 x 256).  Forward reads mf once; backward reads mf once and writes dmf once:
//   dmf[b,p,d] = sum_k g[b,k,p] M[b,k,d]        dM[b,k,d] = sum_p g[b,k,p] mf[b,p,d]
//   de[b,q,d]  = sum_k cls[b,q,k] dM[b,k,d]     dcls[b,q,k] = sum_d e[b,q,d] dM[b,k,d]
// Every sum runs in a fixed order (no atomics): two calls are bit-equal.
#include "common.h"

#include <algorithm>

namespace rscotr {

constexpr int SMX_MAX_K = 32;       // class channels
constexpr int SMX_MAX_D = 256;      // feature channels: 64, 128 or 256 (a lane owns whole float4s of a row)
constexpr int SMX_FWD_WG = 1024;    // forward grid cap (all images together); 256 threads, SMX_FWD_ROWS pixels per trip
constexpr int SMX_FWD_ROWS = 32;
constexpr int SMX_BWD_WG = 512;     // backward grid cap = partial dM slabs in the workspace; 512 threads
constexpr int SMX_BWD_U = 2;        // pixel rows a lane group has in flight (one where K > 16: the registers hold dM)

// M[b,k,:] = sum_q cls[b,q,k] * e[b,q,:].  grid (K, B), 256 threads = D / 4 lanes with one float4 of the row each x NS slices of
// the queries (q = slice, slice + NS, ...: a single thread walking all Q rows waits out Q dependent loads); the slices meet in
// slice order.
__global__ __launch_bounds__(256) void seg_mix_m_kernel(const float* __restrict__ cls, const float* __restrict__ e,
                                                        float* __restrict__ mix, int Q, int K, int D) {
  __shared__ float4 red[256];
  const int k = blockIdx.x, b = blockIdx.y, lpr = D >> 2, ns = 256 / lpr;
  const int dl = threadIdx.x % lpr, qs = threadIdx.x / lpr;
  const float* c = cls + (long)b * Q * K + k;
  const float4* er = reinterpret_cast<const float4*>(e) + (long)b * Q * lpr + dl;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int q = qs; q < Q; q += ns) {
    const float cv = c[(long)q * K];
    const float4 v = er[(long)q * lpr];
    a.x = fmaf(cv, v.x, a.x); a.y = fmaf(cv, v.y, a.y); a.z = fmaf(cv, v.z, a.z); a.w = fmaf(cv, v.w, a.w);
  }
  red[threadIdx.x] = a;  // [slice][lane]
  __syncthreads();
  if (qs == 0) {
    for (int s = 1; s < ns; ++s) {
      const float4 t = red[s * lpr + dl];
      a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
    }
    reinterpret_cast<float4*>(mix)[((long)b * K + k) * lpr + dl] = a;
  }
}

// Forward: 16 lanes per pixel row, CH = D / 64 float4s each (chunk j of lane l = floats 4 * (l + 16 j) ..: every load
// instruction covers four rows with one contiguous 256-byte segment each), four rows per wavefront, two row sets in flight.  M
// sits in LDS (the four lane groups read the same 256 bytes: a broadcast) and is read once per k for both row sets; the 16
// partial dots of a row meet by a butterfly, so every lane of the group holds the sum and lane k % 16 stores it.
template <int CH>
__global__ __launch_bounds__(256) void seg_mix_fwd_kernel(const float* __restrict__ mf, const float* __restrict__ mix,
                                                          float* __restrict__ seg, int K, int P) {
  constexpr int D4 = 16 * CH;  // float4s per row
  extern __shared__ __attribute__((aligned(16))) float smx_smem[];
  float4* sM = reinterpret_cast<float4*>(smx_smem);  // [K][D4]
  const int b = blockIdx.y, tid = threadIdx.x;
  const float4* mb = reinterpret_cast<const float4*>(mix) + (long)b * K * D4;
  for (int i = tid; i < K * D4; i += 256) sM[i] = mb[i];
  __syncthreads();
  const int gl = tid & 15, r = tid >> 4;  // lane in its group, row of the workgroup's set (0 .. 15)
  const float4* mfb = reinterpret_cast<const float4*>(mf) + (long)b * P * D4;
  float* sb = seg + (long)b * K * P;
  for (long p0 = (long)blockIdx.x * SMX_FWD_ROWS; p0 < P; p0 += (long)gridDim.x * SMX_FWD_ROWS) {
    float4 x[2][CH];
    long p[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      p[u] = p0 + u * 16 + r;
      const float4* row = mfb + (p[u] < P ? p[u] : (long)P - 1) * D4 + gl;  // (a row past the end reads the last one and stores nothing)
#pragma unroll
      for (int j = 0; j < CH; ++j) x[u][j] = row[16 * j];
    }
    for (int k = 0; k < K; ++k) {
      float s[2] = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float4 m = sM[k * D4 + gl + 16 * j];
#pragma unroll
        for (int u = 0; u < 2; ++u)
          s[u] = fmaf(m.w, x[u][j].w, fmaf(m.z, x[u][j].z, fmaf(m.y, x[u][j].y, fmaf(m.x, x[u][j].x, s[u]))));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float t = group_sum<16>(s[u]);
        if (gl == (k & 15) && p[u] < P) sb[(long)k * P + p[u]] = t;
      }
    }
  }
}

// Backward, the pass over mf: LPR = D / 4 lanes per pixel row, one float4 of the row each, so a lane's slice of dmf needs no
// other lane, and its slice of dM[k] — acc[k], KT >= K registers x 4 — collects the pixels the lane visits with no cross-lane
// step at all.  8 wavefronts x (64 / LPR) lane groups, U rows in flight per group.  The K upstream gradients of a pixel
// are loaded by every lane of the group (one address per instruction: one request), unconditionally from a clamped channel so
// that all of them are in flight together.  At the end the groups add their acc into one LDS slab in group order and the slab
// goes to the workgroup's slot of `part` (folded by seg_mix_fold_kernel).  dmf == nullptr / part == nullptr: that half is off.
template <int LPR, int KT, int U>
__global__ __launch_bounds__(512) void seg_mix_bwd_kernel(const float* __restrict__ g, const float* __restrict__ mf,
                                                          const float* __restrict__ mix, float* __restrict__ dmf,
                                                          float* __restrict__ part, int K, int P) {
  constexpr int NG = 512 / LPR;  // lane groups of the workgroup
  extern __shared__ __attribute__((aligned(16))) float smx_smem[];
  float4* sM = reinterpret_cast<float4*>(smx_smem);  // [K][LPR]: M of this image, then the dM slab
  const int b = blockIdx.y, tid = threadIdx.x;
  const int gl = tid % LPR, grp = tid / LPR;
  if (dmf) {
    const float4* mb = reinterpret_cast<const float4*>(mix) + (long)b * K * LPR;
    for (int i = tid; i < K * LPR; i += 512) sM[i] = mb[i];
  }
  __syncthreads();
  const float4* mfb = reinterpret_cast<const float4*>(mf) + (long)b * P * LPR;
  float4* db = reinterpret_cast<float4*>(dmf) + (long)b * P * LPR;
  const float* gb = g + (long)b * K * P;
  float4 acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long p0 = (long)blockIdx.x * (NG * U); p0 < P; p0 += (long)gridDim.x * (NG * U)) {
    float4 x[U];
    float gv[U][KT];
    long p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      p[u] = p0 + u * NG + grp;
      const long pc = p[u] < P ? p[u] : (long)P - 1;
      x[u] = mfb[pc * LPR + gl];
#pragma unroll
      for (int k = 0; k < KT; ++k) gv[u][k] = gb[(long)(k < K ? k : K - 1) * P + pc];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (p[u] >= P) continue;  // (uniform over the lane group)
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        if (k < K) {  // (uniform)
          const float gk = gv[u][k];
          if (dmf) {
            const float4 m = sM[k * LPR + gl];
            o.x = fmaf(gk, m.x, o.x); o.y = fmaf(gk, m.y, o.y); o.z = fmaf(gk, m.z, o.z); o.w = fmaf(gk, m.w, o.w);
          }
          acc[k].x = fmaf(gk, x[u].x, acc[k].x); acc[k].y = fmaf(gk, x[u].y, acc[k].y);
          acc[k].z = fmaf(gk, x[u].z, acc[k].z); acc[k].w = fmaf(gk, x[u].w, acc[k].w);
        }
      }
      if (dmf) db[p[u] * LPR + gl] = o;
    }
  }
  if (!part) return;
  for (int w = 0; w < NG; ++w) {  // the groups in order: a fixed summation order, one slab of LDS
    __syncthreads();
    if (grp == w) {
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        if (k < K) {
          float4 t = acc[k];
          if (w > 0) {
            const float4 s = sM[k * LPR + gl];
            t.x += s.x; t.y += s.y; t.z += s.z; t.w += s.w;
          }
          sM[k * LPR + gl] = t;
        }
      }
    }
  }
  __syncthreads();
  float4* out = reinterpret_cast<float4*>(part) + ((long)b * gridDim.x + blockIdx.x) * K * LPR;
  for (int i = tid; i < K * LPR; i += 512) out[i] = sM[i];
}

// dM[b,k,d] = sum over the nwg workgroup slabs of image b.  16 elements x 16 slices of the slabs per workgroup (slab = slice,
// slice + 16, ...: 16 independent loads per thread instead of nwg dependent ones); the slices meet in slice order.
__global__ __launch_bounds__(256) void seg_mix_fold_kernel(const float* __restrict__ part, float* __restrict__ dmix, int nwg,
                                                           int KD, long total) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const long i = (long)blockIdx.x * 16 + el;
  float a = 0.f;
  if (i < total) {
    const float* src = part + (i / KD) * nwg * KD + i % KD;
#pragma unroll 4
    for (int w = sl; w < nwg; w += 16) a += src[(long)w * KD];
  }
  red[sl][el] = a;
  __syncthreads();
  if (sl == 0 && i < total) {
    float t = red[0][el];
    for (int s = 1; s < 16; ++s) t += red[s][el];
    dmix[i] = t;
  }
}

// de[b,q,:] = sum_k cls[b,q,k] dM[b,k,:] (k ascending) and dcls[b,q,k] = sum_d e[b,q,d] dM[b,k,d] (wavefront butterfly, then the
// wavefronts in order).  grid (Q, B), D threads; either output may be null.
__global__ __launch_bounds__(256) void seg_mix_qgrad_kernel(const float* __restrict__ cls, const float* __restrict__ e,
                                                            const float* __restrict__ dmix, float* __restrict__ de,
                                                            float* __restrict__ dcls, int Q, int K, int D) {
  const int q = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const float* c = cls + ((long)b * Q + q) * K;
  const float* dm = dmix + (long)b * K * D + d;
  if (de) {
    float a = 0.f;
    for (int k = 0; k < K; ++k) a = fmaf(c[k], dm[(long)k * D], a);
    de[((long)b * Q + q) * D + d] = a;
  }
  if (!dcls) return;
  __shared__ float red[4][SMX_MAX_K];
  const float ev = e[((long)b * Q + q) * D + d];
  const int lane = d & 63, wv = d >> 6, nw = D >> 6;
  for (int k = 0; k < K; ++k) {
    const float t = wave_sum(ev * dm[(long)k * D]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (d < K) {
    float a = red[0][d];
    for (int w = 1; w < nw; ++w) a += red[w][d];
    dcls[((long)b * Q + q) * K + d] = a;
  }
}

static int smx_shape_ok(int B, int Q, int K, int D, int P) {
  return B >= 0 && B <= SMX_BWD_WG && Q >= 1 && K >= 1 && K <= SMX_MAX_K && P >= 1 && (D == 64 || D == 128 || D == 256);
}

// rows of one image a backward workgroup takes per trip
static int smx_bwd_rows(int K, int D) { return (512 / (D / 4)) * (K <= 16 ? SMX_BWD_U : 1); }

template <int LPR>
static void smx_launch_bwd(int K, dim3 grid, size_t lds, hipStream_t s, const float* g, const float* mf, const float* mix,
                           float* dmf, float* part, int P) {
  if (K <= 8) seg_mix_bwd_kernel<LPR, 8, SMX_BWD_U><<<grid, 512, lds, s>>>(g, mf, mix, dmf, part, K, P);
  else if (K <= 16) seg_mix_bwd_kernel<LPR, 16, SMX_BWD_U><<<grid, 512, lds, s>>>(g, mf, mix, dmf, part, K, P);
  else seg_mix_bwd_kernel<LPR, 32, 1><<<grid, 512, lds, s>>>(g, mf, mix, dmf, part, K, P);
}

}  // namespace rscotr

using namespace rscotr;

// the backward's partial dM slabs: one of K * D floats per workgroup
extern "C" int64_t rscotr_seg_mix_workspace(void) { return (int64_t)SMX_BWD_WG * SMX_MAX_K * SMX_MAX_D * 4; }

extern "C" int rscotr_seg_mix_fwd(const float* cls, const float* e, const float* mf, float* mix, float* seg, int B, int Q, int K,
                                  int D, int P, void* stream) {
  if (!smx_shape_ok(B, Q, K, D, P)) return fail(RSCOTR_E_SHAPE, "rscotr_seg_mix_fwd: bad shape (1 <= K <= 32, D in {64, 128, 256}, B <= 512)");
  if (B == 0) return RSCOTR_OK;
  if (!cls || !e || !mf || !mix || !seg) return fail(RSCOTR_E_ARG, "rscotr_seg_mix_fwd: null pointer");
  if (!aligned16(mf) || !aligned16(mix) || !aligned16(e))
    return fail(RSCOTR_E_ALIGN, "rscotr_seg_mix_fwd: e, mf and mix must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  seg_mix_m_kernel<<<dim3(K, B), 256, 0, s>>>(cls, e, mix, Q, K, D);
  const int nwg = std::max(1, std::min((P + SMX_FWD_ROWS - 1) / SMX_FWD_ROWS, SMX_FWD_WG / B));
  const size_t lds = (size_t)K * D * 4;
  const dim3 grid(nwg, B);
  if (D == 256) seg_mix_fwd_kernel<4><<<grid, 256, lds, s>>>(mf, mix, seg, K, P);
  else if (D == 128) seg_mix_fwd_kernel<2><<<grid, 256, lds, s>>>(mf, mix, seg, K, P);
  else seg_mix_fwd_kernel<1><<<grid, 256, lds, s>>>(mf, mix, seg, K, P);
  return check_launch("rscotr_seg_mix_fwd");
}

// dmf / de / dcls: any of them may be NULL (not wanted).  With dmf alone the partial slabs, the fold and the query launch are
// skipped; with dmf NULL the pass over mf writes nothing but its slab.
extern "C" int rscotr_seg_mix_bwd(const float* g, const float* cls, const float* e, const float* mf, const float* mix, float* dmf,
                                  float* de, float* dcls, float* dmix, int B, int Q, int K, int D, int P, float* workspace,
                                  int64_t workspace_bytes, void* stream) {
  if (!smx_shape_ok(B, Q, K, D, P)) return fail(RSCOTR_E_SHAPE, "rscotr_seg_mix_bwd: bad shape (1 <= K <= 32, D in {64, 128, 256}, B <= 512)");
  if (B == 0 || (!dmf && !de && !dcls)) return RSCOTR_OK;
  const bool qg = de || dcls;
  if (!g || !mf || (dmf && !mix) || (qg && (!cls || !e || !dmix))) return fail(RSCOTR_E_ARG, "rscotr_seg_mix_bwd: null pointer");
  if (!aligned16(mf) || (dmf && (!aligned16(mix) || !aligned16(dmf))))
    return fail(RSCOTR_E_ALIGN, "rscotr_seg_mix_bwd: mf, mix and dmf must be 16-byte aligned");
  if (qg && (!workspace || !aligned16(workspace) || workspace_bytes < rscotr_seg_mix_workspace()))
    return fail(RSCOTR_E_ARG, "rscotr_seg_mix_bwd: 16-byte aligned workspace of rscotr_seg_mix_workspace() bytes required");
  hipStream_t s = (hipStream_t)stream;
  const int rows = smx_bwd_rows(K, D);
  const int nwg = std::max(1, std::min((P + rows - 1) / rows, SMX_BWD_WG / B));
  const size_t lds = (size_t)K * D * 4;
  const dim3 grid(nwg, B);
  float* part = qg ? workspace : nullptr;
  if (D == 256) smx_launch_bwd<64>(K, grid, lds, s, g, mf, mix, dmf, part, P);
  else if (D == 128) smx_launch_bwd<32>(K, grid, lds, s, g, mf, mix, dmf, part, P);
  else smx_launch_bwd<16>(K, grid, lds, s, g, mf, mix, dmf, part, P);
  if (qg) {
    const long total = (long)B * K * D;
    seg_mix_fold_kernel<<<(int)((total + 15) / 16), 256, 0, s>>>(part, dmix, nwg, K * D, total);
    seg_mix_qgrad_kernel<<<dim3(Q, B), D, 0, s>>>(cls, e, dmix, de, dcls, Q, K, D);
  }
  return check_launch("rscotr_seg_mix_bwd");
}
