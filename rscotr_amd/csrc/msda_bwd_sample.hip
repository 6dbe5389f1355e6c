// MSDA backward, the sample kernel: one (b, q-tile, head) per 256-thread workgroup as in the forward (msda_fwd.hip).  Per-lane
// partial sums over 4 channels, a reduce-scatter over the G = D / 4 lanes of a query, grad_loc / grad_attn gathered in LDS and
// written back coalesced.  What it does for grad_value depends on the strategy (msda_bwd.h: MsdaSampleMode): nothing, an atomic
// scatter (global_atomic_add_f32), the scatter only if the sorted strategy stood down, or the bin words and block masks of the
// tiled strategy.  Every instantiation lives in this object; launch_msda_bwd_sample is the only launch site.
#include "msda_bwd.h"

namespace rscotr {

__device__ __forceinline__ void atomic_add4(float* p, float4 v, bool ok) {
  if (ok) {
    unsafeAtomicAdd(p + 0, v.x);
    unsafeAtomicAdd(p + 1, v.y);
    unsafeAtomicAdd(p + 2, v.z);
    unsafeAtomicAdd(p + 3, v.w);
  }
}

// Reduce-scatter over a lane group (see msda_bwd_kernel): one butterfly step at lane offset O on N live values per lane; the
// lane whose `sub & O` is clear keeps the first ceil(N / 2) values, its partner the rest (zero-padded), each adding what the
// other sends.  rs_final<N, O>() = values per lane after the steps O, O / 2, ..., 1.
template <int N, int O>
constexpr int rs_final() {
  if constexpr (O == 0) return N; else return rs_final<(N + 1) / 2, O / 2>();
}
template <int N0, int N, int O>
__device__ __forceinline__ void rs_steps(float (&cur)[N0], int sub, int& base, int& rend) {
  if constexpr (O > 0) {
    constexpr int KEEP = (N + 1) / 2;
    const bool hi = (sub & O) != 0;
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {  // (writes slots < KEEP only: slot i + KEEP is still this step's input)
      const float lo_v = cur[i], hi_v = (i + KEEP < N) ? cur[i + KEEP] : 0.f;
      const float mine = hi ? hi_v : lo_v, other = hi ? lo_v : hi_v;
      cur[i] = mine + __shfl_xor(other, O, 64);
    }
    if (hi) base += KEEP; else rend = min(rend, base + KEEP);
    rs_steps<N0, KEEP, O / 2>(cur, sub, base, rend);
  }
}

// SCATTER: 0 = grad_loc / grad_attn only (grad_value comes from the pull kernel), 1 = also scatter grad_value with
// atomics, 2 = scatter iff the level pyramid has more than `bins_cap` extended bins (the sorted path stood down).
// TILE: also leave what the tile-accumulation backward needs (see that section): one bin word per sample + the block masks.
template <int D, int P, int SCATTER, bool TILE = false>
__global__ __launch_bounds__(256, P <= 4 && SCATTER == 0 ? 4 : 2) void msda_bwd_kernel(
    const float* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ lsi, const float* __restrict__ loc,
    const float* __restrict__ attn, const float* __restrict__ grad_out,
    float* __restrict__ grad_value, float* __restrict__ grad_loc, float* __restrict__ grad_attn,
    int* __restrict__ binw, unsigned long long* __restrict__ mask, MsdaMaskGeom MG, int Nk, int Nq,
    int H, int L, int ntiles, int bins_cap) {
  constexpr int G = D / 4;
  constexpr int QW = kWave / G;
  constexpr int QB = 4 * QW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int LP = L * P;
  bool scatter = SCATTER == 1;
  if (SCATTER == 2) {
    int NE = 0;
    for (int l = 0; l < L; ++l) NE += ((int)shapes[2 * l] + 1) * ((int)shapes[2 * l + 1] + 1);
    scatter = NE > bins_cap;
  }
  // one record per sample (the set-up is done ONCE, by the thread that stages the sample — as in the forward kernel: the G lanes
  // of a (query, head) used to repeat it inside the gather loop), the gradients gathered for a coalesced store, and (TILE) one
  // 4-byte bin word per sample (bin of the top-left tap on the extended grid | -1), staged [L][QB][P]
  MsdaSampleB* recs = reinterpret_cast<MsdaSampleB*>(smem);  // [QB][LP]
  float* s_gattn = smem + QB * LP * 8;       // [QB][LP]    out: grad_attn
  float* s_gloc = smem + QB * LP * 9;        // [QB][LP*2]  out: grad_loc
  int* s_bin = reinterpret_cast<int*>(smem + QB * LP * 11);
  unsigned* s_mask = reinterpret_cast<unsigned*>(smem + QB * LP * 12);  // [L][2] (TILE only)
  if (TILE && threadIdx.x < 2 * L) s_mask[threadIdx.x] = 0u;  // (ordered before the atomics by the barrier below)

  const int bid = blockIdx.x;
  const int h = bid % H;
  const int t = bid / H;
  const int tile = t % ntiles;
  const int b = t / ntiles;
  const int q0 = tile * QB;
  const int tid = threadIdx.x;
  const int tok_stride = H * D;
  if (TILE) __syncthreads();

  for (int i = tid; i < QB * LP; i += 256) {
    const int rr = i / LP, c = i - rr * LP, l = c / P, pp = c - l * P;
    const int q = q0 + rr;
    MsdaSampleB m;
    m.aw = m.hh = m.hw = m.lh = m.lw = 0.f;
    m.e1 = m.ok = m.pad = 0;
    bool in = false;
    int h_low = 0, w_low = 0;
    if (q < Nq) {
      const long e = (((long)b * Nq + q) * H + h) * LP + c;
      const float2 xy = *reinterpret_cast<const float2*>(loc + e * 2);
      const Bilinear gg = bilinear_setup(xy.x, xy.y, (int)shapes[2 * l], (int)shapes[2 * l + 1]);
      m.aw = attn[e];
      m.hh = gg.hh; m.hw = gg.hw; m.lh = gg.lh; m.lw = gg.lw;
      m.e1 = gg.i1 * tok_stride;  // (from the level's first token: grad_value is addressed with the same offset)
      m.ok = (gg.ok1 ? 1 : 0) | (gg.ok2 ? 2 : 0) | (gg.ok3 ? 4 : 0) | (gg.ok4 ? 8 : 0) | (gg.in ? 16 : 0);
      in = gg.in; h_low = gg.h_low; w_low = gg.w_low;
    }
    recs[i] = m;
    if (TILE) {
      s_bin[(l * QB + rr) * P + pp] = in ? ((h_low + 1) << 16) | (w_low + 1) : -1;
      if (in) {  // (+ 0.5: the quotient is at least 1 / 32 away from an integer, far above the rounding of the product)
        const int tt = (int)(((float)(h_low + 1) + 0.5f) * MG.ity[l]) * MG.ntx[l] + (int)(((float)(w_low + 1) + 0.5f) * MG.itx[l]);
        atomicOr(&s_mask[2 * l + ((tt >> 5) & 1)], 1u << (tt & 31));
      }
    }
  }
  __syncthreads();

  const int lane = tid & 63, w = tid >> 6;
  const int r = w * QW + lane / G;
  const int sub = lane % G;
  const int q = q0 + r;
  const bool qok = q < Nq;  // keep whole groups alive for the butterflies

  const long voff = ((long)b * Nk * H + h) * D + sub * 4;
  const float* vb = value + voff;
  float* gvb = grad_value + voff;
  const float4 go = qok ? *reinterpret_cast<const float4*>(
                              grad_out + (((long)b * Nq + q) * H + h) * D + sub * 4)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
  const MsdaSampleB* mine = recs + r * LP;  // (rows past Nq hold zero records: nothing is loaded, nothing counts)

  for (int l = 0; l < L; ++l) {
    const int Hl = (int)shapes[2 * l], Wl = (int)shapes[2 * l + 1];
    const long lofs = (long)lsi[l] * tok_stride;
    const float* vl = vb + lofs;
    float* gvl = gvb + lofs;
    const int rowstep = Wl * tok_stride;
    MsdaSampleB g[P];
    float aw[P];
    float4 v1[P], v2[P], v3[P], v4[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float4* rp = reinterpret_cast<const float4*>(mine + l * P + p);
      const float4 ra = rp[0], rb = rp[1];
      g[p].aw = ra.x; g[p].hh = ra.y; g[p].hw = ra.z; g[p].lh = ra.w;
      g[p].lw = rb.x; g[p].e1 = __float_as_int(rb.y); g[p].ok = __float_as_int(rb.z);
      aw[p] = ra.x;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float* t1 = vl + g[p].e1;
      v1[p] = ld4(t1, g[p].ok & 1);
      v2[p] = ld4(t1 + tok_stride, g[p].ok & 2);
      v3[p] = ld4(t1 + rowstep, g[p].ok & 4);
      v4[p] = ld4(t1 + rowstep + tok_stride, g[p].ok & 8);
    }
    float part[3 * P];
    unsigned inmask = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float hh = g[p].hh, hw = g[p].hw, lh = g[p].lh, lw = g[p].lw;
      const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
      const float4 top = scale4(go, aw[p]);  // grad_out * attention weight
      if (scatter) {
        float* t1 = gvl + g[p].e1;
        atomic_add4(t1, scale4(top, w1), g[p].ok & 1);
        atomic_add4(t1 + tok_stride, scale4(top, w2), g[p].ok & 2);
        atomic_add4(t1 + rowstep, scale4(top, w3), g[p].ok & 4);
        atomic_add4(t1 + rowstep + tok_stride, scale4(top, w4), g[p].ok & 8);
      }
      // d(sample)/d(h_im), d(sample)/d(w_im), and the sample itself, dotted with the grads
      const float d1 = dot4(top, v1[p]), d2 = dot4(top, v2[p]);
      const float d3 = dot4(top, v3[p]), d4 = dot4(top, v4[p]);
      // this lane's share (its 4 channels) of the sample's three sums: [3 p] = d/d(w_im), [3 p + 1] = d/d(h_im), [3 p + 2] = d/d(weight)
      part[3 * p + 0] = -hh * d1 + hh * d2 - lh * d3 + lh * d4;
      part[3 * p + 1] = -hw * d1 - lw * d2 + hw * d3 + lw * d4;
      part[3 * p + 2] = w1 * dot4(go, v1[p]) + w2 * dot4(go, v2[p]) + w3 * dot4(go, v3[p]) + w4 * dot4(go, v4[p]);
      if (g[p].ok & 16) inmask |= 1u << p;
    }
    // the 3 P sums of the level over the G lanes of the group as a REDUCE-SCATTER: at every butterfly step a lane keeps one
    // half of the values and sends the other (12 values on 8 lanes: 6 + 3 + 2 = 11 exchanges against 36 for one all-reduce
    // per value); the pairing of the steps is the butterfly's (offsets G/2 ... 1), so every sum is the same float as before.
    // A lane ends with the values base .. base + NF - 1 (those below rend are real)
    {
      constexpr int N0 = 3 * P;
      int base = 0, rend = N0;
      float cur[N0];
#pragma unroll
      for (int i = 0; i < N0; ++i) cur[i] = part[i];
      rs_steps<N0, N0, G / 2>(cur, sub, base, rend);
      constexpr int NF = rs_final<N0, G / 2>();
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const int idx = base + i;
        if (idx < rend) {
          const int pp = (idx * 11) >> 5, k = idx - 3 * pp;  // idx / 3 for idx < 32
          const bool in = (inmask >> pp) & 1u;
          const float val = cur[i];
          if (k == 2) s_gattn[r * LP + l * P + pp] = in ? val : 0.f;
          else s_gloc[(r * LP + l * P + pp) * 2 + k] = in ? (k == 0 ? (float)Wl : (float)Hl) * val : 0.f;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < QB * LP * 2; i += 256) {
    const int rr = i / (LP * 2), c = i - rr * (LP * 2);
    const int qq = q0 + rr;
    if (qq < Nq) grad_loc[(((long)b * Nq + qq) * H + h) * (LP * 2) + c] = s_gloc[i];
  }
  for (int i = tid; i < QB * LP; i += 256) {
    const int rr = i / LP, c = i - rr * LP;
    const int qq = q0 + rr;
    if (qq < Nq) grad_attn[(((long)b * Nq + qq) * H + h) * LP + c] = s_gattn[i];
  }
  if (TILE) {
    const long SP = (long)Nq * P;
    for (int i = tid; i < L * QB * P; i += 256) {
      const int l = i / (QB * P), rem = i - l * (QB * P);
      if (q0 + rem / P < Nq) binw[((long)(b * H + h) * L + l) * ((SP + 3) & ~3L) + (long)q0 * P + rem] = s_bin[i];
    }
    if (tid < L) mask[((long)(b * H + h) * L + tid) * ntiles + tile] = (unsigned long long)s_mask[2 * tid] | ((unsigned long long)s_mask[2 * tid + 1] << 32);
  }
}

template <int D, int P, int SCATTER, bool TILE>
static void launch_sample(const MsdaBwdArgs& a, int* binw, unsigned long long* mask, const MsdaMaskGeom& MG, int bins_cap) {
  constexpr int QB = msda_qb(D);
  const int ntiles = (a.Nq + QB - 1) / QB;
  const size_t shm = msda_bwd_lds(D, a.L, P);  // records + gathered gradients + bin words staged for a coalesced store + masks
  if (shm > 64 * 1024)  // (D = 16 with L P >= 32; plan_msda_bwd refused what passes MSDA_CU_LDS)
    hipFuncSetAttribute(reinterpret_cast<const void*>(&msda_bwd_kernel<D, P, SCATTER, TILE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  msda_bwd_kernel<D, P, SCATTER, TILE><<<dim3((unsigned)((long)a.B * ntiles * a.H)), dim3(256), shm, a.s>>>(
      a.value, a.shapes, a.lsi, a.loc, a.attn, a.go, a.gv, a.gl, a.ga, binw, mask, MG, a.Nk, a.Nq, a.H, a.L, ntiles, bins_cap);
}

template <int D, int P>
static void launch_sample_mode(const MsdaBwdArgs& a, MsdaSampleMode mode, int* binw, unsigned long long* mask,
                               const MsdaMaskGeom& MG, int bins_cap) {
  switch (mode) {
    case MSDA_SAMPLE_GRADS: launch_sample<D, P, 0, false>(a, binw, mask, MG, bins_cap); break;
    case MSDA_SAMPLE_SCATTER: launch_sample<D, P, 1, false>(a, binw, mask, MG, bins_cap); break;
    case MSDA_SAMPLE_SCATTER_IF: launch_sample<D, P, 2, false>(a, binw, mask, MG, bins_cap); break;
    case MSDA_SAMPLE_TILE: launch_sample<D, P, 0, true>(a, binw, mask, MG, bins_cap); break;
  }
}

void launch_msda_bwd_sample(const MsdaBwdArgs& a, MsdaSampleMode mode, int* binw, unsigned long long* mask,
                            const MsdaMaskGeom* MG, int bins_cap) {
  const MsdaMaskGeom mg = MG ? *MG : MsdaMaskGeom();
#define CALL(DD, PP) launch_sample_mode<DD, PP>(a, mode, binw, mask, mg, bins_cap)
  RSCOTR_DISPATCH_DP(a.D, a.P, CALL)
#undef CALL
}

}  // namespace rscotr
