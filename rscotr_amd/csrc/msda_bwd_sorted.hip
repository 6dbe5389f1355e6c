// MSDA backward, grad_value by counting sort + pull (the "sorted" strategy; kept as an independent formulation, and what a
// tiled request falls back to when msda_tiles_build refuses the pyramid): its workspace layout, its six kernels and
// launch_msda_bwd_sorted.  grad_loc / grad_attn come from the sample kernel (msda_bwd_sample.hip), launched from here.
#include "msda_bwd.h"

namespace rscotr {

// ---------------------------------------------------------------------------------------------
// backward, grad_value by destination ("pull") — no fp32 atomics in the common case
// ---------------------------------------------------------------------------------------------
// Device-scope fp32 atomics execute at the memory side on MI355X (one fabric transaction per
// dword): the 4 taps x D channels of every sample made the scatter formulation ~50x slower than
// the forward gather.  Instead the samples of one (batch, head) are counting-sorted by the token
// their TOP-LEFT tap lands on (an "extended" (H_l+1) x (W_l+1) grid per level, so that top-left
// taps one pixel outside the map have a bin too); every value token then PULLS its gradient from
// the four bins whose 2x2 footprint covers it, D lanes per token, with plain 128-byte gathers of
// grad_out rows (L2-resident: one head's slice per XCD) and a plain coalesced store.  Tokens with
// long lists (the coarse levels) are cut into chunks of MSDA_CH taps that combine with atomics —
// a few hundred lines per launch instead of millions.
//
// Workspace (int32 words, per bh = b*H + h, NE = extended bins <= 2*Nk + 2*L):
//   cnt[BH][NEmax], then per bh: start[NEmax+1] | keyrank[2*Nq*LP] | sorted[Nq*LP] x int4 | itemoff[Nk+1] |
//   items[2*maxItems] | nitems
// taps per work item of the pull kernel
// 32, not 128: with 128 (fewer atomics, plan kernel 34 -> 18 us, round time unchanged) AND the bf16x3 weight-gradient route
// on, the 512^2 seg step lost parity whenever earlier processes had left data in device memory (140-440 of 459 gradient
// tensors outside the tight tier; 10-13 with either switch alone, 8 of 8 runs) — an unwritten word is read somewhere
// on that combination (both use the shared workspace); not found yet, so the long-standing value stays.
constexpr int MSDA_CH = 32;
// LDS words of the bin histogram: the host only knows the bound NE <= 2 Nk + 2 L + 2 (the level shapes live on the
// device); the kernels know NE = sum (H_l + 1)(W_l + 1) (~1.03 Nk for image pyramids) and all take the same
// decision: NE > lds_words -> the sorted path stands down and the sample kernel scatters with atomics instead.
constexpr int MSDA_LDS_WORDS = (156 * 1024) / 4;
constexpr int MSDA_MAXCHUNK = 64;  // sample chunks (one wavefront each) per (b,h) in the histogram pass

struct MsdaWs {
  long chunkcnt;  // word offset of chunkcnt[BH][C][NEmax] (cnt[BH][NEmax] sits at offset 0)
  long body;      // word offset of the first per-(b,h) block
  long per_bh;    // words per (b,h) block
  long start, keyrank, sorted, itemoff, items, nitems, cpart, mclist;  // word offsets inside a bh block
  int NEmax, maxItems, C, CH;
  int lds_words;  // bins the LDS histogram of the hist / plan kernels can hold (<= NEmax)
};

static MsdaWs msda_ws_layout(int BH, int Nk, int Nq, int L, int P) {
  MsdaWs w;
  const long S = (long)Nq * L * P;
  w.NEmax = 2 * Nk + 2 * L + 2;
  w.lds_words = std::min(w.NEmax, MSDA_LDS_WORDS);
  w.CH = MSDA_CH;
  w.maxItems = (int)(Nk + (S * 4 + w.CH - 1) / w.CH + 1);
  w.C = (int)std::max<long>(1, std::min<long>(MSDA_MAXCHUNK, S / 1024));
  w.chunkcnt = ((long)BH * w.NEmax + 3) & ~3L;
  w.body = (w.chunkcnt + (long)BH * w.C * w.NEmax + 3) & ~3L;
  long o = 0;
  w.start = o; o += w.NEmax + 1;
  o = (o + 1) & ~1L;
  w.keyrank = o; o += 2 * S;
  o = (o + 3) & ~3L;
  w.sorted = o; o += 4 * S;  // one 16-byte record per sample: {query, weight, lh, lw}
  w.itemoff = o; o += Nk + 1;
  o = (o + 1) & ~1L;
  w.items = o; o += 2L * w.maxItems;
  w.nitems = o; o += 2;
  o = (o + 3) & ~3L;
  w.cpart = o; o += (long)w.maxItems * 64;  // one partial row (<= 64 channels) per work item of a multi-chunk token
  w.mclist = o; o += Nk + 2;                // [0] = number of multi-chunk tokens, then their ids (ascending)
  w.per_bh = (o + 3) & ~3L;
  return w;
}

struct LevelGeom {
  int Hl[MSDA_MAXL], Wl[MSDA_MAXL], lsi[MSDA_MAXL], ext[MSDA_MAXL + 1];
};

__device__ __forceinline__ void load_geom(LevelGeom* g, const int64_t* shapes, const int64_t* lsi, int L) {
  if (threadIdx.x == 0) {
    int e = 0;
    for (int l = 0; l < L; ++l) {
      g->Hl[l] = (int)shapes[2 * l];
      g->Wl[l] = (int)shapes[2 * l + 1];
      g->lsi[l] = (int)lsi[l];
      g->ext[l] = e;
      e += (g->Hl[l] + 1) * (g->Wl[l] + 1);
    }
    g->ext[L] = e;
  }
  __syncthreads();
}

// grid (C, BH), ONE wavefront per workgroup: LDS histogram of one chunk of the samples of (b,h) over the extended bins;
// the LDS atomic's return value is the sample's rank inside (chunk, bin).  One wavefront walks its chunk in program order,
// so the ranks depend on nothing but the data (the LDS serialises the equal-bin lanes of one instruction in a fixed
// order): the sorted record order, hence the summation order of the pull kernel, is the same in every run.  (With four
// wavefronts per chunk — round 1 — their atomics interleaved by timing and grad_value was reproducible to rounding only.)
__global__ __launch_bounds__(64) void msda_hist_kernel(const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ lsi,
                                                        const float* __restrict__ loc, int* __restrict__ ws,
                                                        MsdaWs W, int Nq, int H, int L, int P) {
  extern __shared__ int s_cnt[];
  __shared__ LevelGeom g;
  load_geom(&g, shapes, lsi, L);
  const int NE = g.ext[L];
  if (NE > W.lds_words) return;  // scatter fallback (see MSDA_LDS_WORDS)
  for (int i = threadIdx.x; i < NE; i += 64) s_cnt[i] = 0;
  __syncthreads();
  const int LP = L * P;
  const long S = (long)Nq * LP;
  const int c = blockIdx.x, bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  int* base = ws + W.body + (long)bh * W.per_bh;
  const long s0 = S * c / W.C, s1 = S * (c + 1) / W.C;
  // four rounds of locations in flight per wavefront (the chain load -> LDS atomic -> store is latency-bound otherwise)
  for (long r0 = s0; r0 < s1; r0 += 4 * 64) {
    float2 xy[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long sid = r0 + u * 64 + threadIdx.x;
      xy[u] = make_float2(-9.f, -9.f);
      if (sid < s1) {
        const int q = (int)(sid / LP), lp = (int)(sid - (long)q * LP);
        xy[u] = *reinterpret_cast<const float2*>(loc + ((((long)b * Nq + q) * H + h) * LP + lp) * 2);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long sid = r0 + u * 64 + threadIdx.x;
      if (sid >= s1) continue;
      const int lp = (int)(sid % LP), l = lp / P;
      const int Hl = g.Hl[l], Wl = g.Wl[l];
      const float h_im = msda_pix(xy[u].y, Hl), w_im = msda_pix(xy[u].x, Wl);
      const bool in = (h_im > -1.f) && (w_im > -1.f) && (h_im < (float)Hl) && (w_im < (float)Wl);
      int key = -1, rank = 0;
      if (in) {
        const int ye = (int)floorf(h_im) + 1, xe = (int)floorf(w_im) + 1;
        key = g.ext[l] + ye * (Wl + 1) + xe;
        rank = atomicAdd(&s_cnt[key], 1);
      }
      *reinterpret_cast<int2*>(base + W.keyrank + 2 * sid) = make_int2(key, rank);
    }
  }
  __syncthreads();
  int* out = ws + W.chunkcnt + ((long)bh * W.C + c) * W.NEmax;
  for (int i = threadIdx.x; i < NE; i += 64) out[i] = s_cnt[i];
}

// grid (ceil(NEmax/256), BH): per bin, exclusive prefix over the chunks (in place) and the total
__global__ __launch_bounds__(256) void msda_binsum_kernel(const int64_t* __restrict__ shapes, int* __restrict__ ws,
                                                          MsdaWs W, int L) {
  int NE = 0;
  for (int l = 0; l < L; ++l) NE += ((int)shapes[2 * l] + 1) * ((int)shapes[2 * l + 1] + 1);
  const int i = blockIdx.x * 256 + threadIdx.x, bh = blockIdx.y;
  if (i >= NE || NE > W.lds_words) return;
  int* cc = ws + W.chunkcnt + (long)bh * W.C * W.NEmax + i;
  int run = 0;
  for (int c = 0; c < W.C; ++c) {
    const int t = cc[(long)c * W.NEmax];
    cc[(long)c * W.NEmax] = run;
    run += t;
  }
  ws[(long)bh * W.NEmax + i] = run;
}

// exclusive prefix over the 1024 threads of the block
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_part, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_part[w] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int i = 0; i < 16; ++i) {
    if (i < w) off += s_part[i];
    tot += s_part[i];
  }
  *total = tot;
  __syncthreads();
  return off + inc - v;
}

// one 1024-thread workgroup per (b,h): bin starts, per-token tap counts -> work items of the pull kernel
template <int D>
__global__ __launch_bounds__(1024) void msda_plan_kernel(const int64_t* __restrict__ shapes,
                                                         const int64_t* __restrict__ lsi, int* __restrict__ ws,
                                                         MsdaWs W, float* __restrict__ grad_value, int Nk, int H,
                                                         int L) {
  extern __shared__ int s_cnt[];
  __shared__ LevelGeom g;
  __shared__ int s_part[16];
  load_geom(&g, shapes, lsi, L);
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  int* base = ws + W.body + (long)bh * W.per_bh;
  const int* cnt = ws + (long)bh * W.NEmax;
  int* start = base + W.start;
  const int NE = g.ext[L];
  if (NE > W.lds_words) return;
  const int tid = threadIdx.x;
  for (int i = tid; i < NE; i += 1024) s_cnt[i] = cnt[i];
  __syncthreads();
  // A: exclusive scan of the bin counts
  {
    const int per = (NE + 1023) / 1024;
    const int i0 = min(NE, tid * per), i1 = min(NE, i0 + per);
    int sum = 0;
    for (int i = i0; i < i1; ++i) sum += s_cnt[i];
    int total;
    int run = block_exclusive_scan(sum, s_part, &total);
    for (int i = i0; i < i1; ++i) {
      start[i] = run;
      run += s_cnt[i];
    }
    if (tid == 0) start[NE] = total;
  }
  // B: taps per token = its four covering bins; chunks of MSDA_CH -> items
  {
    int* itemoff = base + W.itemoff;
    int2* items = reinterpret_cast<int2*>(base + W.items);
    const int per = (Nk + 1023) / 1024;
    const int t0 = min(Nk, tid * per), t1 = min(Nk, t0 + per);
    int sum = 0;
    for (int tok = t0; tok < t1; ++tok) {
      int l = 0;
      while (l + 1 < L && tok >= g.lsi[l + 1]) ++l;
      const int Wl = g.Wl[l], r = tok - g.lsi[l];
      const int y = r / Wl, x = r - y * Wl;
      const int e = g.ext[l] + (y + 1) * (Wl + 1) + (x + 1);
      const int taps = s_cnt[e] + s_cnt[e - 1] + s_cnt[e - (Wl + 1)] + s_cnt[e - (Wl + 1) - 1];
      sum += max(1, (taps + W.CH - 1) / W.CH);
    }
    int total;
    int run = block_exclusive_scan(sum, s_part, &total);
    int nmc = 0;
    for (int tok = t0; tok < t1; ++tok) {
      int l = 0;
      while (l + 1 < L && tok >= g.lsi[l + 1]) ++l;
      const int Wl = g.Wl[l], r = tok - g.lsi[l];
      const int y = r / Wl, x = r - y * Wl;
      const int e = g.ext[l] + (y + 1) * (Wl + 1) + (x + 1);
      const int taps = s_cnt[e] + s_cnt[e - 1] + s_cnt[e - (Wl + 1)] + s_cnt[e - (Wl + 1) - 1];
      const int nch = max(1, (taps + W.CH - 1) / W.CH);
      itemoff[tok] = run;
      for (int j = 0; j < nch; ++j) items[run + j] = make_int2(tok, j);
      run += nch;
      nmc += nch > 1;
    }
    // tokens whose list was cut into several items, in ascending order (the chunk-combine kernel walks this list)
    int mtotal;
    int mrun = block_exclusive_scan(nmc, s_part, &mtotal);
    int* mclist = base + W.mclist;
    for (int tok = t0; tok < t1; ++tok)
      if (itemoff[tok] + 1 < ((tok + 1 < t1) ? itemoff[tok + 1] : run)) mclist[1 + mrun++] = tok;
    if (tid == 0) mclist[0] = mtotal;
    if (tid == 0) {
      itemoff[Nk] = total;
      base[W.nitems] = total;
    }
  }
}

// grid (C, BH): scatter the samples to their sorted slots as 16-byte records {query, attention weight, lh, lw}.
// loc / attn are read here in sample order (coalesced), so that the pull kernel's dependent chain is
// item -> bin -> record -> row instead of item -> bin -> sample id -> loc / attn -> row.
__global__ __launch_bounds__(256) void msda_fill_kernel(const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ lsi,
                                                        const float* __restrict__ loc,
                                                        const float* __restrict__ attn, int* __restrict__ ws, MsdaWs W,
                                                        int Nq, int H, int L, int P) {
  __shared__ LevelGeom g;
  load_geom(&g, shapes, lsi, L);
  if (g.ext[L] > W.lds_words) return;
  const int c = blockIdx.x, bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int LP = L * P;
  const long S = (long)Nq * LP;
  int* base = ws + W.body + (long)bh * W.per_bh;
  int4* rec = reinterpret_cast<int4*>(base + W.sorted);
  const int* cbase = ws + W.chunkcnt + ((long)bh * W.C + c) * W.NEmax;
  const long s0 = S * c / W.C, s1 = S * (c + 1) / W.C;
  for (long sid = s0 + threadIdx.x; sid < s1; sid += 256) {
    const int2 kr = *reinterpret_cast<const int2*>(base + W.keyrank + 2 * sid);
    if (kr.x < 0) continue;
    const int q = (int)(sid / LP), lp = (int)(sid - (long)q * LP), l = lp / P;
    const long so = (((long)b * Nq + q) * H + h) * LP + lp;
    const float2 xy = *reinterpret_cast<const float2*>(loc + so * 2);
    const float a = attn[so];
    const float h_im = msda_pix(xy.y, g.Hl[l]), w_im = msda_pix(xy.x, g.Wl[l]);
    const float lh = h_im - floorf(h_im), lw = w_im - floorf(w_im);
    rec[base[W.start + kr.x] + cbase[kr.x] + kr.y] = make_int4(q, __float_as_int(a), __float_as_int(lh), __float_as_int(lw));
  }
}

// D lanes per work item (token, chunk): gather-accumulate grad_out rows of the chunk's taps.  The kernel is bound
// by its dependent loads (item -> bin counts / starts -> record -> row), not by bandwidth: every lane group works
// on U independent items at once, the loads of each level issued together, which doubles the memory-level
// parallelism of a wavefront at the same occupancy.
template <int D, int U>
__global__ __launch_bounds__(256) void msda_pull_kernel(const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ lsi,
                                                        const float* __restrict__ grad_out,
                                                        float* __restrict__ grad_value, int* __restrict__ ws,
                                                        MsdaWs W, int Nk, int Nq, int H, int L, int blocks_per_bh) {
  constexpr int GPB = 256 / D;  // lane groups per workgroup
  __shared__ LevelGeom g;
  load_geom(&g, shapes, lsi, L);
  if (g.ext[L] > W.lds_words) return;
  const int bh = blockIdx.x / blocks_per_bh, blk = blockIdx.x - bh * blocks_per_bh;
  const int b = bh / H, h = bh % H;
  int* base = ws + W.body + (long)bh * W.per_bh;
  const int* cnt = ws + (long)bh * W.NEmax;
  const int grp = threadIdx.x / D, ln = threadIdx.x % D;
  const int nitems = base[W.nitems];
  if ((long)blk * U * GPB >= nitems) return;  // whole workgroup past the end
  const int4* rec = reinterpret_cast<const int4*>(base + W.sorted);
  const float* go_b = grad_out + ((long)b * Nq * H + h) * D + ln;

  bool live[U];
  int2 it[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int item = (blk * U + u) * GPB + grp;
    live[u] = item < nitems;
    it[u] = live[u] ? reinterpret_cast<const int2*>(base + W.items)[item] : make_int2(0, 0);
  }
  int c[U][4], s[U][4], nch[U], p0[U], p1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int tok = it[u].x;
    int l = 0;
    while (l + 1 < L && tok >= g.lsi[l + 1]) ++l;
    const int Wl = g.Wl[l], r = tok - g.lsi[l];
    const int y = r / Wl, x = r - y * Wl;
    const int e0 = g.ext[l] + (y + 1) * (Wl + 1) + (x + 1);
    const int eb[4] = {e0, e0 - 1, e0 - (Wl + 1), e0 - (Wl + 1) - 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[u][k] = cnt[eb[k]];
      s[u][k] = base[W.start + eb[k]];
    }
    nch[u] = base[W.itemoff + tok + 1] - base[W.itemoff + tok];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int total = live[u] ? c[u][0] + c[u][1] + c[u][2] + c[u][3] : 0;
    p0[u] = it[u].y * W.CH;
    p1[u] = max(p0[u], min(total, p0[u] + W.CH));
  }
  float acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = 0.f;
  for (int pb = 0; pb < W.CH; pb += D) {
    // lane ln resolves tap p0 + pb + ln of each item: which bin, which record, its coefficient
    float coef[U];
    int q[U];
    int nb = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pos = p0[u] + pb + ln;
      coef[u] = 0.f;
      q[u] = 0;
      if (pos < p1[u]) {
        int k = 0, off = pos;
        if (off >= c[u][0]) { off -= c[u][0]; k = 1;
          if (off >= c[u][1]) { off -= c[u][1]; k = 2;
            if (off >= c[u][2]) { off -= c[u][2]; k = 3; } } }
        const int sk = (k == 0) ? s[u][0] : (k == 1) ? s[u][1] : (k == 2) ? s[u][2] : s[u][3];
        const int4 rc = rec[sk + off];
        q[u] = rc.x;
        const float a = __int_as_float(rc.y), lh = __int_as_float(rc.z), lw = __int_as_float(rc.w);
        coef[u] = a * ((k & 2) ? lh : 1.f - lh) * ((k & 1) ? lw : 1.f - lw);
      }
      nb = max(nb, min(D, p1[u] - p0[u] - pb));
    }
#pragma unroll
    for (int o = D; o < kWave; o <<= 1) nb = max(nb, __shfl_xor(nb, o, 64));  // wave-uniform trip count
    if (nb <= 0) break;
    // 8 independent row gathers in flight per item and step; lanes past the end carry coef 0 / row 0
    for (int j0 = 0; j0 < nb; j0 += 8) {
      float cj[U][8], gj[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          cj[u][t] = __shfl(coef[u], j0 + t, D);
          const int qj = __shfl(q[u], j0 + t, D);
          gj[u][t] = go_b[(long)qj * H * D];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[u] += cj[u][t] * gj[u][t];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!live[u]) continue;
    if (nch[u] > 1) {  // chunk of a long list: partial row, folded in chunk order by msda_chunk_combine_kernel (no atomics)
      const int item = (blk * U + u) * GPB + grp;
      reinterpret_cast<float*>(base + W.cpart)[(long)item * D + ln] = acc[u];
    } else {
      grad_value[(((long)b * Nk + it[u].x) * H + h) * D + ln] = acc[u];
    }
  }
}

// grad_value rows of the tokens whose tap list was cut into several work items: partial rows summed in chunk order.
// grid (blocks, BH): D lanes per token of the (b,h)'s multi-chunk list (msda_plan_kernel).
template <int D>
__global__ __launch_bounds__(256) void msda_chunk_combine_kernel(const int64_t* __restrict__ shapes, float* __restrict__ grad_value,
                                                                 const int* __restrict__ ws, MsdaWs W, int Nk, int H, int L) {
  int NE = 0;
  for (int l = 0; l < L; ++l) NE += ((int)shapes[2 * l] + 1) * ((int)shapes[2 * l + 1] + 1);
  if (NE > W.lds_words) return;  // the sorted path stood down
  constexpr int TPB = 256 / D;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int* base = ws + W.body + (long)bh * W.per_bh;
  const int* mclist = base + W.mclist;
  const int n = mclist[0], ln = threadIdx.x % D;
  const float* part = reinterpret_cast<const float*>(base + W.cpart);
  for (int k = blockIdx.x * TPB + threadIdx.x / D; k < n; k += gridDim.x * TPB) {
    const int tok = mclist[1 + k];
    const int i0 = base[W.itemoff + tok], i1 = base[W.itemoff + tok + 1];
    float v = 0.f;
    for (int j = i0; j < i1; ++j) v += part[(long)j * D + ln];
    grad_value[(((long)b * Nk + tok) * H + h) * D + ln] = v;
  }
}

int64_t msda_sorted_ws_bytes(int BH, int Nk, int Nq, int L, int P) {
  const MsdaWs W = msda_ws_layout(BH, Nk, Nq, L, P);
  return (int64_t)(W.body + (long)BH * W.per_bh) * 4;
}

bool msda_sorted_may_stand_down(int Nk, int L) { return 2 * Nk + 2 * L + 2 > MSDA_LDS_WORDS; }  // (MsdaWs: NEmax > lds_words)

template <int D>
static void launch_sorted(const MsdaBwdArgs& a, int* ws, bool may_stand_down) {
  const float *go = a.go, *loc = a.loc, *attn = a.attn;
  const int64_t *shapes = a.shapes, *lsi = a.lsi;
  float* gv = a.gv;
  const int B = a.B, Nk = a.Nk, Nq = a.Nq, H = a.H, L = a.L, P = a.P;
  hipStream_t s = a.s;
  const int BH = B * H;
  const MsdaWs W = msda_ws_layout(BH, Nk, Nq, L, P);
  const size_t hist_lds = (size_t)W.lds_words * sizeof(int);
  if (hist_lds > 48 * 1024) {  // opt in to large dynamic LDS (up to the 160 KB of a CU)
    hipFuncSetAttribute(reinterpret_cast<const void*>(&msda_hist_kernel),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&msda_plan_kernel<D>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds);
  }
  msda_hist_kernel<<<dim3(W.C, BH), 64, hist_lds, s>>>(shapes, lsi, loc, ws, W, Nq, H, L, P);
  if (may_stand_down) {
    // grad_value zeroed for the scatter the sample kernel falls back to; on the sorted path the pull kernel overwrites it
    hipMemsetAsync(gv, 0, (size_t)B * Nk * H * D * sizeof(float), s);
    launch_msda_bwd_sample(a, MSDA_SAMPLE_SCATTER_IF, nullptr, nullptr, nullptr, W.lds_words);
  } else {
    launch_msda_bwd_sample(a, MSDA_SAMPLE_GRADS, nullptr, nullptr, nullptr, 0);
  }
  msda_binsum_kernel<<<dim3((W.NEmax + 255) / 256, BH), 256, 0, s>>>(shapes, ws, W, L);
  msda_plan_kernel<D><<<BH, 1024, hist_lds, s>>>(shapes, lsi, ws, W, gv, Nk, H, L);
  msda_fill_kernel<<<dim3(W.C, BH), 256, 0, s>>>(shapes, lsi, loc, attn, ws, W, Nq, H, L, P);
  constexpr int GPB = 256 / D;
  const int bpb = (W.maxItems + GPB - 1) / GPB;
  msda_pull_kernel<D, 1><<<dim3((unsigned)((long)BH * bpb)), 256, 0, s>>>(shapes, lsi, go, gv, ws, W, Nk, Nq, H, L, bpb);
  msda_chunk_combine_kernel<D><<<dim3(64, BH), 256, 0, s>>>(shapes, gv, ws, W, Nk, H, L);
}

void launch_msda_bwd_sorted(const MsdaBwdArgs& a, int* ws, bool may_stand_down) {
  switch (a.D) {
    case 16: launch_sorted<16>(a, ws, may_stand_down); break;
    case 32: launch_sorted<32>(a, ws, may_stand_down); break;
    case 64: launch_sorted<64>(a, ws, may_stand_down); break;
  }
}

}  // namespace rscotr
