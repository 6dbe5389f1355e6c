// MSDA backward, the tiled strategy: its geometry (MsdaTiles, msda_bwd.h), its workspace layout, msda_tile_kernel,
// msda_tile_combine_kernel and launch_msda_bwd_tiled.
//
// grad_value by TILE ACCUMULATION — deterministic, no global sort (the default strategy).  A sample belongs to the BIN of its top-left tap, (h_low + 1, w_low + 1) on the (H_l + 1) x (W_l + 1) "extended" grid of its
// level; its four taps land on the cells (bin, bin + 1 right, bin + 1 down, both).  The bins of a level are cut into tiles of
// at most 16 x 16 bins (17 x 17 cells with the one-cell halo to the right / bottom), and the samples of a level — in sample
// order — into `nch` chunks; one 256-thread workgroup per (b, h, level, tile, chunk):
//   0. the sample kernel (msda_bwd_kernel<.., TILE = true>) leaves one 4-byte bin word {bin | -1} per sample, laid out
//      (b h, level, q, p), and one 64-bit tile mask per block of its queries and level (a pass of its own over the staged
//      locations);
//   1. SCAN: the workgroup reads the bin words of its chunk (coalesced, L2-resident: all workgroups of a (b, h) run on one
//      XCD) and keeps those whose bin lies in its tile — ballot compaction, so the kept list is in sample order.  No sort of
//      the whole sample set: filtering 16 x redundantly costs less than the counting sort did (5 launches, ~110 us);
//   2. every MSDA_T_CAP kept records (and at the end): stable counting sort of the list by bin inside LDS (one wavefront
//      per quarter of the list, LDS atomics return the rank), then lane groups of D/4 lanes walk the runs of equal bin, bins
//      of one parity class (x & 1, y & 1) at a time: ONE 128-byte gather of the sample's grad_out row serves all four taps
//      (the pull formulation gathers it once per tap), four register accumulators per run, added to the tile's LDS cells
//      at the end of the run — bins of one parity class never share a cell, so plain read-add-write;
//   3. the tile's 17 x 17 cell block goes to a partial buffer; msda_tile_combine_kernel sums, per token, the <= 4 tiles that
//      hold its cell x nch chunks in fixed order and stores grad_value (fully overwritten).
// Every float sum runs in an order fixed by the data layout alone: bit-reproducible.
#include "msda_bwd.h"

namespace rscotr {

constexpr int MSDA_T_TS = 16;      // bins per tile edge (at most)
constexpr int MSDA_T_CW = 17;      // cells per tile edge
constexpr int MSDA_T_CAP = 3072;   // kept records per sort + accumulate round (list entries: 8 bytes)
constexpr int MSDA_T_TARGET = 10;  // mean run length (samples per bin and thread) a sample chunk is sized for
template <int D> constexpr int msda_t_occ() { return D <= 32 ? 3 : 2; }
constexpr int MSDA_T_SEGB = 2048;  // blocks of the sample kernel per scan segment (their numbers live in LDS)

bool msda_tiles_build(MsdaTiles* T, const int64_t* shapes_host, int L, int Nk, long SP, int D) {
  const int tsy_max = D >= 32 ? 8 : 16;  // MsdaTileGeom<D>::TSY
  if (!shapes_host || L < 1 || L > MSDA_T_MAXL) return false;
  constexpr int target = MSDA_T_TARGET;
  T->L = L;
  int nw = 0, tok = 0;
  for (int l = 0; l < L; ++l) {
    const int Hh = (int)shapes_host[2 * l], Ww = (int)shapes_host[2 * l + 1];
    if (Hh < 1 || Ww < 1 || Hh > 32766 || Ww > 32766) return false;
    T->Hl[l] = Hh; T->Wl[l] = Ww; T->lsi[l] = tok;
    T->ntx[l] = (Ww + 1 + MSDA_T_TS - 1) / MSDA_T_TS;
    T->nty[l] = (Hh + 1 + tsy_max - 1) / tsy_max;
    T->tsx[l] = (Ww + 1 + T->ntx[l] - 1) / T->ntx[l];
    T->tsy[l] = (Hh + 1 + T->nty[l] - 1) / T->nty[l];
    const long tiles = (long)T->ntx[l] * T->nty[l];
    // sample chunks: the walk of the tile kernel is a chain of gathers per thread as long as the longest run of equal bin,
    // so a level is cut into as many chunks as keep the MEAN run (samples of the chunk per bin, per thread sharing a bin)
    // near `target` — the coarse levels receive as many samples as the fine ones on a fraction of the bins
    const long nbt = (long)T->tsx[l] * T->tsy[l], sf = std::max<long>(1, std::min<long>(4, (D >= 32 ? 128 : 256) / nbt));
    long nch = (SP + (long)(Hh + 1) * (Ww + 1) * sf * target - 1) / ((long)(Hh + 1) * (Ww + 1) * sf * target);
    nch = std::max<long>(1, std::min<long>(std::min<long>(nch, 64), SP / 512));
    T->nch[l] = (int)nch;
    T->wbase[l] = nw;
    if (tiles * nch > (1 << 20)) return false;
    nw += (int)(tiles * nch);
    tok += Hh * Ww;
  }
  for (int l = L; l < MSDA_T_MAXL; ++l) {
    T->Hl[l] = T->Wl[l] = 1; T->lsi[l] = tok; T->tsx[l] = T->tsy[l] = 2; T->ntx[l] = T->nty[l] = 1; T->nch[l] = 1; T->wbase[l] = nw;
  }
  T->NW = nw;
  return tok == Nk && nw <= (1 << 20);
}

struct MsdaTileWs {
  long binw, mask, part, total;  // byte offsets
};

static MsdaTileWs msda_tile_ws(const MsdaTiles& T, int BH, int Nq, int P, int D) {
  MsdaTileWs w;
  const long SP = (long)Nq * P;
  long o = 0;
  w.binw = o; o += (long)BH * T.L * ((SP + 3) & ~3L) * 4;  // (rows padded to whole 16-byte loads)
  const int QB = msda_qb(D);  // queries per workgroup of the sample kernel
  const long nqt = (Nq + QB - 1) / QB;
  w.mask = o; o += (((long)BH * T.L * nqt * 8) + 15) & ~15L;
  w.part = o; o += (long)BH * T.NW * MSDA_T_CW * ((D >= 32 ? 8 : 16) + 1) * D * 4;
  w.total = o;
  return w;
}

int64_t msda_tiled_ws_bytes(const MsdaTiles& T, int BH, int Nq, int P, int D) { return msda_tile_ws(T, BH, Nq, P, D).total; }

// Per-D geometry of the tile kernel: TB threads own one BIN (two for D >= 32: CH = D / TB channels each), 256 threads per
// workgroup, so a tile has 256 / TB bins: 16 x 16 (D = 16) or 16 x 8 (D = 32, 64).
template <int D>
struct MsdaTileGeom {
  static constexpr int TB = D >= 32 ? 2 : 1;
  static constexpr int CH = D / TB;
  static constexpr int V = CH / 4;                 // float4 per thread and row
  static constexpr int MSDA_T_U16 = 3;  // (4 spilled 17 registers under the 168-register cap of three wavefronts per SIMD once the walk took balanced work items: +21 MiB of scratch writes per launch, encoder call 85 -> 78 us in the lab with 3)
  static constexpr int U = CH <= 16 ? MSDA_T_U16 : 2;  // samples in flight per thread in the walk
  static constexpr int TSY = 256 / TB / MSDA_T_TS;  // bins per tile along y
  static constexpr int NBIN = MSDA_T_TS * TSY;
  static constexpr int NCELL = MSDA_T_CW * (TSY + 1);
  static constexpr size_t lds_bytes() {
    return (size_t)NCELL * D * 4 + (size_t)MSDA_T_CAP * (4 + 2 + 2) + (4 * NBIN + NBIN + 4 + 8 + 4) * 4 + MSDA_T_SEGB * 2;
  }
};

// exclusive prefix sum of one int per thread over the 256 threads of the workgroup; *total = the sum.  `scratch`: 4 ints
// of LDS nobody else touches between the two barriers inside.
__device__ __forceinline__ int block_exclusive_scan_256(int v, int* scratch, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) scratch[w] = inc;
  __syncthreads();
  const int s0 = scratch[0], s1 = scratch[1], s2 = scratch[2], s3 = scratch[3];
  const int before = (w > 0 ? s0 : 0) + (w > 1 ? s1 : 0) + (w > 2 ? s2 : 0);
  *total = s0 + s1 + s2 + s3;
  __syncthreads();
  return before + inc - v;
}

// One 256-thread workgroup per (b, h, level, tile, chunk): see the header of this section.  A thread keeps the four tap
// rows of ITS bin (its CH channels) in registers for the whole life of the workgroup: the walk over the sorted list needs
// no barrier and no LDS accumulator — a thread reads the records of its bin in order, gathers each sample's grad_out row
// (its part) once and feeds the four accumulators; the rows meet in the tile's cells only at the very end.
template <int D, int P>
__global__ __launch_bounds__(256, msda_t_occ<D>()) void msda_tile_kernel(const float* __restrict__ go, const float* __restrict__ loc,
                                                        const float* __restrict__ attn,
                                                        const int* __restrict__ binw, const unsigned long long* __restrict__ mask,
                                                        float* __restrict__ part, MsdaTiles T, int Nq, int bshift,
                                                        int nqt, int H, int BH) {
  constexpr int pshift = P == 1 ? 0 : P == 2 ? 1 : P == 4 ? 2 : 3;
  using Gm = MsdaTileGeom<D>;
  constexpr int TB = Gm::TB, CH = Gm::CH, V = Gm::V, U = Gm::U, NBIN = Gm::NBIN, NCELL = Gm::NCELL;
  constexpr int R = 4;  // consecutive records per thread and scan round (one 16-byte load of bin words)
  extern __shared__ __attribute__((aligned(16))) float t_lds[];
  float* acc = t_lds;                                                   // [NCELL][D] (filled at the very end)
  int* lrec = reinterpret_cast<int*>(acc + NCELL * D);                  // [CAP] sample index << 8 | local bin (kept list)
  unsigned short* order = reinterpret_cast<unsigned short*>(lrec + MSDA_T_CAP);  // [CAP] list positions sorted by bin
  unsigned short* rank = order + MSDA_T_CAP;                            // [CAP]
  int* hist = reinterpret_cast<int*>(rank + MSDA_T_CAP);                // [4][NBIN]
  int* binstart = hist + 4 * NBIN;                                      // [NBIN + 1]
  int* wtot = binstart + NBIN + 4;                                      // [2][4] kept records per wavefront (two buffers)
  int* scratch = wtot + 8;                                              // [4]
  unsigned short* blist = reinterpret_cast<unsigned short*>(scratch + 4);  // [MSDA_T_SEGB] blocks of the segment to scan

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // all workgroups of a (b, h) on one XCD (round-robin dispatch: XCD = id % 8): its records, grad_out slices and
  // partial tiles stay in that L2
  const int x8 = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int bh = x8 + 8 * (j / T.NW), e = j % T.NW;
  if (bh >= BH) return;
  const int b = bh / H, h = bh - b * H;
  int l = 0;
  while (l + 1 < T.L && e >= T.wbase[l + 1]) ++l;
  const int r = e - T.wbase[l];
  const int nch = T.nch[l], chunk = r % nch, tile = r / nch;
  const int ty = tile / T.ntx[l], tx = tile - ty * T.ntx[l];
  const int bx0 = tx * T.tsx[l], by0 = ty * T.tsy[l], bx1 = bx0 + T.tsx[l], by1 = by0 + T.tsy[l];
  const int SP = Nq << pshift;  // (< 2^23: the host checks Nq < 2^20; a multiple of 4 or the host keeps nch = 1 ... see c0)
  // chunk bounds on whole blocks of the sample kernel (BS = 1 << bshift records, >= 16: 16-byte loads of bin words)
  const int BS = 1 << bshift;
  const int c0 = (int)((long)SP * chunk / nch) & ~(BS - 1), c1 = chunk + 1 == nch ? SP : (int)((long)SP * (chunk + 1) / nch) & ~(BS - 1);
  const int* bsrc = binw + ((long)bh * T.L + l) * ((SP + 3) & ~3);

  // Work ITEMS of the walk: after the sort every bin's run is cut into parts of at most R0 records, R0 chosen per sort so
  // that the parts number at most NPAIR (the thread pairs of the workgroup): pair j takes item j.  A bin that collects far
  // more samples than its neighbours (the coarse levels; the padded denoising slots of a DINO decoder call, which all carry
  // the SAME reference box and so put hundreds of samples into one bin: a 150-sample run walked by one pair was a chain of
  // 75 dependent gathers, 80 us for a decoder call against 33 with well-spread queries) is walked by as many pairs as the
  // tile has to spare; the parts of a bin meet in its cells in part order (below), so the sums stay fixed by the data alone
  constexpr int NPAIR = 256 / TB;
  constexpr int RMIN = 16;
  const int pair = tid / TB, sub = tid % TB;
  const float* gob = go + ((long)b * Nq * H + h) * D + sub * CH;  // + q * H * D
  const int qstride = H * D;
  // the walk re-derives a sample's tap weights from its sampling location and attention weight (12 algorithmic bytes per
  // sample, L2-resident) with the sample kernel's arithmetic, hence the same floats — round 2 read a 16-byte record per
  // sample that the sample kernel had written: 45 MB of HBM traffic per launch at the encoder shape of configs[1]
  const int Hl = T.Hl[l], Wl = T.Wl[l];
  const int LP = T.L << pshift;
  const float* locb = loc + (((long)b * Nq * H + h) * T.L + l) * (2 << pshift);   // + q * H * LP * 2 + p * 2
  const float* attb = attn + (((long)b * Nq * H + h) * T.L + l) * (1 << pshift);  // + q * H * LP + p
  const long lstride = (long)H * LP * 2, astride = (long)H * LP;
  typedef float v2f __attribute__((ext_vector_type(2)));  // (pairs: v_pk_fma_f32 does two channels per instruction)
  v2f a1[2 * V], a2[2 * V], a3[2 * V], a4[2 * V];  // the bin's four tap rows (this thread's channels)
  for (int i = tid; i < NCELL * D / 4; i += 256) reinterpret_cast<float4*>(acc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);  // (ordered before the first add by the barriers of the scan)

  // sort the n kept records by bin (stable), then every thread adds the records of its bin to its accumulators
  auto flush = [&](int n) {
    for (int i = tid; i < 4 * NBIN; i += 256) hist[i] = 0;
    __syncthreads();
    const int nw = ((n + 3) / 4 + 63) & ~63;  // records per wavefront (whole rounds of 64)
    const int i0 = w * nw, i1 = min(n, i0 + nw);
    // one wavefront walks its quarter in program order: the rank inside (wavefront, bin) depends on the data only
    for (int i = i0 + lane; i < i1; i += 64) rank[i] = (unsigned short)atomicAdd(&hist[w * NBIN + (lrec[i] & 255)], 1);
    __syncthreads();
    {
      int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
      if (tid < NBIN) { h0 = hist[tid]; h1 = hist[NBIN + tid]; h2 = hist[2 * NBIN + tid]; h3 = hist[3 * NBIN + tid]; }
      int total;
      const int start = block_exclusive_scan_256(h0 + h1 + h2 + h3, scratch, &total);
      if (tid < NBIN) {
        binstart[tid] = start;
        hist[tid] = start; hist[NBIN + tid] = start + h0; hist[2 * NBIN + tid] = start + h0 + h1; hist[3 * NBIN + tid] = start + h0 + h1 + h2;
      }
      if (tid == 0) binstart[NBIN] = total;
    }
    __syncthreads();
    for (int i = i0 + lane; i < i1; i += 64) order[hist[w * NBIN + (lrec[i] & 255)] + rank[i]] = (unsigned short)i;
    __syncthreads();
    // items: parts of at most R0 records per bin, at most NPAIR in all (n / R0 + non-empty bins <= NPAIR)
    const int runlen = tid < NBIN ? binstart[tid + 1] - binstart[tid] : 0;
    const int spare = max(NPAIR - __syncthreads_count(runlen > 0), 1);
    const int R0 = max(RMIN, (n + spare - 1) / spare);
    const int nit = (runlen + R0 - 1) / R0;
    int* itab = hist;  // (the histogram is dead once `order` is written)
    int nitems;
    const int istart = block_exclusive_scan_256(nit, scratch, &nitems);
    for (int k = 0; k < nit; ++k) itab[istart + k] = tid | (k << 8);
    __syncthreads();
    const bool active = pair < nitems;
    const int item = active ? itab[pair] : 0;
    const int bin = item & 255, part_k = item >> 8;
    int s0 = binstart[bin] + part_k * R0, s1 = min(binstart[bin + 1], s0 + R0);
    if (!active) s0 = s1 = 0;
#pragma unroll
    for (int v = 0; v < 2 * V; ++v) a1[v] = a2[v] = a3[v] = a4[v] = v2f{0.f, 0.f};
#pragma unroll 1
    for (int i = s0; i < s1; i += U) {  // U samples in flight per thread, applied in list (= sample) order
      float2 xy[U];
      float aws[U];
      float4 g[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int sidx = lrec[order[min(i + u, s1 - 1)]] >> 8;
        const int q = sidx >> pshift, pp = sidx & (P - 1);
        xy[u] = *reinterpret_cast<const float2*>(locb + q * lstride + pp * 2);
        aws[u] = attb[q * astride + pp];
        const float4* row = reinterpret_cast<const float4*>(gob + (long)q * qstride);
#pragma unroll
        for (int v = 0; v < V; ++v) g[u][v] = row[v];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i + u < s1) {
          const float aw = aws[u];  // (bilinear_setup's arithmetic)
          const float h_im = msda_pix(xy[u].y, Hl), w_im = msda_pix(xy[u].x, Wl);
          const float lh = h_im - floorf(h_im), lw = w_im - floorf(w_im);
          const float hw = 1.f - lw, hh = 1.f - lh;
          const float ah = aw * hh, al = aw * lh;  // the tap weights carry the attention weight
          const float w1 = ah * hw, w2 = ah * lw, w3 = al * hw, w4 = al * lw;
          const v2f W1 = {w1, w1}, W2 = {w2, w2}, W3 = {w3, w3}, W4 = {w4, w4};
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const v2f lo = {g[u][v].x, g[u][v].y}, hi = {g[u][v].z, g[u][v].w};
            a1[2 * v] += lo * W1; a1[2 * v + 1] += hi * W1;
            a2[2 * v] += lo * W2; a2[2 * v + 1] += hi * W2;
            a3[2 * v] += lo * W3; a3[2 * v + 1] += hi * W3;
            a4[2 * v] += lo * W4; a4[2 * v + 1] += hi * W4;
          }
        }
      }
    }
    // The parts of one bin are consecutive items, i.e. neighbouring pairs.  (1) Inside a wavefront their rows are summed by a
    // suffix scan over the pairs (Hillis-Steele, shuffles; a fixed tree): the FIRST pair of a bin in each wavefront ends up
    // with the sum of the bin's parts in that wavefront.  (2) Those heads add their rows to the tile's cells — tap k of bin
    // (x, y) belongs to cell (x + (k & 1), y + (k >> 1)) — one tap at a time and, for a bin whose parts straddle wavefronts,
    // one wavefront after the other (at most four rounds): no two threads touch a cell together, and every sum runs in an
    // order the data alone fixes
    {
      constexpr int PPW = 64 / TB;  // pairs per wavefront
      const int pl = lane / TB;
      const int segid = active ? bin : -1 - pl;  // (idle pairs: segments of their own)
      int maxk = active ? part_k : 0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) maxk = max(maxk, __shfl_xor(maxk, o, 64));
      for (int d = 1; d <= maxk && d < PPW; d <<= 1) {  // (wave-uniform: a segment is at most maxk + 1 pairs long)
        const int seg_there = __shfl_down(segid, d * TB, 64);  // (by every lane: a shuffle inside `a && b` would run with the top lanes — the partners — switched off)
        const bool take = (pl + d < PPW) && seg_there == segid;
#pragma unroll
        for (int v = 0; v < 2 * V; ++v) {
          const float x1 = __shfl_down(a1[v].x, d * TB, 64), y1 = __shfl_down(a1[v].y, d * TB, 64);
          const float x2 = __shfl_down(a2[v].x, d * TB, 64), y2 = __shfl_down(a2[v].y, d * TB, 64);
          const float x3 = __shfl_down(a3[v].x, d * TB, 64), y3 = __shfl_down(a3[v].y, d * TB, 64);
          const float x4 = __shfl_down(a4[v].x, d * TB, 64), y4 = __shfl_down(a4[v].y, d * TB, 64);
          if (take) {
            a1[v] += v2f{x1, y1}; a2[v] += v2f{x2, y2}; a3[v] += v2f{x3, y3}; a4[v] += v2f{x4, y4};
          }
        }
      }
      const bool head = active && (part_k == 0 || pl == 0);
      const int round = head ? pair / PPW - (pair - part_k) / PPW : 0;  // wavefronts between the bin's first item and this one
      const int lbx = bin & (MSDA_T_TS - 1), lby = bin / MSDA_T_TS;
      float4* c = reinterpret_cast<float4*>(acc + (lby * MSDA_T_CW + lbx) * D + sub * CH);
      constexpr int CS = D / 4;  // float4 per cell
      auto add = [](float4* p, const float4& v) { float4 o = *p; o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w; *p = o; };
      for (int k = 0; __syncthreads_or(head && round >= k); ++k) {
        const bool mine = head && round == k;
        if (mine) {
#pragma unroll
          for (int v = 0; v < V; ++v) add(c + v, make_float4(a1[2 * v].x, a1[2 * v].y, a1[2 * v + 1].x, a1[2 * v + 1].y));
        }
        __syncthreads();
        if (mine) {
#pragma unroll
          for (int v = 0; v < V; ++v) add(c + CS + v, make_float4(a2[2 * v].x, a2[2 * v].y, a2[2 * v + 1].x, a2[2 * v + 1].y));
        }
        __syncthreads();
        if (mine) {
#pragma unroll
          for (int v = 0; v < V; ++v) add(c + MSDA_T_CW * CS + v, make_float4(a3[2 * v].x, a3[2 * v].y, a3[2 * v + 1].x, a3[2 * v + 1].y));
        }
        __syncthreads();
        if (mine) {
#pragma unroll
          for (int v = 0; v < V; ++v) add(c + (MSDA_T_CW + 1) * CS + v, make_float4(a4[2 * v].x, a4[2 * v].y, a4[2 * v + 1].x, a4[2 * v + 1].y));
        }
        __syncthreads();
      }
    }
  };

  // scan: only the blocks whose mask names this tile (kept in order in `blist`, a segment of MSDA_T_SEGB blocks at a
  // time); one 16-byte load of R = 4 consecutive bin words per thread and round (one barrier per 1024 records), two rounds
  // requested ahead; the kept list is in sample order (blocks ascending, thread-major inside a round = index order)
  int n = 0, it = 0;
  const int4 none = make_int4(-1, -1, -1, -1);
  const unsigned long long* msrc = mask + ((long)bh * T.L + l) * nqt;
  const int mbit = tile & 63;
  const int blk0 = c0 >> bshift, nblk = (c1 - c0 + BS - 1) >> bshift;
  const int slot = (tid * R) >> bshift, off = (tid * R) & (BS - 1), BPR = (256 * R) >> bshift;  // blocks per round
  for (int seg = 0; seg < nblk; seg += MSDA_T_SEGB) {
    const int segn = min(nblk - seg, MSDA_T_SEGB);
    int cnt = 0;
    for (int j0 = 0; j0 < segn; j0 += 256, ++it) {
      const int jj = j0 + tid;
      const bool keep = jj < segn && ((msrc[blk0 + seg + jj] >> mbit) & 1ull) != 0ull;
      const unsigned long long m = __ballot(keep);
      int* wt = wtot + (it & 1) * 4;
      if (lane == 0) wt[w] = __popcll(m);
      __syncthreads();
      const int t0 = wt[0], t1 = wt[1], t2 = wt[2], t3 = wt[3];
      if (keep) blist[cnt + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0) + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)jj;
      cnt += t0 + t1 + t2 + t3;
    }
    __syncthreads();
    auto index = [&](int rb) {  // first record of this thread in the round that starts at list position rb (-1: none)
      const int k = rb + slot;
      return k < cnt ? ((blk0 + seg + (int)blist[k]) << bshift) + off : -1;
    };
    auto fetch = [&](int i) { return i >= 0 ? *reinterpret_cast<const int4*>(bsrc + i) : none; };
    int i0 = index(0), i1 = index(BPR);
    int4 nx0 = fetch(i0), nx1 = fetch(i1);
    for (int rb = 0; rb < cnt; rb += BPR, ++it) {
      const int4 c4 = nx0;
      const int ib = i0;
      nx0 = nx1; i0 = i1;
      i1 = index(rb + 2 * BPR);
      nx1 = fetch(i1);
      const int cur[R] = {c4.x, c4.y, c4.z, c4.w};
      bool sel[R];
      int before = 0, wsum = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int bx = cur[k] & 0xffff, by = cur[k] >> 16;  // (-1: by = -1: outside every tile)
        sel[k] = ib >= 0 && cur[k] >= 0 && bx >= bx0 && bx < bx1 && by >= by0 && by < by1 && ib + k < SP;
        const unsigned long long m = __ballot(sel[k]);
        before += __popcll(m & ((1ull << lane) - 1ull));
        wsum += __popcll(m);
      }
      int* wt = wtot + (it & 1) * 4;
      if (lane == 0) wt[w] = wsum;
      __syncthreads();
      const int t0 = wt[0], t1 = wt[1], t2 = wt[2], t3 = wt[3];
      int pos = n + before + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (sel[k]) {
          const int bx = cur[k] & 0xffff, by = cur[k] >> 16;
          lrec[pos++] = ((ib + k) << 8) | ((by - by0) * MSDA_T_TS + (bx - bx0));
        }
      }
      n += t0 + t1 + t2 + t3;
      if (n > MSDA_T_CAP - 256 * R) {
        __syncthreads();
        flush(n);
        n = 0;
      }
    }
    __syncthreads();  // (blist is rebuilt)
  }
  __syncthreads();
  if (n > 0) flush(n);
  float4* dst = reinterpret_cast<float4*>(part + ((long)bh * T.NW + e) * NCELL * D);
  for (int i = tid; i < NCELL * D / 4; i += 256) dst[i] = reinterpret_cast<const float4*>(acc)[i];
}

// grad_value row of every token = the cells that alias it in the (at most four) tiles that hold it, every sample chunk, in
// fixed order.  D/4 lanes per token; workgroups mapped like msda_tile_kernel (one XCD per (b, h)).
template <int D>
__global__ __launch_bounds__(256) void msda_tile_combine_kernel(const float* __restrict__ part, float* __restrict__ grad_value,
                                                                MsdaTiles T, int Nk, int H, int BH, int bpb,
                                                                unsigned* __restrict__ amax_out) {
  constexpr int G = D / 4, TPB = 256 / G;
  constexpr int NCELL = MsdaTileGeom<D>::NCELL;
  const int x8 = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int bh = x8 + 8 * (j / bpb), blk = j % bpb;
  if (bh >= BH) return;
  const int tok = blk * TPB + threadIdx.x / G, c4 = threadIdx.x % G;
  float amx = 0.f;  // max |grad_value| of this lane -> the tensor's range word (the value projection's dX / dW operand)
  if (tok < Nk) {
    const int b = bh / H, h = bh - b * H;
    int l = 0;
    while (l + 1 < T.L && tok >= T.lsi[l + 1]) ++l;
    const int Wl = T.Wl[l], tsx = T.tsx[l], tsy = T.tsy[l], ntx = T.ntx[l], nch = T.nch[l];
    const int rr = tok - T.lsi[l], y = rr / Wl, x = rr - y * Wl;
    const int cx = x + 1, cy = y + 1;  // extended-grid cell of the token
    const int tx = cx / tsx, ty = cy / tsy, lx = cx - tx * tsx, ly = cy - ty * tsy;
    const float* base = part + ((long)bh * T.NW + T.wbase[l]) * NCELL * D + c4 * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    auto tile_cells = [&](int ttx, int tty, int ccy, int ccx) {
      const float* p = base + ((long)(tty * ntx + ttx) * nch * NCELL + ccy * MSDA_T_CW + ccx) * D;
      for (int c = 0; c < nch; ++c) {
        const float4 u = *reinterpret_cast<const float4*>(p + (long)c * NCELL * D);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
    };
    const bool hx = lx == 0 && tx > 0, hy = ly == 0 && ty > 0;  // also the halo column / row of the left / upper tile
    if (hx && hy) tile_cells(tx - 1, ty - 1, tsy, tsx);
    if (hy) tile_cells(tx, ty - 1, tsy, lx);
    if (hx) tile_cells(tx - 1, ty, ly, tsx);
    tile_cells(tx, ty, ly, lx);
    *reinterpret_cast<float4*>(grad_value + (((long)b * Nk + tok) * H + h) * D + c4 * 4) = v;
    amx = amax4(0.f, v);
  }
  amax_commit(amax_out, amx);  // (every lane of the wavefront, also those past the last token)
}

template <int D, int P>
static void launch_tiled(const MsdaBwdArgs& a, const MsdaTiles& T, char* ws, unsigned* amax_gv) {
  constexpr int QB = msda_qb(D);
  const int B = a.B, Nk = a.Nk, Nq = a.Nq, H = a.H;
  hipStream_t s = a.s;
  const int ntiles = (Nq + QB - 1) / QB;
  const int BH = B * H;
  const MsdaTileWs W = msda_tile_ws(T, BH, Nq, P, D);
  int* binw = reinterpret_cast<int*>(ws + W.binw);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(ws + W.mask);
  float* part = reinterpret_cast<float*>(ws + W.part);
  MsdaMaskGeom MG;
  for (int l = 0; l < MSDA_T_MAXL; ++l) { MG.itx[l] = 1.f / (float)T.tsx[l]; MG.ity[l] = 1.f / (float)T.tsy[l]; MG.ntx[l] = T.ntx[l]; }
  // grad_loc / grad_attn by sample + one bin word per sample + one tile mask per block of QB queries
  launch_msda_bwd_sample(a, MSDA_SAMPLE_TILE, binw, mask, &MG, 0);
  constexpr size_t lds = MsdaTileGeom<D>::lds_bytes();
  static const bool attr_set = [] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&msda_tile_kernel<D, P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return true;
  }();
  (void)attr_set;
  const unsigned bh8 = (unsigned)((BH + 7) / 8) * 8;
  int bshift = 0;
  while ((1 << bshift) < QB * P) ++bshift;
  msda_tile_kernel<D, P><<<dim3(bh8 * (unsigned)T.NW), 256, lds, s>>>(a.go, a.loc, a.attn, binw, mask, part, T, Nq, bshift, ntiles, H, BH);
  const int bpb = (Nk + 256 / (D / 4) - 1) / (256 / (D / 4));
  msda_tile_combine_kernel<D><<<dim3(bh8 * (unsigned)bpb), 256, 0, s>>>(part, a.gv, T, Nk, H, BH, bpb, amax_gv);
}

void launch_msda_bwd_tiled(const MsdaBwdArgs& a, const MsdaTiles& T, char* ws, unsigned* amax_gv) {
#define CALL(DD, PP) launch_tiled<DD, PP>(a, T, ws, amax_gv)
  RSCOTR_DISPATCH_DP(a.D, a.P, CALL)
#undef CALL
}

}  // namespace rscotr
