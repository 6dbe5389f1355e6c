// Swin (shifted-)window attention core for gfx950: everything between the qkv Linear and the
// proj Linear of mmdet's ShiftWindowMSA / WindowMSA (the Swin-T backbone the reference builds from
// configs/multi/MTL_slvlcls_swin-t-p4-w7_1x1_resisc&dior&potsdam.py:9-25 and runs at
// models/multi/multitask_learner.py:83) in ONE kernel per direction:
//   zero-pad to a multiple of 7 -> cyclic shift -> 7x7 window partition -> per (window, head)
//   softmax(q k^T / sqrt(32) + relative-position bias [+ -100 shift mask]) v -> window reverse ->
//   un-shift -> crop.
// The reference does this with F.pad, torch.roll, three reshape/permute copies, two batched
// matmuls, a gather of the bias table, two adds, a softmax and the inverse copies (~20 launches
// forward, ~40 backward per block).  Here pad/shift/partition are index arithmetic on the token
// grid, so the kernel reads the (B, H*W, 3C) output of the qkv GEMM in place and writes
// (B, H*W, C) for the proj GEMM.
//
// Upstream semantics kept: the qkv Linear acts on the zero padding too, so a pad
// token has q = k = v = qkv bias and takes part in the softmax; pad tokens are only masked from
// other regions by the shift mask; relative-position index (dy+6)*13 + (dx+6); shift is applied
// even when the map is not larger than one window.
//
// CDNA4 mapping: one 256-thread workgroup per (batch, window, head) item, persistent over items of a
// fixed head; the products run on the matrix cores (see the section header below).  Backward
// recomputes the probabilities from q, k (nothing but qkv is saved) and leaves the bias-table and
// pad-token (qkv-bias) gradients as one partial row per workgroup, folded by a second launch.
// In backward a workgroup that runs several items loads the operand tiles of the next item into
// registers before the products of the current one, and every result leaves through an LDS tile as
// 16-byte row pieces (see "Item loop of the backward" below).
#include "common.h"
#include "rscotr.h"

namespace rscotr {

constexpr int WS = 7, WN = 49, HD = 32, TBL = 169;
// per-workgroup partial row of the backward kernels: [0, TBL) bias-table gradient of the workgroup's head,
// [WATTN_PBIAS, WATTN_PBIAS + 3 HD) pad-token gradient of the head's q | k | v bias slice
constexpr int WATTN_PBIAS = 172, WATTN_PROW = WATTN_PBIAS + 3 * HD;

struct WinGeom {
  int H, W, Hp, Wp, nWw, nW, C, heads, shift;
};

struct TokPos {
  bool pad;
  long tok;   // token index inside the image (y*W + x) when !pad
  int label;  // shift-mask region label
};

__device__ __forceinline__ TokPos win_token(const WinGeom& g, int wy, int wx, int t) {
  TokPos r;
  const int ys = wy * WS + t / WS, xs = wx * WS + t % WS;  // position on the shifted, padded canvas
  int yo = ys + g.shift, xo = xs + g.shift;                // roll(-shift): shifted[y] = padded[(y+shift) % Hp]
  if (yo >= g.Hp) yo -= g.Hp;
  if (xo >= g.Wp) xo -= g.Wp;
  r.pad = (yo >= g.H) || (xo >= g.W);
  r.tok = (long)yo * g.W + xo;
  const int ry = ys < g.Hp - WS ? 0 : (ys < g.Hp - g.shift ? 1 : 2);
  const int rx = xs < g.Wp - WS ? 0 : (xs < g.Wp - g.shift ? 1 : 2);
  r.label = ry * 3 + rx;
  return r;
}

// =====================================================================================================
// Matrix cores.  The 49x49x32 products of a (window, head) are small, but on the VALU they are bound by
// wave-wide LDS broadcasts (8 ds_read_b128 per 32 FMAs, one wavefront per SIMD: measured ~590 cycles per
// key row against ~150 of FMA issue; rounds 1-6 kept that kernel and a one-wavefront matrix-core kernel as
// A/B forms).  v_mfma_f32_32x32x2_f32 runs at the same FLOP rate but takes its operands as ONE dword per
// lane and step, so the same products cost 50-64 MFMAs each:
//   S  = Q K^T          (64 x 64 x 32, both operands row-per-lane reads of [token][33] tiles)
//   O  = P V            (64 x 32 x 50)
//   dP = dO V^T, dV = P^T dO, dQ = dS K, dK = dS^T Q   in backward.
// Operand tiles are 49 rows with an odd stride (33): a lane reading row (l & 31) at a fixed channel is
// conflict-free; rows >= 49 of the 64-row MFMA tiles are clamped reads whose results are discarded or
// multiplied by the zero padding of the score matrix SP (50 x 50, row / column 49 are zeros, stride 51).
constexpr int LDT = HD + 1;   // 33
constexpr int NPD = WN + 1;   // 50: padded score dimension (index 49 = zero row / column)
constexpr int LDP = NPD + 1;  // 51

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct TileRegs {
  float4 v[(WN * (HD / 4) + 63) / 64];  // 7
};

__device__ __forceinline__ void tile_load(TileRegs& r, const float* __restrict__ src_tok0, long tok_stride,
                                          const float* __restrict__ pad_vals, const int* sTok, int lane) {
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int idx = lane + i * 64;
    r.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < WN * (HD / 4)) {
      const int t = idx >> 3, c4 = idx & 7;
      const int tok = sTok[t];
      if (tok >= 0) r.v[i] = *reinterpret_cast<const float4*>(src_tok0 + (long)tok * tok_stride + c4 * 4);
      else if (pad_vals) r.v[i] = *reinterpret_cast<const float4*>(pad_vals + c4 * 4);
    }
  }
}

__device__ __forceinline__ void tile_store(const TileRegs& r, float* dst, float scale, int lane) {
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int idx = lane + i * 64;
    if (idx < WN * (HD / 4)) {
      float* d = dst + (idx >> 3) * LDT + (idx & 7) * 4;
      d[0] = r.v[i].x * scale; d[1] = r.v[i].y * scale; d[2] = r.v[i].z * scale; d[3] = r.v[i].w * scale;
    }
  }
}

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// row of C element r held by this lane inside a 32-row tile
__device__ __forceinline__ int crow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// sum of v over the 32 lanes of a half-wave (lanes l and l^32 never mix)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// =====================================================================================================
// Four wavefronts per (window, head) item.  One wavefront per item is a chain of ~280 dependent-latency MFMAs,
// five LDS phases and a 49-step row softmax: ~50 us per item however few items there are (stages 3-4 have 600 items for
// 1024 SIMDs).  Here the 256 threads of a workgroup share one item: each wavefront stages one of the four operand tiles,
// owns one 32 x 32 tile of S, the softmax runs four lanes per row, the forward's O = P V runs on waves 0,1 (rows 0-31 /
// 32-63), and the backward products are spread as
//   waves 0,1: dP rows 0-31 / 32-63 (kept in registers) -> dS for those rows          -> dQ rows 0-31 / 32-63
//   waves 2,3: dV rows 0-31 / 32-63 (registers) -> through sV to global memory while 0,1 form dS -> dK rows 0-31 / 32-63
// so the MFMA chain of an item is 16 + 32 + 25 instead of 278 issues (dP + dV are 114 tile steps: an even four-way split
// would be 29 against these 32, so that phase is left as it is).  The relative-position-bias gradient is a GATHER
// (thread t < 169 sums dS over the <= 49 (i, j) pairs of its table entry in fixed order, in a register across the items
// of the workgroup) instead of ~64 LDS float atomics per lane and item: no atomics at all, bit-reproducible.
//
// Item loop of the backward.  (1) Prefetch: the token map of item n + 1 is written (third of three sTok / sLab slots, so the row stores of
// item n - 1 may still be reading theirs) and its operand tiles are loaded into registers (TileRegs) BEFORE the products of
// item n; they go to LDS at the end of the iteration, once the last product has read the old tiles.  The wait for them
// (wait_loads) stands BEFORE the last rows of item n are stored, so it covers the prefetch alone and those stores are not
// waited for until the end of item n + 1.  GUARD: the map and the loads of item n + 1 sit
// behind `more = bw + stride < B * nW` and nowhere else; the last item of a workgroup prefetches nothing, so no address is
// formed from an item index >= B * nW.  The staged tiles cost 28 + 8 registers; with the per-thread address arithmetic
// kept inside the loop (item_tid) the kernel still needs only 123 VGPRs and no scratch.
// (2) Results: dV / dQ / dK go from the accumulators to an LDS tile ([49][33]: the operand tiles that are dead by then,
// dV and dQ -> sV, dK -> sG) and from there to global memory as float4 pieces, eight lanes per token row like tile_load,
// with one pad / real decision per piece from sTok and max|.| for the range word folded in the same pass.  The pad-token
// (qkv-bias) sums are taken from the accumulators on their way to the tile (acc_to_tile; sPadm = the pad bits of the
// token map), per lane and in register order, and folded wave by wave at the end.  Every product and every sum keeps the
// order it had when each accumulator register was stored by its own instruction: the results are bit-identical to that
// form (which a training run, where rounding differences grow from step to step, can be compared against).
__device__ __forceinline__ void mma_rr1(f32x16& acc, const float* A, const float* B, int mi, int ni, int lane) {
  const int fr = lane & 31, fk = lane >> 5;
  const float* a = A + min(mi * 32 + fr, WN - 1) * LDT + fk;
  const float* b = B + min(ni * 32 + fr, WN - 1) * LDT + fk;
#pragma unroll
  for (int kk = 0; kk < HD; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc, 0, 0, 0);
}

__device__ __forceinline__ void mma_pt1(f32x16& acc, const float* SP, const float* T, int mi, int lane) {
  const int fr = lane & 31, fk = lane >> 5;
  const float* a = SP + min(mi * 32 + fr, WN) * LDP + fk;
#pragma unroll 5
  for (int kk = 0; kk < NPD; kk += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], T[min(kk + fk, WN - 1) * LDT + fr], acc, 0, 0, 0);
}

__device__ __forceinline__ void mma_ptT1(f32x16& acc, const float* SP, const float* T, int mi, int lane) {
  const int fr = lane & 31, fk = lane >> 5;
  const int j = min(mi * 32 + fr, WN);
#pragma unroll 5
  for (int kk = 0; kk < NPD; kk += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(SP[(kk + fk) * LDP + j], T[min(kk + fk, WN - 1) * LDT + fr], acc, 0, 0, 0);
}

__device__ __forceinline__ void store_scores1(const f32x16& acc, float* sP, const float* sT, const int* sLab, int shift,
                                              int mi, int ni, int lane) {
  const int fr = lane & 31;
  const int j = ni * 32 + fr, jc = min(j, WN - 1);
  const int jb = (6 - jc / WS) * 13 + (6 - jc % WS), jl = sLab[jc];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = mi * 32 + crow(r, lane);
    if (i >= WN || j >= WN) continue;
    const int ti = (i / WS) * 13 + i % WS;
    sP[i * LDP + j] = acc[r] + sT[ti + jb] + ((shift > 0 && jl != sLab[i]) ? -100.0f : 0.f);
  }
}

// softmax of the 49 rows of sP in place, four lanes per row (all 256 threads call it)
__device__ __forceinline__ void softmax_rows4(float* sP, int tid) {
  const int row = tid >> 2, q = tid & 3;
  float* rowp = sP + min(row, WN - 1) * LDP;
  float v[13];
  float m = -3.0e38f;
#pragma unroll
  for (int u = 0; u < 13; ++u) {
    const int j = q + 4 * u;
    v[u] = j < WN ? rowp[j] : -3.0e38f;
    m = fmaxf(m, v[u]);
  }
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < 13; ++u) {
    v[u] = (q + 4 * u < WN) ? __expf(v[u] - m) : 0.f;
    sum += v[u];
  }
  sum += __shfl_xor(sum, 1, 64);
  sum += __shfl_xor(sum, 2, 64);
  const float inv = 1.f / sum;
  if (row < WN) {
#pragma unroll
    for (int u = 0; u < 13; ++u)
      if (q + 4 * u < WN) rowp[q + 4 * u] = v[u] * inv;
  }
}

// wave w loads operand tile w of item (image b, token map sTok) into registers (0: q, 1: k, 2: v, 3: dO when `dout` is given)
__device__ __forceinline__ void stage_load(TileRegs& r, const float* __restrict__ qkv, const float* __restrict__ qkv_b,
                                           const float* __restrict__ dout, const WinGeom& g, int b, int head,
                                           const int* sTok, int w, int lane) {
  if (w == 3 && !dout) return;
  const long L = (long)g.H * g.W;
  const float* src = w == 3 ? dout + (long)b * L * g.C + head * HD : qkv + (long)b * L * 3 * g.C + head * HD + w * g.C;
  const long tstride = w == 3 ? g.C : 3 * g.C;
  const float* padv = (w == 3 || !qkv_b) ? nullptr : qkv_b + w * g.C + head * HD;
  tile_load(r, src, tstride, padv, sTok, lane);
}

// ... and writes it to its LDS tile (q scaled)
__device__ __forceinline__ void stage_store(const TileRegs& r, float* sQ, float* sK, float* sV, float* sG, float scale,
                                            int w, int lane) {
  if (w == 3 && !sG) return;
  float* dst = w == 0 ? sQ : (w == 1 ? sK : (w == 2 ? sV : sG));
  tile_store(r, dst, w == 0 ? scale : 1.f, lane);
}

// wave w stages operand tile w of the item at once (the forward's loop; 0: q * scale, 1: k, 2: v)
__device__ __forceinline__ void stage_item_tiles(float* sQ, float* sK, float* sV, float* sG, const float* base,
                                                 const float* __restrict__ qkv_b, const float* dout_b, const WinGeom& g,
                                                 int head, const int* sTok, float scale, int w, int lane) {
  if (w == 3 && !dout_b) return;
  const float* src = w == 3 ? dout_b : base + w * g.C;
  const long tstride = w == 3 ? g.C : 3 * g.C;
  const float* padv = (w == 3 || !qkv_b) ? nullptr : qkv_b + w * g.C + head * HD;
  float* dst = w == 0 ? sQ : (w == 1 ? sK : (w == 2 ? sV : sG));
  TileRegs r;
  tile_load(r, src, tstride, padv, sTok, lane);
  tile_store(r, dst, w == 0 ? scale : 1.f, lane);
}

// Thread index as the item loop sees it: opaque to the optimiser, so that the per-thread address arithmetic of an item
// (LDS tile offsets, row-piece indices, operand rows) is redone per item instead of being hoisted out of the loop and held
// in registers across it: hoisted, the backward needs > 256 VGPRs and spills; inside the loop it needs ~125, no scratch.
__device__ __forceinline__ int item_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// every vector-memory operation of this wavefront has completed (vmcnt(0); the other counters are left alone).  Stated on
// every path, where the compiler's own wait would sit inside the branch of the loading wavefronts only and a second one
// would follow on the merged path, behind the row stores.
__device__ __forceinline__ void wait_loads() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// token map of item bw (threads 0..48, all in wave 0): sTok = token index inside the image or -1 for a pad token,
// sLab = shift-mask label; padm[0..1] = bit t of the 64-bit word: token t is a pad token
__device__ __forceinline__ void token_map(const WinGeom& g, int bw, int* sLab, int* sTok, unsigned* padm, int tid) {
  if (tid >= 64) return;
  const int win = bw % g.nW;
  const TokPos me = win_token(g, win / g.nWw, win % g.nWw, min(tid, WN - 1));
  const unsigned long long pads = __ballot(tid < WN && me.pad);
  if (tid < WN) {
    sLab[tid] = me.label;
    sTok[tid] = me.pad ? -1 : (int)me.tok;
  }
  if (tid == 0) {
    padm[0] = (unsigned)pads;
    padm[1] = (unsigned)(pads >> 32);
  }
}

// accumulator of a 32-row tile (rows mi * 32 + crow, column lane & 31) -> result tile sO[49][LDT]; the rows of pad tokens
// (bits of `pads`) are also added to `pad_acc`, element by element in register order: the summation order of the pad-token
// (qkv-bias) gradient is that of the accumulator layout, item after item
__device__ __forceinline__ void acc_to_tile(const f32x16& acc, float* sO, float scale, int mi, int lane,
                                            unsigned long long pads, float& pad_acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = mi * 32 + crow(r, lane);
    if (i < WN) {
      sO[i * LDT + (lane & 31)] = acc[r] * scale;
      if ((pads >> i) & 1ull) pad_acc += acc[r] * scale;
    }
  }
}

// rows of a result tile -> global memory: piece idx (< 49 * 8) is channels 4 (idx & 7) .. + 3 of token row idx >> 3;
// dst_tok0 = channel 0 of token 0 of this head in the image.  Pad rows are skipped.  Returns max |.| of what was stored.
__device__ __forceinline__ float tile_row_piece(const float* sO, float* __restrict__ dst_tok0, long tok_stride,
                                                const int* sTok, int idx, float amx) {
  const int t = idx >> 3, c4 = idx & 7;
  const int tok = sTok[t];
  if (tok >= 0) {
    const float* s = sO + t * LDT + c4 * 4;
    const float4 v = make_float4(s[0], s[1], s[2], s[3]);
    *reinterpret_cast<float4*>(dst_tok0 + (long)tok * tok_stride + c4 * 4) = v;
    amx = fmaxf(fmaxf(amx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  return amx;
}

__global__ __launch_bounds__(256) void swin_wattn_fwd_mfma4_kernel(const float* __restrict__ qkv,
                                                                   const float* __restrict__ qkv_b,
                                                                   const float* __restrict__ table,
                                                                   float* __restrict__ out, WinGeom g, int B,
                                                                   unsigned* __restrict__ amax_out) {
  // The forward keeps the plain loop (map, gather, products, per-register stores): with O = P V on the two wavefronts whose
  // summation order the results are defined by, the prefetched loop and the LDS row stores of the backward measured 1-3 us
  // SLOWER here at stages 1-2 and level at stages 3-4 (profiles/README.md); this kernel already runs four workgroups per CU.
  __shared__ float sQ[WN * LDT], sK[WN * LDT], sV[WN * LDT];
  __shared__ float sP[NPD * LDP];
  __shared__ float sT[TBL];
  __shared__ int sLab[WN], sTok[WN];
  float amx = 0.f;  // max |out| -> the output's range word (the proj Linear multiplies with it)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int head = blockIdx.x % g.heads;
  const int stride = gridDim.x / g.heads;
  const float scale = 0.17677669529663687f;
  const long L = (long)g.H * g.W;
  for (int t = tid; t < TBL; t += 256) sT[t] = table[t * g.heads + head];
  for (int t = tid; t < NPD * LDP; t += 256) sP[t] = 0.f;  // the padding row / column stay zero
  for (int bw = blockIdx.x / g.heads; bw < B * g.nW; bw += stride) {
    const int b = bw / g.nW, win = bw % g.nW, wy = win / g.nWw, wx = win % g.nWw;
    __syncthreads();
    if (tid < WN) {
      const TokPos me = win_token(g, wy, wx, tid);
      sLab[tid] = me.label;
      sTok[tid] = me.pad ? -1 : (int)me.tok;
    }
    __syncthreads();
    stage_item_tiles(sQ, sK, sV, nullptr, qkv + (long)b * L * 3 * g.C + head * HD, qkv_b, nullptr, g, head, sTok, scale, w, lane);
    __syncthreads();
    {
      f32x16 a;
      zero16(a);
      mma_rr1(a, sQ, sK, w >> 1, w & 1, lane);
      store_scores1(a, sP, sT, sLab, g.shift, w >> 1, w & 1, lane);
    }
    __syncthreads();
    softmax_rows4(sP, tid);
    __syncthreads();
    if (w < 2) {  // O rows 32 w .. 32 w + 31
      f32x16 o;
      zero16(o);
      mma_pt1(o, sP, sV, w, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = w * 32 + crow(r, lane);
        if (i < WN) {
          const int tok = sTok[i];
          if (tok >= 0) { out[((long)b * L + tok) * g.C + head * HD + (lane & 31)] = o[r]; amx = fmaxf(amx, fabsf(o[r])); }
        }
      }
    }
  }
  amax_commit(amax_out, amx);
}

// rows of the forward output for delta (four lanes per row, 8 channels each); zeros for pad rows and without `outp`
__device__ __forceinline__ void delta_rows_load(float4& o_a, float4& o_b, const float* __restrict__ outp, const WinGeom& g,
                                                int b, int head, const int* sTok, int tid) {
  o_a = make_float4(0.f, 0.f, 0.f, 0.f);
  o_b = o_a;
  if (outp && (tid >> 2) < WN) {
    const int tok = sTok[tid >> 2];
    if (tok >= 0) {
      const float4* o4 =
          reinterpret_cast<const float4*>(outp + ((long)b * g.H * g.W + tok) * g.C + head * HD + (tid & 3) * 8);
      o_a = o4[0];
      o_b = o4[1];
    }
  }
}

__device__ __forceinline__ void swin_wattn_bwd_mfma4_body(const float* __restrict__ qkv,
                                                                   const float* __restrict__ qkv_b,
                                                                   const float* __restrict__ table,
                                                                   const float* __restrict__ dout,
                                                                   const float* __restrict__ outp,
                                                                   float* __restrict__ dqkv, float* __restrict__ part,
                                                                   const WinGeom& g, int B, unsigned* __restrict__ amax_out) {
  __shared__ float sQ[WN * LDT], sK[WN * LDT], sV[WN * LDT], sG[WN * LDT];
  __shared__ float sP[NPD * LDP];
  __shared__ float sT[TBL];
  float amx = 0.f;  // max |dqkv| of what this lane stores -> the gradient's range word (common.h: amax_commit)
  __shared__ float sDelta[64];
  __shared__ int sLab[3][WN], sTok[3][WN];
  __shared__ unsigned sPadm[3][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 31;
  const int head = blockIdx.x % g.heads;
  const int stride = gridDim.x / g.heads;
  const int nitem = B * g.nW;
  const float scale = 0.17677669529663687f;
  const long L = (long)g.H * g.W;
  float* prow = part + (long)blockIdx.x * WATTN_PROW;
  int bw = blockIdx.x / g.heads;
  float dT = 0.f;    // thread t < 169: gradient of table entry t over this workgroup's items
  float accB[3] = {0.f, 0.f, 0.f};  // pad-token sums of this lane's rows: dq (waves 0,1), dk, dv (waves 2,3), column fr
  if (bw < nitem) {  // (always with wattn_grid)
    for (int t = tid; t < TBL; t += 256) sT[t] = table[t * g.heads + head];
    for (int t = tid; t < NPD * LDP; t += 256) sP[t] = 0.f;
    token_map(g, bw, sLab[0], sTok[0], sPadm[0], tid);
    __syncthreads();
  }
  const int tdy = tid / 13 - 6, tdx = tid % 13 - 6;
  const int iy0 = max(0, tdy), iy1 = min(6, 6 + tdy), ix0 = max(0, tdx), ix1 = min(6, 6 + tdx);
  TileRegs pre;
  float4 o_a, o_b;
  if (bw < nitem) {
    stage_load(pre, qkv, qkv_b, dout, g, bw / g.nW, head, sTok[0], w, lane);
    delta_rows_load(o_a, o_b, outp, g, bw / g.nW, head, sTok[0], tid);
    wait_loads();
    stage_store(pre, sQ, sK, sV, sG, scale, w, lane);
  }
  int cur = 0;
  for (; bw < nitem; bw += stride) {
    const int b = bw / g.nW;
    const int nxt = cur == 2 ? 0 : cur + 1;
    const bool more = bw + stride < nitem;  // the ONLY gate of anything indexed by the next item
    const int* tok_cur = sTok[cur];
    const unsigned long long pads = sPadm[cur][0] | ((unsigned long long)sPadm[cur][1] << 32);  // (uniform)
    const int tid = item_tid(), lane = tid & 63, w = tid >> 6, fr = lane & 31;
    // delta_i = sum_j P_ij dP_ij = dO_i . O_i (O = the forward output of this head): with the forward output at hand
    // it is a 32-channel dot product per row (four lanes per row) instead of a cross-lane reduction per dS row
    const float4 c_a = o_a, c_b = o_b;
    if (more) token_map(g, bw + stride, sLab[nxt], sTok[nxt], sPadm[nxt], tid);
    __syncthreads();
    if (more) {
      stage_load(pre, qkv, qkv_b, dout, g, (bw + stride) / g.nW, head, sTok[nxt], w, lane);
      delta_rows_load(o_a, o_b, outp, g, (bw + stride) / g.nW, head, sTok[nxt], tid);
    }
    float* dq_base = dqkv + (long)b * L * 3 * g.C + head * HD;
    if (outp) {
      const float* gq = sG + min(tid >> 2, WN - 1) * LDT + (tid & 3) * 8;
      float d = ((c_a.x * gq[0] + c_a.y * gq[1]) + (c_a.z * gq[2] + c_a.w * gq[3])) +
                ((c_b.x * gq[4] + c_b.y * gq[5]) + (c_b.z * gq[6] + c_b.w * gq[7]));
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      if ((tid & 3) == 0) sDelta[tid >> 2] = d;  // (read after the barriers below)
    }
    {  // ---- 1. S tile (w >> 1, w & 1) -> sP
      f32x16 a;
      zero16(a);
      mma_rr1(a, sQ, sK, w >> 1, w & 1, lane);
      store_scores1(a, sP, sT, sLab[cur], g.shift, w >> 1, w & 1, lane);
    }
    __syncthreads();
    softmax_rows4(sP, tid);
    __syncthreads();
    // ---- 2. waves 0,1: dP rows of tile w (both column tiles, registers); waves 2,3: dV rows of tile w - 2 (registers)
    f32x16 dp[2];
    if (w < 2) {
      zero16(dp[0]); zero16(dp[1]);
      mma_rr1(dp[0], sG, sV, w, 0, lane);
      mma_rr1(dp[1], sG, sV, w, 1, lane);
    } else {
      zero16(dp[0]);
      mma_ptT1(dp[0], sP, sG, w - 2, lane);
    }
    __syncthreads();  // P has been consumed as an MFMA operand before the rows overwrite it with dS
    if (w < 2) {      // ---- 3. delta_i = sum_j P_ij dP_ij, dS = P (dP - delta) -> sP
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = w * 32 + crow(r, lane);  // same row for the 32 lanes of a half-wave
        const bool iv = i < WN;
        const int j0 = fr, j1 = 32 + fr;
        const float p0 = iv ? sP[i * LDP + j0] : 0.f;
        const float p1 = (iv && j1 < WN) ? sP[i * LDP + j1] : 0.f;
        const float delta = outp ? sDelta[min(i, 63)] : half_sum(p0 * dp[0][r] + p1 * dp[1][r]);
        if (iv) {
          sP[i * LDP + j0] = p0 * (dp[0][r] - delta);
          if (j1 < WN) sP[i * LDP + j1] = p1 * (dp[1][r] - delta);
        }
      }
    } else {  // ... meanwhile waves 2,3 send the dV rows out through sV (dead: dP is done).  Each of the two reads back
      // only the rows it wrote itself (32 (w - 2) .. + 31), so no barrier stands between its LDS writes and reads
      acc_to_tile(dp[0], sV, 1.f, w - 2, lane, pads, accB[2]);
      const int p0 = (w - 2) * 32 * (HD / 4) + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p0 + i * 64 < WN * (HD / 4)) amx = tile_row_piece(sV, dq_base + 2 * g.C, 3 * g.C, tok_cur, p0 + i * 64, amx);
    }
    __syncthreads();
    if (w < 2) {  // ---- 4. dQ = scale * dS K   (rows = query i) -> sV (the dV rows left it before the barrier above)
      f32x16 dq;
      zero16(dq);
      mma_pt1(dq, sP, sK, w, lane);
      acc_to_tile(dq, sV, scale, w, lane, pads, accB[0]);
    } else {      // ---- 5. dK = dS^T (q * scale)   (rows = key j; sQ already holds q * scale) -> sG (dead since dP / dV)
      f32x16 dk;
      zero16(dk);
      mma_ptT1(dk, sP, sQ, w - 2, lane);
      acc_to_tile(dk, sG, 1.f, w - 2, lane, pads, accB[1]);
    }
    __syncthreads();
    // the wait for the prefetched tiles stands BEFORE the dQ / dK rows are stored: it covers the prefetch (and the dV rows,
    // two phases old), and these stores stay in flight through the next item
    wait_loads();
#pragma unroll
    for (int i = 0; i < 2; ++i)  // dQ rows, dK rows
      if (tid + i * 256 < WN * (HD / 4)) {
        amx = tile_row_piece(sV, dq_base, 3 * g.C, tok_cur, tid + i * 256, amx);
        amx = tile_row_piece(sG, dq_base + g.C, 3 * g.C, tok_cur, tid + i * 256, amx);
      }
    __syncthreads();  // sV / sG have been read: the tiles of the next item may replace them
    if (more) stage_store(pre, sQ, sK, sV, sG, scale, w, lane);
    if (tid < TBL) {  // bias-table gradient: entry (dy, dx) = sum of dS over the pairs i - j = (dy, dx), fixed order
      // (constant trip counts + predicates: the 49 LDS reads are issued together instead of one dependent read per add;
      // sP keeps dS until the S tiles of the next item, which are behind the next barrier)
      float acc7 = 0.f;
#pragma unroll 1
      for (int iy = iy0; iy <= iy1; ++iy) {  // (seven reads in flight per row of the window: registers)
        float v[WS];
#pragma unroll
        for (int ix = 0; ix < WS; ++ix) {
          const bool ok = ix >= ix0 && ix <= ix1;
          v[ix] = ok ? sP[(iy * WS + ix) * LDP + (iy - tdy) * WS + (ix - tdx)] : 0.f;
        }
        acc7 += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + v[6]);
      }
      dT += acc7;
    }
    cur = nxt;
  }
  // this workgroup's share of the bias-table / pad-token (qkv-bias) gradients: one partial row, folded over the
  // workgroups of the head in fixed order by wattn_param_fold_kernel
  __syncthreads();  // (the table gather of the last item has read sP: its memory now carries the fold of the pad-token sums)
  float(*sBw)[3 * HD] = reinterpret_cast<float(*)[3 * HD]>(sP);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float other = __shfl_xor(accB[k], 32, 64);
    if (lane < 32) sBw[w][k * HD + fr] = accB[k] + other;
  }
  __syncthreads();
  if (tid < TBL) prow[tid] = dT;
  if (tid < 3 * HD) prow[WATTN_PBIAS + tid] = ((sBw[0][tid] + sBw[1][tid]) + sBw[2][tid]) + sBw[3][tid];
  amax_commit(amax_out, amx);
}

// Resident workgroups per CU = wavefronts per SIMD: four.  123 VGPRs without scratch and 37.5 KB of LDS allow it; that is
// why the results leave through the dead operand tiles (sV, sG) and not through tiles of their own (50 KB: three per CU).
// Measured per stage (profiles/README.md), two -> three -> four per CU: level where every workgroup has one item and fits
// anyway (stages 3, 4 of Swin-T at 512^2); 80 -> 76 -> 60 us and 52 -> 44 -> 40 us where workgroups loop (stages 1, 2).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void swin_wattn_bwd_mfma4_kernel(
    const float* __restrict__ qkv, const float* __restrict__ qkv_b, const float* __restrict__ table,
    const float* __restrict__ dout, const float* __restrict__ outp, float* __restrict__ dqkv, float* __restrict__ part,
    WinGeom g, int B, unsigned* __restrict__ amax_out) {
  swin_wattn_bwd_mfma4_body(qkv, qkv_b, table, dout, outp, dqkv, part, g, B, amax_out);
}

static int wattn_geom(const char* fn, WinGeom* g, int B, int H, int W, int C, int heads, int ws, int shift) {
  if (B < 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0)
    return fail(RSCOTR_E_SHAPE, "%s: bad shape B=%d H=%d W=%d C=%d heads=%d", fn, B, H, W, C, heads);
  if (ws != WS) return fail(RSCOTR_E_SHAPE, "%s: window size %d (only 7 is built)", fn, ws);
  if (C != heads * HD) return fail(RSCOTR_E_SHAPE, "%s: C=%d must be heads*32 (heads=%d)", fn, C, heads);
  if (shift < 0 || shift >= WS) return fail(RSCOTR_E_SHAPE, "%s: shift %d outside [0,7)", fn, shift);
  g->H = H; g->W = W; g->C = C; g->heads = heads; g->shift = shift;
  g->Hp = (H + WS - 1) / WS * WS;
  g->Wp = (W + WS - 1) / WS * WS;
  g->nWw = g->Wp / WS;
  g->nW = (g->Hp / WS) * g->nWw;
  return RSCOTR_OK;
}

static int wattn_grid(const WinGeom& g, int B, int per_cu) {
  const long items = (long)B * g.nW;                       // windows per head
  long per_head = std::min<long>(items, std::max<long>(1, (256L * per_cu) / g.heads));
  return (int)(per_head * g.heads);
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_swin_wattn_fwd(const float* qkv, const float* qkv_bias, const float* bias_table,
                                     float* out, int B, int H, int W, int C, int heads, int ws, int shift,
                                     uint32_t* amax_out, void* stream) {
  WinGeom g;
  if (int e = wattn_geom("rscotr_swin_wattn_fwd", &g, B, H, W, C, heads, ws, shift)) return e;
  if (B == 0) return RSCOTR_OK;
  if (!qkv || !bias_table || !out) return fail(RSCOTR_E_ARG, "rscotr_swin_wattn_fwd: null pointer");
  if (!aligned16(qkv) || !aligned16(out) || (qkv_bias && !aligned16(qkv_bias)))
    return fail(RSCOTR_E_ALIGN, "rscotr_swin_wattn_fwd: pointers must be 16-byte aligned");
  // algorithmic work: q k^T and P v of every (image, window, head) on the 49 real tokens: 4 * 49 * 49 * 32 flop
  const double items = (double)B * ((H + ws - 1) / ws) * ((W + ws - 1) / ws) * heads;
  ProfScope prof(PROF_MFMA, items * 4.0 * 49 * 49 * 32, (hipStream_t)stream, "rscotr::swin_wattn_fwd_kernel");
  swin_wattn_fwd_mfma4_kernel<<<wattn_grid(g, B, 4), 256, 0, (hipStream_t)stream>>>(qkv, qkv_bias, bias_table, out, g, B, amax_out);
  return check_launch("rscotr_swin_wattn_fwd");
}

// workgroups per head of the backward launch (the partial rows of a head are rows head, head + heads, ...)
static int wattn_bwd_grid(const WinGeom& g, int B) { return wattn_grid(g, B, 4); }

namespace rscotr {
// grid (ceil(WATTN_PROW / 64), heads): column block x head; the 4 wavefronts take the head's partial rows round-robin,
// fold through LDS in fixed order, and ADD into dtable[t][head] / dqkv_b[k * C + head * HD + c].
__global__ __launch_bounds__(256) void wattn_param_fold_kernel(const float* __restrict__ part, float* __restrict__ dtable,
                                                               float* __restrict__ dqkv_b, int heads, int C, int rows) {
  __shared__ float red[3][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane, head = blockIdx.y;
  float a = 0.f;
  if (col < WATTN_PROW) {
#pragma unroll 8
    for (int r = w; r < rows; r += 4) a += part[((long)r * heads + head) * WATTN_PROW + col];
  }
  if (w > 0) red[w - 1][lane] = a;
  __syncthreads();
  if (w != 0 || col >= WATTN_PROW) return;
  a += red[0][lane];
  a += red[1][lane];
  a += red[2][lane];
  if (col < TBL) {
    if (dtable) dtable[col * heads + head] += a;
  } else if (col >= WATTN_PBIAS && dqkv_b) {
    const int t = col - WATTN_PBIAS;
    dqkv_b[(t / HD) * C + head * HD + (t % HD)] += a;
  }
}

// The same fold for ALL pending window-attention backward passes of a backward pass in one launch
// (rscotr_swin_wattn_flush): grid (ceil(WATTN_PROW / 64), total heads); table rows {partial rows, dtable | 0,
// dqkv_bias | 0, heads, C, rows per head, first head of this entry in the grid}.
__global__ __launch_bounds__(256) void wattn_param_flush_kernel(const int64_t* __restrict__ table, int n) {
  __shared__ float red[3][64];
  int e = 0;
  while (e + 1 < n && (int)table[(long)(e + 1) * 16 + 6] <= (int)blockIdx.y) ++e;
  const int64_t* t = table + (long)e * 16;
  const float* part = reinterpret_cast<const float*>(t[0]);
  float* dtable = reinterpret_cast<float*>(t[1]);
  float* dqkv_b = reinterpret_cast<float*>(t[2]);
  const int heads = (int)t[3], C = (int)t[4], rows = (int)t[5], head = (int)blockIdx.y - (int)t[6];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  float a = 0.f;
  if (col < WATTN_PROW) {
#pragma unroll 8
    for (int r = w; r < rows; r += 4) a += part[((long)r * heads + head) * WATTN_PROW + col];
  }
  if (w > 0) red[w - 1][lane] = a;
  __syncthreads();
  if (w != 0 || col >= WATTN_PROW) return;
  a += red[0][lane];
  a += red[1][lane];
  a += red[2][lane];
  if (col < TBL) {
    if (dtable) dtable[col * heads + head] += a;
  } else if (col >= WATTN_PBIAS && dqkv_b) {
    const int c = col - WATTN_PBIAS;
    dqkv_b[(c / HD) * C + head * HD + (c % HD)] += a;
  }
}
}  // namespace rscotr

// table: device (n, 16) int64 rows {partial rows left by rscotr_swin_wattn_bwd(dqkv_bias = dbias_table = NULL), dbias_table | 0,
// dqkv_bias | 0, heads, C, rows per head (= workspace bytes / (heads * WATTN_PROW * 4)), first grid row of the entry (running
// sum of heads), 0 ...}; total_heads = sum of heads.  The destinations are ADDED to.
extern "C" int rscotr_swin_wattn_flush(const int64_t* table, int n, int total_heads, void* stream) {
  if (n < 0 || total_heads < 0) return fail(RSCOTR_E_SHAPE, "rscotr_swin_wattn_flush: negative count");
  if (n == 0 || total_heads == 0) return RSCOTR_OK;
  if (!table) return fail(RSCOTR_E_ARG, "rscotr_swin_wattn_flush: null table");
  wattn_param_flush_kernel<<<dim3((WATTN_PROW + 63) / 64, (unsigned)total_heads), 256, 0, (hipStream_t)stream>>>(table, n);
  return check_launch("rscotr_swin_wattn_flush");
}

extern "C" int64_t rscotr_swin_wattn_bwd_workspace(int B, int H, int W, int C, int heads) {
  WinGeom g;
  if (B <= 0 || wattn_geom("rscotr_swin_wattn_bwd_workspace", &g, B, H, W, C, heads, WS, 0)) return 0;
  return (int64_t)wattn_bwd_grid(g, B) * WATTN_PROW * 4;
}

extern "C" int rscotr_swin_wattn_bwd(const float* qkv, const float* qkv_bias, const float* bias_table,
                                     const float* dout, float* dqkv, float* dqkv_bias, float* dbias_table,
                                     int B, int H, int W, int C, int heads, int ws, int shift, const float* out,
                                     float* workspace, int64_t workspace_bytes, uint32_t* amax_out, void* stream) {
  WinGeom g;
  if (int e = wattn_geom("rscotr_swin_wattn_bwd", &g, B, H, W, C, heads, ws, shift)) return e;
  if (B == 0) return RSCOTR_OK;
  if (!qkv || !bias_table || !dout || !dqkv) return fail(RSCOTR_E_ARG, "rscotr_swin_wattn_bwd: null pointer");
  if (!aligned16(qkv) || !aligned16(dout) || !aligned16(dqkv) || (qkv_bias && !aligned16(qkv_bias)))
    return fail(RSCOTR_E_ALIGN, "rscotr_swin_wattn_bwd: pointers must be 16-byte aligned");
  const int nwg = wattn_bwd_grid(g, B);
  if (!workspace || workspace_bytes < (int64_t)nwg * WATTN_PROW * 4)
    return fail(RSCOTR_E_ARG, "rscotr_swin_wattn_bwd: workspace of rscotr_swin_wattn_bwd_workspace() bytes required");
  hipStream_t s = (hipStream_t)stream;
  // algorithmic work: S = q k^T (recomputed), dP = dO v^T, dV = P^T dO, dQ = dS k, dK = dS^T q: 10 * 49 * 49 * 32 flop per item
  const double items = (double)B * ((H + ws - 1) / ws) * ((W + ws - 1) / ws) * heads;
  ProfScope prof(PROF_MFMA, items * 10.0 * 49 * 49 * 32, s, "rscotr::swin_wattn_bwd_kernel");
  const float* o = (out && aligned16(out)) ? out : nullptr;
  swin_wattn_bwd_mfma4_kernel<<<nwg, 256, 0, s>>>(qkv, qkv_bias, bias_table, dout, o, dqkv, workspace, g, B, amax_out);
  if (dbias_table || dqkv_bias)
    wattn_param_fold_kernel<<<dim3((WATTN_PROW + 63) / 64, heads), 256, 0, s>>>(workspace, dbias_table, dqkv_bias, heads, C,
                                                                              nwg / heads);
  return check_launch("rscotr_swin_wattn_bwd");
}
