// Fused bilinear-upsample + softmax + Lovasz-softmax loss for the seg head (gfx950): mmseg 0.28 LovaszLoss,
// loss_type='multi_class', as BaseDecodeHead.losses reaches it, on a segmented device sort.
//
//   u = resize(seg_logit (B,C,h,w), size=label.shape, mode='bilinear', align_corners=False);  p = softmax(u, dim=1)
//   a SEGMENT is one class slot over the valid pixels (label != ignore_index) of the batch, or of one image (per_image);
//   fg_i = [label_i == c]  (a label outside [0, C) is background for every class),  e_i = |fg_i - p_i,c|
//   e sorted descending, equal errors by ascending flat pixel index (a stable sort);  G = sum fg,  F_k the foreground count
//   among the first k + 1 sorted elements:
//     I_k = G - F_k,  U_k = G + (k + 1 - F_k),   g_k = 1 / U_k (foreground) | I_k / (U_k (U_k - 1)) (background)
//     (G == 0: g_0 = 1, every other g_k = 0),    loss_seg = sum_k e_(k) g_k,     d loss_seg / d p_i,c = -+ g_rank(i)
//   loss = loss_weight * mean over the summed segments of class_weight[c] loss_seg  (per_image: per image, then mean | sum)
//   A segment is summed when it has a valid pixel and (not `present` or G > 0).
//
// Forward launches (all grids fixed by the shape: the op captures into a hipGraph; a segment that is not summed returns at the
// top of every sort / scan workgroup on the device flag):
//   upsample_lovasz_key_kernel     one thread per pixel, a workgroup stays inside one image: log-sum-exp (saved), then per class
//                                  slot the sort key 0xFFFFFFFE - bits(e) (a non-negative float orders as its bits; ascending on
//                                  this key is descending on e; an ignored pixel gets 0xFFFFFFFF and ranks behind every valid
//                                  one) and the payload {flat pixel index, fg in bit 31}; G and the valid count per segment as
//                                  integer sums
//   upsample_lovasz_plan_kernel    which segments are summed, their coefficient loss_weight * class_weight / #summed (/ B), the
//                                  class -> slot table of backward
//   4 x { lovasz_sort_hist_kernel  LSD radix sort, 8 bits a pass: a wavefront counts the digits of its tile of LOV_TILE
//         lovasz_sort_scan_kernel  elements (integer LDS atomics); one workgroup per segment turns the [digit][tile] counts
//         lovasz_sort_scatter_kernel }  into offsets; a wavefront re-reads its tile 64 elements at a time in order, ranks equal
//                                  digits by lane (ballots), and scatters: stable
//   lovasz_fg_count_kernel         foreground count of every LOV_SCAN elements of the sorted valid prefix
//   lovasz_apply_kernel            F_k from the counts before the tile + ballots, g_k in closed form from the integer counts
//                                  (fp64), the tile's sum of e g in fixed order, D = -+ g_k * coefficient scattered through the
//                                  payload index into the (slot, B*H*W) plane: each cell once, never for an ignored pixel
//   upsample_lovasz_final_kernel   the segments' tile sums folded in fixed order (fp64) into loss[0]
// Backward: upsample_lovasz_s_kernel writes S(pix) = sum_slots p_c D_c over the summed segments, then the blocked gather of
// seg_upsample.h with the term p_c (D_c - S), D_c read through the pixel index (Term::PIXEL); ignored pixels and segments that
// were not summed are never read.
// No float atomics, every float sum in a fixed order: two runs are bit-equal.  Nothing synchronises with the host.
#include <algorithm>

#include "seg_upsample.h"

namespace rscotr {

constexpr int LOV_TILE = 2048;                    // elements a wavefront ranks: one histogram column of a sort pass
constexpr int LOV_WG_TILES = 4;                   // wavefronts of a sort workgroup
constexpr int LOV_WG = LOV_TILE * LOV_WG_TILES;   // elements of a sort workgroup
constexpr int LOV_SCAN = 2048;                    // elements of a scan workgroup (8 rounds of 256)
constexpr int LOV_CHUNKS = 128;                   // key-pass workgroups per image at most
static_assert(LOV_TILE % 64 == 0 && LOV_SCAN % 256 == 0, "whole rounds");

// The buffers carved out of the caller's workspace
struct LovWs {
  uint32_t *keyA, *keyB, *payA, *payB, *hist, *fgcnt;
  double* lpart;
  int *segG, *segNV;
  float* segcoef;
  int64_t bytes;
};

static LovWs lovasz_carve(void* base, int nslots, long N, int nseg, long L) {
  const long ntile = (L + LOV_TILE - 1) / LOV_TILE, nscan = (L + LOV_SCAN - 1) / LOV_SCAN;
  char* p = static_cast<char*>(base);
  auto take = [&](int64_t n) { char* r = p; p += (n + 255) / 256 * 256; return r; };
  LovWs ws;
  ws.keyA = (uint32_t*)take((int64_t)nslots * N * 4);
  ws.keyB = (uint32_t*)take((int64_t)nslots * N * 4);
  ws.payA = (uint32_t*)take((int64_t)nslots * N * 4);
  ws.payB = (uint32_t*)take((int64_t)nslots * N * 4);
  ws.hist = (uint32_t*)take((int64_t)nseg * 256 * ntile * 4);
  ws.fgcnt = (uint32_t*)take((int64_t)nseg * nscan * 4);
  ws.lpart = (double*)take((int64_t)nseg * nscan * 8);
  ws.segG = (int*)take((int64_t)nseg * 2 * 4);  // G | valid count: one memset
  ws.segNV = ws.segG + nseg;
  ws.segcoef = (float*)take((int64_t)nseg * 4);
  ws.bytes = p - static_cast<char*>(base);
  return ws;
}

__global__ __launch_bounds__(256) void upsample_lovasz_key_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                  const int* __restrict__ slots, float* __restrict__ lse,
                                                                  uint32_t* __restrict__ key, uint32_t* __restrict__ pay,
                                                                  int* segG, int* segNV, int C, int nslots, int h, int w, int H,
                                                                  int W, int ignore, int per_image, int nchunk, long N) {
  extern __shared__ int lov_cnt[];  // [nslots] foreground counts of this workgroup, [nslots]: its valid count
  const int b = blockIdx.x / nchunk, k = blockIdx.x % nchunk;
  const int HW = H * W, tid = threadIdx.x, lane = tid & 63;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const float* base = logit + (long)b * C * h * w;
  const int64_t* lab_b = label + (long)b * HW;
  const int step = nchunk * 256;
  const long L = per_image ? (long)HW : N;
  for (int i = tid; i <= nslots; i += 256) lov_cnt[i] = 0;
  __syncthreads();
  for (int i0 = k * 256; i0 < HW; i0 += step) {  // (uniform trip count: the ballots below see whole wavefronts)
    const int i = i0 + tid;
    const bool in = i < HW;
    const int ii = min(i, HW - 1);
    const Taps taps(ii / W, ii % W, sy, sx, h, w);
    const long lab = lab_b[ii];
    const bool valid = in && lab != ignore;
    float m = -3.0e38f, s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = taps.at(base + (long)c * h * w);
      if (v > m) { s = s * __expf(m - v) + 1.f; m = v; }
      else s += __expf(v - m);
    }
    const float l = m + __logf(s);
    if (in) lse[(long)b * HW + i] = l;
    const unsigned long long vb = __ballot(valid);
    if (lane == 0 && vb) atomicAdd(&lov_cnt[nslots], __popcll(vb));
    const long gp = (long)b * HW + ii;
    const long local = per_image ? (long)ii : gp;
    for (int sl = 0; sl < nslots; ++sl) {
      const int c = slots ? slots[sl] : sl;
      const float p = __expf(taps.at(base + (long)c * h * w) - l);
      const bool fg = valid && lab == c;
      const float e = fg ? fabsf(1.f - p) : p;
      if (in) {
        const long o = (long)(per_image ? b * nslots + sl : sl) * L + local;
        key[o] = valid ? 0xFFFFFFFEu - __float_as_uint(e) : 0xFFFFFFFFu;
        pay[o] = (uint32_t)gp | (fg ? 0x80000000u : 0u);
      }
      const unsigned long long fb = __ballot(fg);
      if (lane == 0 && fb) atomicAdd(&lov_cnt[sl], __popcll(fb));
    }
  }
  __syncthreads();
  for (int sl = tid; sl < nslots; sl += 256) {
    const int seg = per_image ? b * nslots + sl : sl;
    if (lov_cnt[sl]) atomicAdd(&segG[seg], lov_cnt[sl]);
    if (lov_cnt[nslots]) atomicAdd(&segNV[seg], lov_cnt[nslots]);
  }
}

// one workgroup.  meta = [nseg] summed flag | [C] class -> slot (-1: the class has no slot)
__global__ __launch_bounds__(256) void upsample_lovasz_plan_kernel(const int* __restrict__ segG, const int* __restrict__ segNV,
                                                                   const int* __restrict__ slots, const float* __restrict__ cw,
                                                                   int* __restrict__ meta, float* __restrict__ segcoef, int C,
                                                                   int nslots, int nseg, int B, int present, int per_image,
                                                                   int image_mean, float loss_weight) {
  for (int seg = threadIdx.x; seg < nseg; seg += 256) {
    const int sl = seg % nslots, g0 = seg - sl;
    const bool act = segNV[seg] > 0 && (!present || segG[seg] > 0);
    int cnt = 0;
    for (int s2 = 0; s2 < nslots; ++s2) cnt += (segNV[g0 + s2] > 0 && (!present || segG[g0 + s2] > 0)) ? 1 : 0;
    const int c = slots ? slots[sl] : sl;
    double kk = 0.0;
    if (act) kk = (double)loss_weight * (double)(cw ? cw[c] : 1.f) / (double)cnt / (per_image && image_mean ? (double)B : 1.0);
    meta[seg] = act ? 1 : 0;
    segcoef[seg] = (float)kk;
  }
  for (int c = threadIdx.x; c < C; c += 256) meta[nseg + c] = -1;
  __syncthreads();
  for (int sl = threadIdx.x; sl < nslots; sl += 256) meta[nseg + (slots ? slots[sl] : sl)] = sl;
}

// ---- the segmented stable LSD radix sort: one pass of 8 bits -------------------------------------------------------------------
// hist[(seg * 256 + digit) * ntile + tile]: the count, then (after the scan) the first output position of that digit of that tile
__global__ __launch_bounds__(256) void lovasz_sort_hist_kernel(const uint32_t* __restrict__ key, const int* __restrict__ act,
                                                               uint32_t* __restrict__ hist, long L, int ntile, int nwg, int shift) {
  const int seg = blockIdx.x / nwg, wg = blockIdx.x % nwg;
  if (!act[seg]) return;
  __shared__ unsigned sh[LOV_WG_TILES][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long tile = (long)wg * LOV_WG_TILES + wv;
  for (int d = lane; d < 256; d += 64) sh[wv][d] = 0;
  __syncthreads();
  const uint32_t* kseg = key + (long)seg * L;
  for (int r = 0; r < LOV_TILE / 64; ++r) {
    const long idx = tile * LOV_TILE + r * 64 + lane;
    if (idx < L) atomicAdd(&sh[wv][(kseg[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (tile < ntile)
    for (int d = lane; d < 256; d += 64) hist[((long)seg * 256 + d) * ntile + tile] = sh[wv][d];
}

// one workgroup per segment, thread d owns digit d: exclusive scan in (digit, tile) order
__global__ __launch_bounds__(256) void lovasz_sort_scan_kernel(const int* __restrict__ act, uint32_t* __restrict__ hist, int ntile) {
  const int seg = blockIdx.x, d = threadIdx.x;
  if (!act[seg]) return;
  __shared__ unsigned tot[256];
  uint32_t* row = hist + ((long)seg * 256 + d) * ntile;
  unsigned sum = 0;
  for (int t = 0; t < ntile; ++t) sum += row[t];
  tot[d] = sum;
  __syncthreads();
  unsigned run = 0;
  for (int q = 0; q < d; ++q) run += tot[q];
  for (int t = 0; t < ntile; ++t) {
    const unsigned v = row[t];
    row[t] = run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void lovasz_sort_scatter_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ pay,
                                                                  uint32_t* __restrict__ okey, uint32_t* __restrict__ opay,
                                                                  const int* __restrict__ act, const uint32_t* __restrict__ hist,
                                                                  long L, int ntile, int nwg, int shift) {
  const int seg = blockIdx.x / nwg, wg = blockIdx.x % nwg;
  if (!act[seg]) return;
  __shared__ unsigned sb[LOV_WG_TILES][256];  // next output position of a digit of this wavefront's tile
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long tile = (long)wg * LOV_WG_TILES + wv;
  if (tile < ntile)
    for (int d = lane; d < 256; d += 64) sb[wv][d] = hist[((long)seg * 256 + d) * ntile + tile];
  __syncthreads();
  const long so = (long)seg * L;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = 0; r < LOV_TILE / 64; ++r) {  // 64 elements in order; (uniform trip count: barriers and ballots inside)
    const long idx = tile * LOV_TILE + r * 64 + lane;
    const bool in = idx < L;
    const uint32_t kv = in ? key[so + idx] : 0u, pv = in ? pay[so + idx] : 0u;
    const unsigned d = (kv >> shift) & 255u;
    unsigned long long peers = __ballot(in);  // the lanes of this round holding the same digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bb = __ballot(in && on);
      peers &= on ? bb : ~bb;
    }
    const int rank = __popcll(peers & below), total = __popcll(peers);
    unsigned pos = 0;
    if (in) {
      pos = sb[wv][d] + (unsigned)rank;  // (pos < L: the scanned counts of this segment)
      okey[so + pos] = kv;
      opay[so + pos] = pv;
    }
    __syncthreads();
    if (in && rank == total - 1) sb[wv][d] = pos + 1u;  // the last lane of a digit moves its cursor
    __syncthreads();
  }
}

// ---- the scan over the sorted order -----------------------------------------------------------------------------------------------
__device__ __forceinline__ int lov_block_sum_int(int v, int* red) {  // 256 threads; red: 4 ints
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void lovasz_fg_count_kernel(const uint32_t* __restrict__ pay, const int* __restrict__ act,
                                                              const int* __restrict__ segNV, uint32_t* __restrict__ fgcnt, long L,
                                                              int nscan) {
  const int seg = blockIdx.x / nscan, t = blockIdx.x % nscan;
  if (!act[seg]) return;
  __shared__ int red[4];
  const long nv = segNV[seg];
  int cnt = 0;
  for (int r = 0; r < LOV_SCAN / 256; ++r) {
    const long idx = (long)t * LOV_SCAN + r * 256 + threadIdx.x;
    if (idx < nv) cnt += (int)(pay[(long)seg * L + idx] >> 31);
  }
  cnt = lov_block_sum_int(cnt, red);
  if (threadIdx.x == 0) fgcnt[(long)seg * nscan + t] = (uint32_t)cnt;
}

__global__ __launch_bounds__(256) void lovasz_apply_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ pay,
                                                           const int* __restrict__ act, const int* __restrict__ segG,
                                                           const int* __restrict__ segNV, const float* __restrict__ segcoef,
                                                           const uint32_t* __restrict__ fgcnt, double* __restrict__ lpart,
                                                           float* __restrict__ dplane, long L, long N, int nscan, int nslots) {
  constexpr int R = LOV_SCAN / 256;
  const int seg = blockIdx.x / nscan, t = blockIdx.x % nscan;
  if (!act[seg]) return;
  const long nv = segNV[seg];
  if ((long)t * LOV_SCAN >= nv) return;  // (uniform)
  __shared__ int red[4];
  __shared__ int sW[R][4];
  __shared__ double dred[256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long G = segG[seg];
  const double coef = (double)segcoef[seg];
  int before = 0;  // foreground elements of the tiles before this one
  for (int q = tid; q < t; q += 256) before += (int)fgcnt[(long)seg * nscan + q];
  before = lov_block_sum_int(before, red);
  uint32_t kv[R], pv[R];
  int incl[R];
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long idx = (long)t * LOV_SCAN + r * 256 + tid;
    const bool in = idx < nv;
    kv[r] = in ? key[(long)seg * L + idx] : 0u;
    pv[r] = in ? pay[(long)seg * L + idx] : 0u;
    const unsigned long long bal = __ballot(in && (pv[r] >> 31));
    incl[r] = __popcll(bal & upto);
    if (lane == 0) sW[r][wv] = __popcll(bal);
  }
  __syncthreads();
  double acc = 0.0;
  long run = before;
  float* drow = dplane + (long)(seg % nslots) * N;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    long off = run;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < wv) off += sW[r][q];
      run += sW[r][q];
    }
    const long idx = (long)t * LOV_SCAN + r * 256 + tid;
    if (idx < nv) {
      const bool fg = pv[r] >> 31;
      const long F = off + incl[r];          // foreground among the first idx + 1 sorted elements
      const long I = G - F, U = G + (idx + 1 - F);
      double g;
      if (G == 0) g = idx == 0 ? 1.0 : 0.0;
      else if (fg) g = 1.0 / (double)U;
      else g = (double)I / ((double)U * (double)(U - 1));
      const float e = __uint_as_float(0xFFFFFFFEu - kv[r]);
      acc += (double)e * g;
      drow[pv[r] & 0x7FFFFFFFu] = (float)(fg ? -g * coef : g * coef);
    }
  }
  dred[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // a fixed tree
    if (tid < o) dred[tid] += dred[tid + o];
    __syncthreads();
  }
  if (tid == 0) lpart[(long)seg * nscan + t] = dred[0];
}

__global__ __launch_bounds__(256) void upsample_lovasz_final_kernel(const int* __restrict__ act, const int* __restrict__ segNV,
                                                                    const float* __restrict__ segcoef,
                                                                    const double* __restrict__ lpart, float* __restrict__ loss,
                                                                    int nseg, int nscan) {
  __shared__ double dred[256];
  double acc = 0.0;
  for (int seg = threadIdx.x; seg < nseg; seg += 256) {
    if (!act[seg]) continue;
    const long used = ((long)segNV[seg] + LOV_SCAN - 1) / LOV_SCAN;
    double s = 0.0;
    for (long t = 0; t < used; ++t) s += lpart[(long)seg * nscan + t];
    acc += (double)segcoef[seg] * s;
  }
  dred[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += dred[i];
    loss[0] = (float)t;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// S(pix) = sum over the summed class slots of p_c D_c(pix); 0 at an ignored pixel (the gather skips it)
__global__ __launch_bounds__(256) void upsample_lovasz_s_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                const int* __restrict__ slots, const float* __restrict__ lse,
                                                                const float* __restrict__ dplane, const int* __restrict__ act,
                                                                float* __restrict__ pix_s, int B, int C, int nslots, int h, int w,
                                                                int H, int W, int ignore, int per_image) {
  const long npix = (long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    if (label[p] == ignore) {
      pix_s[p] = 0.f;
      continue;
    }
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long)W * H));
    const Taps taps(y, x, sy, sx, h, w);
    const float* base = logit + (long)b * C * h * w;
    const float l = lse[p];
    float s = 0.f;
    for (int sl = 0; sl < nslots; ++sl) {
      if (!act[per_image ? b * nslots + sl : sl]) continue;
      const int c = slots ? slots[sl] : sl;
      s = fmaf(__expf(taps.at(base + (long)c * h * w) - l), dplane[(long)sl * npix + p], s);
    }
    pix_s[p] = s;
  }
}

// the gather's term p_c (D_c(pix) - S(pix)); D_c = 0 for a class without a summed slot (its plane is never read)
struct LovaszTerm {
  static constexpr bool PLANE = true;
  static constexpr bool RAW = false;
  static constexpr bool PIXEL = true;
  const int64_t* __restrict__ label;
  const float* __restrict__ dplane;
  const float* __restrict__ pix_s;
  const int* __restrict__ meta;  // [nseg] summed | [C] class -> slot
  int C, nslots, nseg, ignore, per_image;
  long npix;
  const float* drow;  // this lane's class: its D plane, or null
  __device__ __forceinline__ void load_class(int b, int c) {
    drow = nullptr;
    if (c < C) {
      const int sl = meta[nseg + c];
      if (sl >= 0 && meta[per_image ? b * nslots + sl : sl]) drow = dplane + (long)sl * npix;
    }
  }
  __device__ __forceinline__ int stage(long p, float& plane) const {
    plane = pix_s[p];
    return label[p] != ignore ? 0 : -1;
  }
  __device__ __forceinline__ bool skip(int lab) const { return lab < 0; }
  __device__ __forceinline__ float term(float prob, int c, int lab, float plane, long p) const {
    return prob * ((drow ? drow[p] : 0.f) - plane);
  }
};

__global__ __launch_bounds__(512) void upsample_lovasz_bwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                  const float* __restrict__ lse, const float* __restrict__ dplane,
                                                                  const float* __restrict__ pix_s, const int* __restrict__ meta,
                                                                  const float* __restrict__ gscale, float* __restrict__ dlogit,
                                                                  int B, int C, int nslots, int nseg, int h, int w, int H, int W,
                                                                  int ignore, int per_image) {
  upsample_gather(LovaszTerm{label, dplane, pix_s, meta, C, nslots, nseg, ignore, per_image, (long)B * H * W, nullptr}, logit, lse,
                  gscale, dlogit, C, h, w, H, W);
}

static int lovasz_check(const char* entry, int B, int C, int nslots, int h, int w, int H, int W) {
  if (int e = upsample_check_shape(entry, B, C, h, w, H, W)) return e;
  if (nslots <= 0 || nslots > C) return fail(RSCOTR_E_ARG, "%s: 1 <= nslots <= C required", entry);
  if ((long)B * H * W > 0x7fffffffL)  // the payload keeps the flat pixel index in 31 bits
    return fail(RSCOTR_E_SHAPE, "%s: more than 2^31 - 1 pixels", entry);
  if ((long)B * C > 0x3fffffffL || (long)C * h * w > 0x7fffffffL) return fail(RSCOTR_E_SHAPE, "%s: shape too large", entry);
  return RSCOTR_OK;
}

static int64_t lovasz_workspace(int B, int C, int nslots, int H, int W, int per_image) {
  if (B <= 0 || C <= 0 || nslots <= 0 || H <= 0 || W <= 0) return 0;
  const long N = (long)B * H * W;
  return lovasz_carve(nullptr, nslots, N, per_image ? B * nslots : nslots, per_image ? (long)H * W : N).bytes;
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int64_t rscotr_upsample_lovasz_workspace(int B, int C, int nslots, int H, int W, int per_image) {
  return lovasz_workspace(B, C, nslots, H, W, per_image);
}

extern "C" int rscotr_upsample_lovasz_sort_tile(void) { return LOV_TILE; }
extern "C" int rscotr_upsample_lovasz_sort_workgroup(void) { return LOV_WG; }

extern "C" int rscotr_upsample_lovasz_fwd(const float* logit, const int64_t* label, const int* slots, const float* class_weight,
                                          float* lse, float* dplane, int* meta, float* loss, int B, int C, int nslots, int h,
                                          int w, int H, int W, int ignore_index, int present, int per_image, int image_mean,
                                          float loss_weight, float* workspace, int64_t workspace_bytes, void* stream) {
  const char* entry = "rscotr_upsample_lovasz_fwd";
  if (int e = lovasz_check(entry, B, C, nslots, h, w, H, W)) return e;
  if (!loss) return fail(RSCOTR_E_ARG, "%s: null pointer", entry);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    (void)hipMemsetAsync(loss, 0, sizeof(float), s);
    return RSCOTR_OK;
  }
  if (!logit || !label || !lse || !dplane || !meta) return fail(RSCOTR_E_ARG, "%s: null pointer", entry);
  if (!workspace || workspace_bytes < lovasz_workspace(B, C, nslots, H, W, per_image))
    return fail(RSCOTR_E_ARG, "%s: workspace of rscotr_upsample_lovasz_workspace(B, C, nslots, H, W, per_image) bytes required",
                entry);
  const long N = (long)B * H * W, L = per_image ? (long)H * W : N;
  const long nseg_l = per_image ? (long)B * nslots : nslots;
  const long ntile = (L + LOV_TILE - 1) / LOV_TILE, nwg = (L + LOV_WG - 1) / LOV_WG, nscan = (L + LOV_SCAN - 1) / LOV_SCAN;
  const int nchunk = (int)std::min<long>(((long)H * W + 255) / 256, LOV_CHUNKS);
  if (nseg_l * nscan > 0x7fffffffL || nseg_l * 256 * ntile > 0x7fffffffL || (long)B * nchunk > 0x7fffffffL)
    return fail(RSCOTR_E_SHAPE, "%s: too many segments", entry);
  if ((size_t)(nslots + 1) * 4 > 48 * 1024) return fail(RSCOTR_E_SHAPE, "%s: too many class slots", entry);
  const int nseg = (int)nseg_l;
  const LovWs ws = lovasz_carve(workspace, nslots, N, nseg, L);
  (void)hipMemsetAsync(ws.segG, 0, (size_t)nseg * 2 * sizeof(int), s);
  upsample_lovasz_key_kernel<<<B * nchunk, 256, (size_t)(nslots + 1) * 4, s>>>(logit, label, slots, lse, ws.keyA, ws.payA, ws.segG,
                                                                              ws.segNV, C, nslots, h, w, H, W, ignore_index,
                                                                              per_image, nchunk, N);
  upsample_lovasz_plan_kernel<<<1, 256, 0, s>>>(ws.segG, ws.segNV, slots, class_weight, meta, ws.segcoef, C, nslots, nseg, B,
                                                present, per_image, image_mean, loss_weight);
  uint32_t *kin = ws.keyA, *pin = ws.payA, *kout = ws.keyB, *pout = ws.payB;
  for (int shift = 0; shift < 32; shift += 8) {
    lovasz_sort_hist_kernel<<<(int)(nseg * nwg), 256, 0, s>>>(kin, meta, ws.hist, L, (int)ntile, (int)nwg, shift);
    lovasz_sort_scan_kernel<<<nseg, 256, 0, s>>>(meta, ws.hist, (int)ntile);
    lovasz_sort_scatter_kernel<<<(int)(nseg * nwg), 256, 0, s>>>(kin, pin, kout, pout, meta, ws.hist, L, (int)ntile, (int)nwg,
                                                                 shift);
    std::swap(kin, kout);
    std::swap(pin, pout);
  }
  lovasz_fg_count_kernel<<<(int)(nseg * nscan), 256, 0, s>>>(pin, meta, ws.segNV, ws.fgcnt, L, (int)nscan);
  lovasz_apply_kernel<<<(int)(nseg * nscan), 256, 0, s>>>(kin, pin, meta, ws.segG, ws.segNV, ws.segcoef, ws.fgcnt, ws.lpart, dplane,
                                                          L, N, (int)nscan, nslots);
  upsample_lovasz_final_kernel<<<1, 256, 0, s>>>(meta, ws.segNV, ws.segcoef, ws.lpart, loss, nseg, (int)nscan);
  return check_launch(entry);
}

// dlogit (B,C,h,w) = grad_scale[0] * d(loss)/d(logit); grad_scale is a DEVICE scalar (the upstream gradient); pix_s (B,H,W) is
// the caller's scratch plane for S; slots, lse, dplane and meta as the forward entry took / left them
extern "C" int rscotr_upsample_lovasz_bwd(const float* logit, const int64_t* label, const int* slots, const float* lse,
                                          const float* dplane, const int* meta, const float* grad_scale, float* pix_s,
                                          float* dlogit, int B, int C, int nslots, int h, int w, int H, int W, int ignore_index,
                                          int per_image, void* stream) {
  const char* entry = "rscotr_upsample_lovasz_bwd";
  if (int e = lovasz_check(entry, B, C, nslots, h, w, H, W)) return e;
  if (B == 0) return RSCOTR_OK;
  if (!logit || !label || !lse || !dplane || !meta || !grad_scale || !pix_s || !dlogit)
    return fail(RSCOTR_E_ARG, "%s: null pointer", entry);
  hipStream_t s = (hipStream_t)stream;
  const long npix = (long)B * H * W;
  const int nwg = (int)std::min<long>((npix + 255) / 256, 4096);
  const int nseg = per_image ? B * nslots : nslots;
  upsample_lovasz_s_kernel<<<nwg, 256, 0, s>>>(logit, label, slots, lse, dplane, meta, pix_s, B, C, nslots, h, w, H, W,
                                               ignore_index, per_image);
  launch_upsample_gather<upsample_lovasz_bwd_kernel, true>(s, B, h, w, logit, label, lse, dplane, pix_s, meta, grad_scale, dlogit,
                                                           B, C, nslots, nseg, h, w, H, W, ignore_index, per_image);
  return check_launch(entry);
}
