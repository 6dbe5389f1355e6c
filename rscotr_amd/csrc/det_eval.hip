// Detection evaluation on the device (include/rscotr.h: rscotr_det_decode_f32, rscotr_det_match).
//
// det_decode: the inference tail of DINOHead._get_bboxes_single for a batch, ONE workgroup of 1024 threads per image:
// sigmoid of the Q * C last-layer logits as order-preserving keys in LDS, the exact top-K of det_select.h (radix select,
// ties to the lower flat index, bitonic sort into torch.topk(sorted=True) order), then per winner label = idx % C, the box of
// query idx / C through the fp32 operation sequence of the torch chain (cxcywh -> xyxy, * img_w / img_h, clamp, optional IEEE
// divide by the scale factor), every product, sum and quotient rounded on its own: the box columns are bit-equal to the chain
// evaluated in fp32 on the CPU.  Instead of ~10 launches and two device-to-host copies per image.
//
// det_match: COCOeval.evaluateImg (rscotr_amd/metrics.py `_evaluate_img`) for every (image, class, area range, IoU
// threshold) of a batch in one launch.  One workgroup of 8 wavefronts per (image, class): the ground truths of the class
// (fp32 boxes, <= 1024) and the indices of its first max_det detections are compacted into LDS in their original order; then
// one wavefront per (area range, threshold) pair walks the detections in score order.  The ground truths are spread over
// the 64 lanes; each lane computes the fp64 IoU of its unmatched ground truths from the fp32 boxes (the operation order of
// `_iou_xyxy`, contraction off: the same bits as the host; recomputed per pair instead of a D x G fp64 tile, which would cap
// the ground truths of a class at ~160), keeps its best candidate, and a cross-lane butterfly picks the winner of the
// host's sequential walk: a regular ground truth before an ignored one, then the larger IoU, then the LATER ground truth (the
// host replaces on equality).  The matched set is one bit per ground truth in a per-lane mask.  Flag words are OR-ed
// together in LDS (integer, order-independent) and written once: no float atomics, bit-reproducible.
#include "det_select.h"

namespace rscotr {
namespace {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------------------- decode
__global__ __launch_bounds__(SEL_THREADS) void det_decode_kernel(const float* __restrict__ cls, const float* __restrict__ box,
                                                                 const float* __restrict__ meta, float* __restrict__ dets,
                                                                 long long* __restrict__ labels, int N, int C, int K,
                                                                 int rescale) {
  extern __shared__ __attribute__((aligned(16))) unsigned sel_lds[];
  unsigned* keys = sel_lds;                                                                    // [N]
  unsigned long long* cand = reinterpret_cast<unsigned long long*>(sel_lds + ((N + 3) & ~3));  // [1024] (key << 32 | ~idx)
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* cb = cls + (long)b * N;
  for (int n = tid; n < N; n += SEL_THREADS) {
    const float x = cb[n];
    const float s = 1.f / (1.f + expf(-x));
    keys[n] = order_key(s != s ? __uint_as_float(0x7fc00000u) : s);  // (a NaN of either sign ranks above 1.0, as torch.topk)
  }
  select_sort_topk(keys, cand, N, K);

  const float* m = meta + (long)b * 6;
  const float img_h = m[0], img_w = m[1];
  for (int k = tid; k < K; k += SEL_THREADS) {
    const unsigned long long e = cand[k];
    const int n = (int)(0xffffffffu - (unsigned)(e & 0xffffffffull));
    const int q = n / C;
    const float4 p = *reinterpret_cast<const float4*>(box + ((long)b * (N / C) + q) * 4);  // cx, cy, w, h
    // ops.bbox_cxcywh_to_xyxy: cx - 0.5 * w, ...; then * img_w / img_h; then clamp(min=0, max=img_w / img_h), NaN kept
    const float hw = 0.5f * p.z, hh = 0.5f * p.w;
    float v[4] = {(p.x - hw) * img_w, (p.y - hh) * img_h, (p.x + hw) * img_w, (p.y + hh) * img_h};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float hi = (i & 1) ? img_h : img_w;
      v[i] = v[i] < 0.f ? 0.f : (v[i] > hi ? hi : v[i]);
      if (rescale) v[i] = __fdiv_rn(v[i], m[2 + i]);
    }
    float* o = dets + ((long)b * K + k) * 5;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    o[4] = order_key_value((unsigned)(e >> 32));
    labels[(long)b * K + k] = n - q * C;
  }
}

// ----------------------------------------------------------------------------------------------------------- match
constexpr int kMatchThreads = 512, kMatchWaves = kMatchThreads / 64;
constexpr int kMatchMaxGt = 1024;     // ground truths of one (image, class): 16 per lane, one bit each in a 32-bit mask
constexpr int kMatchMaxK = 1024;      // detections per image
// thresholds: bits 0 .. 15 matched, 16 .. 31 ignored, bit 31 ALONE = dropped.  At T == 16 no evaluated detection has that word:
// ignored at threshold 15 means matched there (bit 15) or unmatched with its area outside the range, hence bit 0 or bit 16.
constexpr int kMatchMaxT = 16;
constexpr int kMatchMaxFlagWords = 8192;  // min(max_det, K) * A flag words in dynamic LDS (32 KB)

// rank of this thread among the threads of the workgroup whose `pred` holds, in thread order; total over the workgroup.
// Every thread calls it; two barriers.
__device__ __forceinline__ int block_rank(bool pred, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(pred);
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kMatchWaves; ++w) {
    const int c = wsum[w];
    if (w < wave) before += c;
    total += c;
  }
  __syncthreads();
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

struct Cand {
  int pri;     // 0 none, 1 an ignored ground truth, 2 a regular one
  double iou;
  int g;       // position among the ground truths of the class (original order)
};

// the winner of the host's walk over the ground truths (non-ignored first, stable): the regular one, then the larger IoU,
// then the later one.  Written with the host's `<` so that both orders of a NaN compare the same way (the later wins).
__device__ __forceinline__ Cand better(Cand a, Cand c) {
  const bool take_c = a.pri != c.pri ? c.pri > a.pri : (c.iou < a.iou ? false : (a.iou < c.iou ? true : c.g > a.g));
  Cand r;
  r.pri = take_c ? c.pri : a.pri;
  r.iou = take_c ? c.iou : a.iou;
  r.g = take_c ? c.g : a.g;
  return r;
}

__global__ __launch_bounds__(kMatchThreads) void det_match_kernel(
    const float* __restrict__ dets, const long long* __restrict__ labels, const int* __restrict__ n_det,
    const float* __restrict__ gt, const long long* __restrict__ gt_labels, const long long* __restrict__ gt_off,
    const double* __restrict__ ranges, const double* __restrict__ thrs, int* __restrict__ flags, int* __restrict__ npig,
    int K, long G_total, int C, int A, int T, int max_det) {
  extern __shared__ int s_flags[];  // [D * A], D <= min(max_det, K)
  __shared__ float4 s_gt[kMatchMaxGt];
  __shared__ int s_didx[kMatchMaxK];
  __shared__ int s_wsum[kMatchWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / C, c = blockIdx.x - b * C;
  const int nd = min(max(n_det[b], 0), K);
  const float* db = dets + (long)b * K * 5;
  const long long* lb = labels + (long)b * K;
  int* fb = flags + (long)b * K * A;

  // ground truths of class c in their original order (offsets clamped into [0, G_total], counts into the LDS table)
  long g0 = gt_off[b], g1 = gt_off[b + 1];
  g0 = g0 < 0 ? 0 : (g0 > G_total ? G_total : g0);
  g1 = g1 < g0 ? g0 : (g1 > G_total ? G_total : g1);
  int G = 0;
  for (long i0 = g0; i0 < g1; i0 += kMatchThreads) {
    const long i = i0 + tid;
    const bool mine = i < g1 && gt_labels[i] == (long long)c;
    int total;
    const int r = G + block_rank(mine, s_wsum, total);
    if (mine && r < kMatchMaxGt) s_gt[r] = *reinterpret_cast<const float4*>(gt + i * 4);
    G += total;
  }
  G = min(G, kMatchMaxGt);

  // detections of class c in score order: the first max_det are evaluated, the others dropped
  const int d_cap = min(max_det, K);
  int D = 0;
  for (int k0 = 0; k0 < K; k0 += kMatchThreads) {
    const int k = k0 + tid;
    const long long l = k < nd ? lb[k] : -1;
    const bool mine = k < nd && l == (long long)c;
    int total;
    const int r = D + block_rank(mine, s_wsum, total);
    if (mine && r < d_cap) s_didx[r] = k;
    // rows nobody evaluates: beyond max_det of their class, beyond n_det, or with a label outside [0, C) (class 0 writes those)
    if (k < K && ((mine && r >= d_cap) || (c == 0 && (k >= nd || l < 0 || l >= (long long)C))))
      for (int a = 0; a < A; ++a) fb[(long)k * A + a] = (int)0x80000000u;
    D += total;
  }
  D = min(D, d_cap);
  for (int i = tid; i < D * A; i += kMatchThreads) s_flags[i] = 0;
  __syncthreads();

  for (int p = wave; p < A * T; p += kMatchWaves) {
    const int a = p / T, t = p - a * T;
    const double lo = ranges[2 * a], hi = ranges[2 * a + 1];
    const double t0 = thrs[t], thr = t0 < 1 - 1e-10 ? t0 : 1 - 1e-10;  // min(t, 1 - 1e-10)
    if (t == 0) {  // non-ignored ground truths of this area range
      int cnt = 0;
      for (int j0 = 0; j0 < G; j0 += 64) {
        bool reg = false;
        if (j0 + lane < G) {
          const float4 q = s_gt[j0 + lane];
          const double ag = ((double)q.z - (double)q.x) * ((double)q.w - (double)q.y);
          reg = !((ag < lo) | (ag > hi));
        }
        cnt += __popcll(__ballot(reg));
      }
      if (lane == 0) npig[((long)b * C + c) * A + a] = cnt;
    }
    unsigned taken = 0u;  // bit j: ground truth lane + 64 j is matched at this (area range, threshold)
    for (int r = 0; r < D; ++r) {
      const float* dp = db + (long)s_didx[r] * 5;
      const double dx1 = dp[0], dy1 = dp[1], dx2 = dp[2], dy2 = dp[3];
      const double ad = (dx2 - dx1) * (dy2 - dy1);
      Cand best = {0, thr, -1};
      for (int j = 0; j * 64 < G; ++j) {
        const int g = j * 64 + lane;
        if (g >= G || ((taken >> j) & 1u)) continue;
        const float4 q = s_gt[g];
        const double gx1 = q.x, gy1 = q.y, gx2 = q.z, gy2 = q.w;
        const double x1 = dx1 > gx1 ? dx1 : gx1, y1 = dy1 > gy1 ? dy1 : gy1;
        const double x2 = dx2 < gx2 ? dx2 : gx2, y2 = dy2 < gy2 ? dy2 : gy2;
        double iw = x2 - x1, ih = y2 - y1;
        iw = iw < 0.0 ? 0.0 : iw;
        ih = ih < 0.0 ? 0.0 : ih;
        const double inter = iw * ih;
        const double ag = (gx2 - gx1) * (gy2 - gy1);
        const double iou = inter / ((ad + ag) - inter);
        if (iou < thr) continue;  // (the host's `if ious < iou: continue` against the threshold)
        const Cand cd = {((ag < lo) | (ag > hi)) ? 1 : 2, iou, g};
        best = best.pri == 0 ? cd : better(best, cd);
      }
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        Cand o;
        o.pri = __shfl_xor(best.pri, s);
        o.iou = __shfl_xor(best.iou, s);
        o.g = __shfl_xor(best.g, s);
        if (o.pri != 0) best = best.pri == 0 ? o : better(best, o);
      }
      int bits;
      if (best.pri != 0) {
        if ((best.g & 63) == lane) taken |= 1u << (best.g >> 6);
        bits = (1 << t) | (best.pri == 1 ? 1 << (16 + t) : 0);
      } else {
        bits = ((ad < lo) | (ad > hi)) ? 1 << (16 + t) : 0;  // unmatched and outside the area range: ignored
      }
      if (lane == 0 && bits) atomicOr(&s_flags[r * A + a], bits);
    }
  }
  __syncthreads();
  for (int i = tid; i < D * A; i += kMatchThreads) {
    const int r = i / A, a = i - r * A;
    fb[(long)s_didx[r] * A + a] = s_flags[i];
  }
}

}  // namespace
}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_det_decode_f32(const float* cls, const float* box, const float* meta, float* dets, int64_t* labels, int B,
                                     int Q, int C, int K, int rescale, void* stream) {
  const char* fn = "rscotr_det_decode_f32";
  if (B < 0 || Q <= 0 || C <= 0 || K <= 0) return fail(RSCOTR_E_SHAPE, "%s: bad shape B=%d Q=%d C=%d K=%d", fn, B, Q, C, K);
  const int64_t N = (int64_t)Q * C;
  if (N > SEL_MAX_N || K > N || K > SEL_MAX_K)
    return fail(RSCOTR_E_SHAPE, "%s: needs Q * C <= %d and K <= min(Q * C, %d) (Q=%d C=%d K=%d)", fn, SEL_MAX_N, SEL_MAX_K, Q, C, K);
  if (B == 0) return RSCOTR_OK;
  if (!cls || !box || !meta || !dets || !labels) return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  if (!aligned16(box)) return fail(RSCOTR_E_ALIGN, "%s: box must be 16-byte aligned", fn);
  static const bool attr_set = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(det_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)select_lds_bytes(SEL_MAX_N));
    return true;
  }();
  (void)attr_set;
  det_decode_kernel<<<dim3((unsigned)B), SEL_THREADS, select_lds_bytes((int)N), (hipStream_t)stream>>>(
      cls, box, meta, dets, reinterpret_cast<long long*>(labels), (int)N, C, K, rescale ? 1 : 0);
  return check_launch(fn);
}

extern "C" int rscotr_det_match(const float* dets, const int64_t* labels, const int32_t* n_det, const float* gt_boxes,
                                const int64_t* gt_labels, const int64_t* gt_offsets, const double* area_ranges,
                                const double* iou_thrs, int32_t* flags, int32_t* npig, int B, int K, int64_t G, int C, int A,
                                int T, int max_det, void* stream) {
  const char* fn = "rscotr_det_match";
  if (B < 0 || K <= 0 || G < 0 || C <= 0 || A <= 0 || T <= 0 || max_det <= 0)
    return fail(RSCOTR_E_SHAPE, "%s: bad shape B=%d K=%d G=%lld C=%d A=%d T=%d max_det=%d", fn, B, K, (long long)G, C, A, T, max_det);
  if (K > kMatchMaxK || T > kMatchMaxT) return fail(RSCOTR_E_SHAPE, "%s: needs K <= %d and T <= %d (K=%d T=%d)", fn, kMatchMaxK, kMatchMaxT, K, T);
  const int64_t words = (int64_t)(max_det < K ? max_det : K) * A;
  if (words > kMatchMaxFlagWords)
    return fail(RSCOTR_E_SHAPE, "%s: min(max_det, K) * A = %lld exceeds %d", fn, (long long)words, kMatchMaxFlagWords);
  if ((int64_t)B * C > INT32_MAX) return fail(RSCOTR_E_SHAPE, "%s: B * C must fit 31 bits", fn);
  if (B == 0) return RSCOTR_OK;
  if (!dets || !labels || !n_det || !gt_offsets || !area_ranges || !iou_thrs || !flags || !npig || (G > 0 && (!gt_boxes || !gt_labels)))
    return fail(RSCOTR_E_ARG, "%s: null pointer", fn);
  if (gt_boxes && !aligned16(gt_boxes)) return fail(RSCOTR_E_ALIGN, "%s: gt_boxes must be 16-byte aligned", fn);
  det_match_kernel<<<dim3((unsigned)(B * C)), kMatchThreads, (size_t)words * 4, (hipStream_t)stream>>>(
      dets, reinterpret_cast<const long long*>(labels), n_det, gt_boxes, reinterpret_cast<const long long*>(gt_labels),
      reinterpret_cast<const long long*>(gt_offsets), area_ranges, iou_thrs, flags, npig, K, (long)G, C, A, T, max_det);
  return check_launch(fn);
}
