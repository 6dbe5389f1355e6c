// Dense masked attention pieces for the det / seg decoders: torch.nn.MultiheadAttention as wrapped by mmcv
// MultiheadAttention (configs/multi/MTL_slvlcls_...potsdam.py:81-85,144-151; reached from
// models/multi/bbox_head/transformer.py:103-108 and models/multi/seg_head/mask2former_head.py:183-192).
// The two products per head run on rscotr_gemm_f32_batched (per-head slices addressed in place); this file
// holds what sits between them: P = softmax(scale * S + mask) over the key axis, and its backward
// dS = scale * P * (dP - sum_k P_k dP_k), both in place.  A boolean mask (True = blocked, as in torch) is
// indexed by `mask_mode`: 0 none, 1 shared (Lq, Lk), 2 per image (B, Lq, Lk), 3 per image and head
// (B*heads, Lq, Lk).
//
// Mapping: one wavefront per row (rows are 64 ... 4096 keys: at most 16 KB, they stay in L1/L2 across the
// passes), four rows per workgroup; max / sum by wave butterflies.
#include "common.h"
#include <stdlib.h>

namespace rscotr {

__device__ __forceinline__ const unsigned char* mask_row(const unsigned char* mask, int mode, long row, int Lq,
                                                         int Lk, int heads) {
  if (mode == 0) return nullptr;
  const long i = row % Lq, bh = row / Lq;
  const long blk = mode == 1 ? 0 : (mode == 2 ? bh / heads : bh);
  return mask + (blk * Lq + i) * Lk;
}

__global__ __launch_bounds__(256) void softmax_mask_fwd_kernel(float* __restrict__ S, const unsigned char* __restrict__ mask,
                                                               int mode, long rows, int Lq, int Lk, int heads, float scale) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float* s = S + row * Lk;
  const unsigned char* m = mask_row(mask, mode, row, Lq, Lk, heads);
  float mx = -3.0e38f;
  for (int j = lane; j < Lk; j += 64) {
    const bool blocked = m && m[j];
    if (!blocked) mx = fmaxf(mx, s[j] * scale);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < Lk; j += 64) {
    const bool blocked = m && m[j];
    const float e = blocked ? 0.f : expf(s[j] * scale - mx);
    s[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;  // a fully blocked row (never produced on this path) -> zeros
  for (int j = lane; j < Lk; j += 64) s[j] *= inv;
}

// Rows of Lk = 4 * 64 * NV keys at most (Lk a multiple of 4) stay in registers as NV float4 per lane: one read and one write
// per element with 16-byte accesses instead of three scalar passes (the det decoder's 800-key rows: 22 -> ~10 us per call).
template <int NV>
__global__ __launch_bounds__(256) void softmax_mask_fwd_vec_kernel(float* __restrict__ S, const unsigned char* __restrict__ mask,
                                                                   int mode, long rows, int Lq, int Lk, int heads, float scale) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, Lk4 = Lk >> 2;
  float4* s4 = reinterpret_cast<float4*>(S + row * Lk);
  const unsigned char* m = mask_row(mask, mode, row, Lq, Lk, heads);
  float4 v[NV];
  unsigned long long blk = 0ull;  // bit 4 i + k: element k of vector i is blocked (or past the row)
  float mx = -3.0e38f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + i * 64;
    if (c < Lk4) {
      v[i] = s4[c];
      unsigned b4 = 0u;
      if (m) {
        const uchar4 mm = reinterpret_cast<const uchar4*>(m)[c];
        b4 = (mm.x ? 1u : 0u) | (mm.y ? 2u : 0u) | (mm.z ? 4u : 0u) | (mm.w ? 8u : 0u);
      }
      v[i].x *= scale; v[i].y *= scale; v[i].z *= scale; v[i].w *= scale;
      if (!(b4 & 1u)) mx = fmaxf(mx, v[i].x);
      if (!(b4 & 2u)) mx = fmaxf(mx, v[i].y);
      if (!(b4 & 4u)) mx = fmaxf(mx, v[i].z);
      if (!(b4 & 8u)) mx = fmaxf(mx, v[i].w);
      blk |= (unsigned long long)b4 << (4 * i);
    } else {
      blk |= 15ull << (4 * i);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const unsigned b4 = (unsigned)(blk >> (4 * i)) & 15u;
    v[i].x = (b4 & 1u) ? 0.f : expf(v[i].x - mx);
    v[i].y = (b4 & 2u) ? 0.f : expf(v[i].y - mx);
    v[i].z = (b4 & 4u) ? 0.f : expf(v[i].z - mx);
    v[i].w = (b4 & 8u) ? 0.f : expf(v[i].w - mx);
    sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  sum = wave_sum(sum);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + i * 64;
    if (c < Lk4) s4[c] = make_float4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void softmax_bwd_vec_kernel(const float* __restrict__ P, float* __restrict__ dP, long rows,
                                                              int Lk, float scale) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, Lk4 = Lk >> 2;
  const float4* p4 = reinterpret_cast<const float4*>(P + row * Lk);
  float4* d4 = reinterpret_cast<float4*>(dP + row * Lk);
  float4 p[NV], d[NV];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + i * 64;
    if (c < Lk4) {
      p[i] = p4[c];
      d[i] = d4[c];
      dot += (p[i].x * d[i].x + p[i].y * d[i].y) + (p[i].z * d[i].z + p[i].w * d[i].w);
    }
  }
  dot = wave_sum(dot);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + i * 64;
    if (c < Lk4)
      d4[c] = make_float4(scale * p[i].x * (d[i].x - dot), scale * p[i].y * (d[i].y - dot), scale * p[i].z * (d[i].z - dot),
                          scale * p[i].w * (d[i].w - dot));
  }
}

// dP <- scale * P * (dP - sum_k P_k dP_k)
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, long rows,
                                                          int Lk, float scale) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* p = P + row * Lk;
  float* d = dP + row * Lk;
  float dot = 0.f;
  for (int j = lane; j < Lk; j += 64) dot += p[j] * d[j];
  dot = wave_sum(dot);
  for (int j = lane; j < Lk; j += 64) d[j] = scale * p[j] * (d[j] - dot);
}

// DINO decoder query positions: gen_sineembed_for_position (models/multi/bbox_head/transformer.py:43-76):
// pos (rows, 4) = (x, y, w, h) in [0,1] -> out (rows, 512) = [emb(y) | emb(x) | emb(w) | emb(h)], each 128 wide with
// emb(v)[2i] = sin(2*pi*v / 10000^(2i/128)), emb(v)[2i+1] = cos(same).  One thread per output element.
__global__ __launch_bounds__(256) void sine_embed4_kernel(const float* __restrict__ pos, float* __restrict__ out, long rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * 512) return;
  const long row = i >> 9;
  const int c = (int)(i & 511), which = c >> 7, d = c & 127;
  const int src = which == 0 ? 1 : (which == 1 ? 0 : which);  // order (y, x, w, h)
  const float dim_t = powf(10000.0f, (float)(2 * (d / 2)) / 128.0f);
  const float v = pos[row * 4 + src] * 6.283185307179586f / dim_t;
  out[i] = (d & 1) ? cosf(v) : sinf(v);
}

}  // namespace rscotr

using namespace rscotr;

extern "C" int rscotr_sine_embed4(const float* pos, float* out, int64_t rows, void* stream) {
  if (rows < 0) return fail(RSCOTR_E_SHAPE, "rscotr_sine_embed4: negative rows");
  if (rows == 0) return RSCOTR_OK;
  if (!pos || !out) return fail(RSCOTR_E_ARG, "rscotr_sine_embed4: null pointer");
  sine_embed4_kernel<<<(unsigned)((rows * 512 + 255) / 256), 256, 0, (hipStream_t)stream>>>(pos, out, rows);
  return check_launch("rscotr_sine_embed4");
}

extern "C" int rscotr_softmax_mask_fwd(float* S, const unsigned char* mask, int mask_mode, int B, int heads, int Lq,
                                       int Lk, float scale, void* stream) {
  if (B < 0 || heads <= 0 || Lq < 0 || Lk <= 0) return fail(RSCOTR_E_SHAPE, "rscotr_softmax_mask_fwd: bad shape");
  if (mask_mode < 0 || mask_mode > 3 || (mask_mode > 0 && !mask)) return fail(RSCOTR_E_ARG, "rscotr_softmax_mask_fwd: bad mask");
  const long rows = (long)B * heads * Lq;
  if (rows == 0) return RSCOTR_OK;
  if (!S) return fail(RSCOTR_E_ARG, "rscotr_softmax_mask_fwd: null pointer");
  const unsigned grid = (unsigned)((rows + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (Lk & 3) == 0 && Lk <= 4096 && aligned16(S) && (!mask || (reinterpret_cast<uintptr_t>(mask) & 3u) == 0);
  if (vec && Lk <= 256) softmax_mask_fwd_vec_kernel<1><<<grid, 256, 0, st>>>(S, mask, mask_mode, rows, Lq, Lk, heads, scale);
  else if (vec && Lk <= 1024) softmax_mask_fwd_vec_kernel<4><<<grid, 256, 0, st>>>(S, mask, mask_mode, rows, Lq, Lk, heads, scale);
  else if (vec && Lk <= 2048) softmax_mask_fwd_vec_kernel<8><<<grid, 256, 0, st>>>(S, mask, mask_mode, rows, Lq, Lk, heads, scale);
  else if (vec) softmax_mask_fwd_vec_kernel<16><<<grid, 256, 0, st>>>(S, mask, mask_mode, rows, Lq, Lk, heads, scale);
  else softmax_mask_fwd_kernel<<<grid, 256, 0, st>>>(S, mask, mask_mode, rows, Lq, Lk, heads, scale);
  return check_launch("rscotr_softmax_mask_fwd");
}

extern "C" int rscotr_softmax_bwd(const float* P, float* dP, int64_t rows, int Lk, float scale, void* stream) {
  if (rows < 0 || Lk <= 0) return fail(RSCOTR_E_SHAPE, "rscotr_softmax_bwd: bad shape");
  if (rows == 0) return RSCOTR_OK;
  if (!P || !dP) return fail(RSCOTR_E_ARG, "rscotr_softmax_bwd: null pointer");
  const unsigned grid = (unsigned)((rows + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (Lk & 3) == 0 && Lk <= 4096 && aligned16(P) && aligned16(dP);
  if (vec && Lk <= 256) softmax_bwd_vec_kernel<1><<<grid, 256, 0, st>>>(P, dP, rows, Lk, scale);
  else if (vec && Lk <= 1024) softmax_bwd_vec_kernel<4><<<grid, 256, 0, st>>>(P, dP, rows, Lk, scale);
  else if (vec && Lk <= 2048) softmax_bwd_vec_kernel<8><<<grid, 256, 0, st>>>(P, dP, rows, Lk, scale);
  else if (vec) softmax_bwd_vec_kernel<16><<<grid, 256, 0, st>>>(P, dP, rows, Lk, scale);
  else softmax_bwd_kernel<<<grid, 256, 0, st>>>(P, dP, rows, Lk, scale);
  return check_launch("rscotr_softmax_bwd");
}
