// Fixed-order sums behind the products: split-K combines (immediate and deferred), the batched entry's slab sum, column sums.
#include "gemm_plan.h"
#include <algorithm>

namespace rscotr {
// Combine split-K slabs (fixed order: deterministic) and apply the epilogue; also the row-sum partials.
// VEC: N % 4 == 0 and 16-byte aligned slabs -> one float4 of one output row per thread per step.
template <bool VEC>
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(GemmParams p) {
  const long total = (long)p.M * p.N;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  float amx = 0.f;
  if (VEC) {
    const long total4 = total >> 2;
    const float4* sl = reinterpret_cast<const float4*>(p.slabs);
    for (long i = gid; i < total4; i += (long)gridDim.x * 256) {
      float4 v = sl[i];
#pragma unroll 8
      for (int s = 1; s < p.splits; ++s) {
        const float4 t = sl[(long)s * total4 + i];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
      const long e = i << 2;
      const int m = (int)(e / p.N), n = (int)(e - (long)m * p.N);
      if (p.vecC) {
        epilogue_store4(p, v, m, n, amx);
      } else {
        float* c = p.C + (long)m * p.ldc + n;
        c[0] = epilogue_one(p, v.x, m, n, amx);
        c[1] = epilogue_one(p, v.y, m, n + 1, amx);
        c[2] = epilogue_one(p, v.z, m, n + 2, amx);
        c[3] = epilogue_one(p, v.w, m, n + 3, amx);
      }
    }
  } else {
    for (long i = gid; i < total; i += (long)gridDim.x * 256) {
      float v = 0.f;
#pragma unroll 8
      for (int s = 0; s < p.splits; ++s) v += p.slabs[(long)s * total + i];
      const int m = (int)(i / p.N), n = (int)(i - (long)m * p.N);
      p.C[(long)m * p.ldc + n] = epilogue_one(p, v, m, n, amx);
    }
  }
  if (p.rowsum && gid < p.M) {
    float v = 0.f;
    for (int s = 0; s < p.splits; ++s) v += p.rs_slabs[(long)s * p.M + gid];
    p.rowsum[gid] = p.rowsum_acc ? p.rowsum[gid] + v : v;
  }
  amax_commit(p.amax_out, amx);
}

// Same combine for SMALL outputs cut into many slabs (the 256x256 weight gradients of the encoder / decoder
// projections: 16 tiles x ~31 slabs): one thread per output float4 leaves 64 workgroups walking 31 dependent-latency
// loads each (8 us for 8 MB).  Here the 4 wavefronts of a workgroup share 64 output float4s and take the slabs
// round-robin (wave g: slabs g, g+4, ...), partial sums meet in LDS in fixed order (deterministic); 4x the
// workgroups, a quarter of the loads per thread, every load a 1 KB wave-contiguous segment.
__global__ __launch_bounds__(256) void gemm_splitk_reduce_sg_kernel(GemmParams p) {
  __shared__ float4 red[3][64];
  const long total4 = ((long)p.M * p.N) >> 2;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + lane;
  const float4* sl = reinterpret_cast<const float4*>(p.slabs);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float amx = 0.f;
  if (i < total4) {
#pragma unroll 8
    for (int s = g; s < p.splits; s += 4) {
      const float4 t = sl[(long)s * total4 + i];
      v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
  }
  if (g > 0) red[g - 1][lane] = v;
  __syncthreads();
  if (g == 0 && i < total4) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = red[k][lane];
      v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    const long e = i << 2;
    const int m = (int)(e / p.N), n = (int)(e - (long)m * p.N);
    if (p.vecC) {
      epilogue_store4(p, v, m, n, amx);
    } else {
      float* c = p.C + (long)m * p.ldc + n;
      c[0] = epilogue_one(p, v.x, m, n, amx);
      c[1] = epilogue_one(p, v.y, m, n + 1, amx);
      c[2] = epilogue_one(p, v.z, m, n + 2, amx);
      c[3] = epilogue_one(p, v.w, m, n + 3, amx);
    }
  }
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (p.rowsum && gid < p.M) {
    float r = 0.f;
    for (int s = 0; s < p.splits; ++s) r += p.rs_slabs[(long)s * p.M + gid];
    p.rowsum[gid] = p.rowsum_acc ? p.rowsum[gid] + r : r;
  }
  amax_commit(p.amax_out, amx);
}

// Column sums of a row-major (M, N) matrix: out[n] = sum_m X[m, n]  (bias gradients).
// Stage 1: grid (ceil(N/256), GY): a workgroup reduces a (rows x 256 columns) slab with 16-byte loads
// (wave w takes rows r0+w, r0+w+4, ...), folds its 4 wavefronts through LDS and stores one partial
// row.  Stage 2 sums the GY partial rows.  No atomics: same-address fp32 atomics from hundreds of
// workgroups serialise at the memory side.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ X, float* __restrict__ part,
                                                             int M, int N, int ld, int rows_per_block, int vec) {
  __shared__ float4 red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < N) {
    if (vec && c + 3 < N) {
#pragma unroll 4
      for (int r = r0 + w; r < r1; r += 4) {
        const float4 v = *reinterpret_cast<const float4*>(X + (long)r * ld + c);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    } else {
      for (int r = r0 + w; r < r1; r += 4) {
        const float* src = X + (long)r * ld + c;
        acc.x += src[0];
        if (c + 1 < N) acc.y += src[1];
        if (c + 2 < N) acc.z += src[2];
        if (c + 3 < N) acc.w += src[3];
      }
    }
  }
  red[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < N) {
    float4 t = red[0][lane];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      t.x += red[i][lane].x; t.y += red[i][lane].y; t.z += red[i][lane].z; t.w += red[i][lane].w;
    }
    float* dst = part + (long)blockIdx.y * N + c;
    dst[0] = t.x;
    if (c + 1 < N) dst[1] = t.y;
    if (c + 2 < N) dst[2] = t.z;
    if (c + 3 < N) dst[3] = t.w;
  }
}

// out[n] (+)= sum_g part[g][n]
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                           int G, int N, int accumulate) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = accumulate ? out[n] : 0.f;
#pragma unroll 8
  for (int g = 0; g < G; ++g) s += part[(long)g * N + n];
  out[n] = s;
}

static int colsum_gy(int M, int N) {
  const int gx = (N + 255) / 256;
  int gy = std::max(1, std::min((M + 63) / 64, std::max(1, 512 / gx)));
  return std::min(gy, 256);
}

// combine kernel for the slabs of p (p.splits > 1)
void splitk_reduce_launch(const GemmParams& p, const float* workspace, hipStream_t s) {
  const int M = p.M, N = p.N;
  const long total = (long)M * N;
  const bool vec = (N % 4 == 0) && aligned16(workspace) && (total % 4 == 0);
  const long work = vec ? total / 4 : total;
  const int blocks = (int)std::min<long>((std::max<long>(work, M) + 255) / 256, 2048);
  ProfScope prof(PROF_HBM, (p.splits + 1.0 + (p.resid ? 1.0 : 0.0) + (p.aux ? 1.0 : 0.0) + (p.accumulate ? 1.0 : 0.0)) * 4.0 * total, s,
                 "rscotr::gemm_splitk_reduce_kernel");
  if (vec && p.splits >= 8 && blocks < 512 && (work + 63) / 64 * 256 >= M)
    gemm_splitk_reduce_sg_kernel<<<(unsigned)((work + 63) / 64), 256, 0, s>>>(p);
  else if (vec) gemm_splitk_reduce_kernel<true><<<blocks, 256, 0, s>>>(p);
  else gemm_splitk_reduce_kernel<false><<<blocks, 256, 0, s>>>(p);
}

// One workgroup = 256 output float4s (or row sums) of one pending problem: C[m, n..n+3] += sum_s slab_s (fixed order).
__global__ __launch_bounds__(256) void splitk_flush_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ wgmap) {
  const int entry = wgmap[2 * blockIdx.x], chunk = wgmap[2 * blockIdx.x + 1];
  const int64_t* t = table + (long)entry * 8;
  const float4* sl = reinterpret_cast<const float4*>(t[0]);
  const float* rsl = reinterpret_cast<const float*>(t[1]);
  float* C = reinterpret_cast<float*>(t[2]);
  float* rowsum = reinterpret_cast<float*>(t[3]);
  const int M = (int)t[4], N = (int)t[5], ldc = (int)t[6], splits = (int)t[7];
  const long total4 = ((long)M * N) >> 2;
  const long i = (long)chunk * 256 + threadIdx.x;
  if (i < total4) {
    float4 v = sl[i];
#pragma unroll 8
    for (int s = 1; s < splits; ++s) {
      const float4 u = sl[(long)s * total4 + i];
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const long e = i << 2;
    const int m = (int)(e / N), n = (int)(e - (long)m * N);
    float4* c = reinterpret_cast<float4*>(C + (long)m * ldc + n);
    float4 o = *c;
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *c = o;
  }
  if (rowsum && i < M) {
    float r = 0.f;
    for (int s = 0; s < splits; ++s) r += rsl[(long)s * M + i];
    rowsum[i] += r;
  }
}

// out[i] = sum_s slabs[s][i] (float4 lanes; n % 4 == 0)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float4* __restrict__ slabs, float4* __restrict__ out, long n4,
                                                       int splits) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 a = slabs[i];
    for (int s = 1; s < splits; ++s) {
      const float4 v = slabs[(long)s * n4 + i];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    out[i] = a;
  }
}

void launch_slab_sum(const float* slabs, float* out, long n4, int splits, hipStream_t s) {
  slab_sum_kernel<<<(unsigned)std::min<long>((n4 + 255) / 256, 1024), 256, 0, s>>>(reinterpret_cast<const float4*>(slabs),
                                                                                 reinterpret_cast<float4*>(out), n4, splits);
}
}  // namespace rscotr
using namespace rscotr;

// table: device (n, 8) int64 rows {slabs, row-sum slabs | 0, C, rowsum | 0, M, N, ldc, splits} (N % 4 == 0, ldc % 4 == 0,
// 16-byte aligned pointers: caller-checked); wgmap: device (nwg, 2) int32 rows {table row, chunk of 256 float4s}, with
// ceil(max(M * N / 4, M) / 256) chunks per row.
extern "C" int rscotr_splitk_flush(const int64_t* table, const int32_t* wgmap, int nwg, double bytes, void* stream) {
  if (nwg < 0) return fail(RSCOTR_E_SHAPE, "rscotr_splitk_flush: negative workgroup count");
  if (nwg == 0) return RSCOTR_OK;
  if (!table || !wgmap) return fail(RSCOTR_E_ARG, "rscotr_splitk_flush: null pointer");
  ProfScope prof(PROF_HBM, bytes, (hipStream_t)stream, "rscotr::splitk_flush_kernel");
  splitk_flush_kernel<<<dim3((unsigned)nwg), 256, 0, (hipStream_t)stream>>>(table, wgmap);
  return check_launch("rscotr_splitk_flush");
}

extern "C" int64_t rscotr_colsum_f32_workspace(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (int64_t)colsum_gy(M, N) * N * 4;
}

extern "C" int rscotr_colsum_f32(const float* X, float* out, int M, int N, int ld, int accumulate,
                                 float* workspace, int64_t workspace_bytes, void* stream) {
  if (M < 0 || N < 0) return fail(RSCOTR_E_SHAPE, "rscotr_colsum_f32: negative dimension");
  if (N == 0) return RSCOTR_OK;
  if (!X || !out) return fail(RSCOTR_E_ARG, "rscotr_colsum_f32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {
    if (!accumulate) hipMemsetAsync(out, 0, (size_t)N * 4, s);
    return RSCOTR_OK;
  }
  const int gy = colsum_gy(M, N);
  if (!workspace || workspace_bytes < (int64_t)gy * N * 4)
    return fail(RSCOTR_E_ARG, "rscotr_colsum_f32: workspace of rscotr_colsum_f32_workspace() bytes required");
  const int rpb = (M + gy - 1) / gy;
  const int gyu = (M + rpb - 1) / rpb;
  const int vec = aligned16(X) && (ld % 4 == 0);
  colsum_partial_kernel<<<dim3((N + 255) / 256, gyu), 256, 0, s>>>(X, workspace, M, N, ld, rpb, vec);
  colsum_final_kernel<<<(N + 255) / 256, 256, 0, s>>>(workspace, out, gyu, N, accumulate);
  return check_launch("rscotr_colsum_f32");
}
