#include "common.h"
#include <algorithm>
// Value range of a tensor for the fp16 split product: slot = max(slot, bit pattern of max |X[r, c]|) over rows x cols with
// row stride ld (slot = a range word of kAmaxPlanes sub-words, common.h).  The caller zeroes the slot (one memset for all slots of an iteration); the maximum is taken per lane,
// per wavefront (shuffles), per workgroup (LDS), and the workgroup marks the byte of its binade in the word (common.h: an idempotent plain
// store — no atomics, deterministic).  NaNs compare above every finite pattern.
namespace rscotr {
// max over this thread's share (thread tid of nth) of the bit patterns of |X[r, c]|
__device__ __forceinline__ unsigned amax_scan(const float* __restrict__ X, long rows, int cols, int ld, bool vec, long tid, long nth) {
  unsigned m = 0u;
  if (vec) {
    const int c4 = cols >> 2;
    const long n4 = rows * c4;
    for (long i = tid; i < n4; i += nth) {
      const long r = i / c4;
      const int c = (int)(i - r * c4) << 2;
      const uint4 v = *reinterpret_cast<const uint4*>(X + r * ld + c);
      m = max(max(m, v.x & 0x7fffffffu), max(max(v.y & 0x7fffffffu, v.z & 0x7fffffffu), v.w & 0x7fffffffu));
    }
  } else {
    const long n = rows * cols;
    for (long i = tid; i < n; i += nth) {
      const long r = i / cols;
      m = max(m, __float_as_uint(X[r * ld + (i - r * cols)]) & 0x7fffffffu);
    }
  }
  return m;
}

// wavefront (shuffles) -> workgroup (sm: 4 words of LDS) -> the byte of the binade in the word
__device__ __forceinline__ void amax_mark(unsigned m, unsigned* sm, unsigned* __restrict__ slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    if (m) range_mark(slot, range_byte(m));  // (a plain byte store: common.h)
  }
}

__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ X, long rows, int cols, int ld, int vec,
                                                   unsigned* __restrict__ slot) {
  __shared__ unsigned sm[4];
  amax_mark(amax_scan(X, rows, cols, ld, vec, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256), sm, slot);
}

// The same for MANY tensors in one launch (the operands of the grouped weight-gradient launch that arrived without a range):
// table rows {X, rows, cols, ld, slot, first block}; entry e owns blocks [first_e, first_{e+1}) (the last one up to gridDim.x).
__global__ __launch_bounds__(256) void amax_group_kernel(const int64_t* __restrict__ table, int n) {
  __shared__ unsigned sm[4];
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)table[(long)mid * 6 + 5] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int64_t* t = table + (long)lo * 6;
  const float* X = reinterpret_cast<const float*>(t[0]);
  const long rows = t[1];
  const int cols = (int)t[2], ld = (int)t[3];
  unsigned* slot = reinterpret_cast<unsigned*>(t[4]);
  const int first = (int)t[5], nb = (lo + 1 < n ? (int)table[(long)(lo + 1) * 6 + 5] : (int)gridDim.x) - first;
  const long tid = (long)(blockIdx.x - first) * 256 + threadIdx.x, nth = (long)nb * 256;
  amax_mark(amax_scan(X, rows, cols, ld, ((t[0] & 15) == 0) && cols % 4 == 0 && ld % 4 == 0, tid, nth), sm, slot);
}
}  // namespace rscotr

extern "C" int rscotr_amax_group(const int64_t* table, int n, int total_blocks, void* stream) {
  if (n < 0 || total_blocks < 0) return rscotr::fail(RSCOTR_E_SHAPE, "rscotr_amax_group: negative count");
  if (n == 0 || total_blocks == 0) return RSCOTR_OK;
  if (!table) return rscotr::fail(RSCOTR_E_ARG, "rscotr_amax_group: null table");
  rscotr::amax_group_kernel<<<dim3((unsigned)total_blocks), 256, 0, (hipStream_t)stream>>>(table, n);
  return rscotr::check_launch("rscotr_amax_group");
}

extern "C" int rscotr_amax_f32(const float* X, int64_t rows, int cols, int ld, uint32_t* slot, void* stream) {
  if (rows < 0 || cols < 0 || ld < cols) return rscotr::fail(RSCOTR_E_SHAPE, "rscotr_amax_f32: bad shape");
  if (rows == 0 || cols == 0) return RSCOTR_OK;
  if (!X || !slot) return rscotr::fail(RSCOTR_E_ARG, "rscotr_amax_f32: null pointer");
  const int vec = rscotr::aligned16(X) && cols % 4 == 0 && ld % 4 == 0;
  const long n = rows * (long)cols;
  const unsigned grid = (unsigned)std::max<long>(1, std::min<long>(256, (n + 8191) / 8192));
  rscotr::amax_kernel<<<dim3(grid), 256, 0, (hipStream_t)stream>>>(X, rows, cols, ld, vec, slot);
  return rscotr::check_launch("rscotr_amax_f32");
}
