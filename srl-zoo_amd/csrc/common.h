// common.h — shared device/host helpers for libsrlz_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/srlz.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// error.cpp
void srlz_set_error(const char* fmt, ...);
int srlz_hip_fail(hipError_t e, const char* what);

#define SRLZ_HIP(expr)                                   \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return srlz_hip_fail(_e, #expr); \
  } while (0)

// Raise a kernel's dynamic-LDS limit once (per call site / template instantiation), not on every launch: the call is
// host overhead on a launch-bound path, and it is not a stream operation, so it must not happen while the stream is being
// captured into a hipGraph (models/learner.py::_graphStep) — after the warm-up launches every limit is already in place.
// (One host thread drives one GPU per process, so the per-site static needs no lock.)
#define SRLZ_MAX_LDS(fn, bytes)                                                                                         \
  do {                                                                                                                  \
    static int srlz_lds_set_ = -1;                                                                                      \
    if ((int)(bytes) > srlz_lds_set_) {                                                                                 \
      SRLZ_HIP(hipFuncSetAttribute((const void*)(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)));      \
      srlz_lds_set_ = (int)(bytes);                                                                                     \
    }                                                                                                                   \
  } while (0)

#define SRLZ_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      srlz_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

// Launch, then return the launch's error (a bad LDS request, a grid of 0 ...) from the calling function: a launch that is not checked
// fails silently and its consumer reads memory nobody wrote.  A templated kernel name with commas goes in parentheses.
#define SRLZ_LAUNCH(kernel, grid, block, lds_bytes, stream, ...)                 \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, __VA_ARGS__);     \
    SRLZ_HIP(hipGetLastError());                                                 \
  } while (0)

static inline hipStream_t as_stream(srlz_stream_t s) { return (hipStream_t)s; }

// Observed (not contractual) dispatch: block b runs on XCD b % 8.  Give every XCD a contiguous run of tiles so
// neighbouring tiles (which share halo rows) hit the same L2.  Bijective for any nb.
__device__ __forceinline__ int xcd_remap(int bid, int nb) {
  const int q = nb >> 3, r = nb & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// a * b + c with a < 2^24 and a wave-uniform 0 <= b < 2^24, as the one full-rate instruction it is (hipcc turns the intrinsic form
// __umul24(a, b) + c into a quarter-rate v_mad_u64_u32 whenever it cannot see the ranges, and plain 32-bit products are quarter-rate
// v_mul_lo_u32): the pixel-offset arithmetic of the stagings, where every issue slot is paid for in matrix time
__device__ __forceinline__ unsigned mad_u24(unsigned a, int b_uniform, unsigned c) {
  unsigned r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b_uniform), "v"(c));
  return r;
}

// Granlund-Montgomery division by an invariant for 31-bit dividends: l = ceil(log2 d), m = floor(2^(31+l) / d) + 1 (< 2^32),
// q / d == umulhi(q, m) >> (l - 1) for every 0 <= q < 2^31 (d >= 2).  A run-time integer division is ~20 VALU instructions.
static inline void fastdiv_init(unsigned d, unsigned* m, int* sh) {
  int l = 0;
  while ((1u << l) < d) ++l;
  if (l == 0) l = 1;  // d == 1: m = 2^32 does not fit; callers have d >= 2
  *m = (unsigned)((((unsigned long long)1 << (31 + l)) / d) + 1);
  *sh = l - 1;
}
__device__ __forceinline__ int fastdiv(int q, unsigned m, int sh) { return (int)(__umulhi((unsigned)q, m) >> sh); }

// A buffer resource over `bytes` bytes at `p` (raw, unstrided): a buffer access whose offset lies outside is DROPPED by the hardware
// (a load returns 0), which makes a conditional access branch-free — the lane that must not write passes its file's *_DROP offset.
// That matters beyond the branch itself: vmcnt counts stores too and is in-order, and behind a store inside a branch hipcc can only
// wait for everything, so every later wait for a prefetch would also wait for these stores' HBM round trip.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_buffer(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

// Epilogue option of the conv2 / conv3 data-gradient launches, whose output is the gradient of a POOLED map (conv64_dgrad_poolsum_kernel,
// conv64_wino_kernel<.., true>): instead of BatchNorm-forward statistics the tile's partial record receives the two BatchNorm-BACKWARD
// sums of the block that produced the pooled map,  sum dz  and  sum dz*xhat  with dz = d pooled where pooled > 0 (the gradient lives at
// the window's argmax, and the pooled value IS relu(bn(y)) there: xhat follows from it) — what bn_relu_pool_bwd_reduce computes in a
// pass of its own over (d pooled, pooled, argmax).  y / argmax are only touched for channels whose BatchNorm scale is (almost) 0 (xhat
// cannot be recovered from the pooled value there).
namespace {
struct PoolSum {
  const float* pooled;    // [N,Hd,Wd,64] like the launch's dst; NULL = off
  const float* bnp;       // records of the pooled block's BatchNorm (256 floats per group)
  const float* y;         // raw convolution output under the pooling [N,H,W,64]
  const uint8_t* argmax;  // [N,Hd,Wd,64]
  long long y_gstride;    // floats between two groups' images in y
  int H, W, pad;
};
}  // namespace
#define SRLZ_NO_POOLSUM PoolSum{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (d, i) before (e, j) in the order of the key (value, index): smaller value first, equal values by the lower index
__device__ __forceinline__ bool key_less_d(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// Minimum of (d, i) by that key over the wave, left in every lane.  A comparison, not a sum: the result is the same in any order.
__device__ __forceinline__ void wave_min_key_d(double& d, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double e = __shfl_xor(d, o, 64);
    const int j = __shfl_xor(i, o, 64);
    if (key_less_d(e, j, d, i)) {
      d = e;
      i = j;
    }
  }
}

// Sum of v over a block of NWAVES waves in a fixed order (deterministic): fp64 wave sums, one LDS slot per wave, one barrier.
// Contract: blockDim.x == 64 * NWAVES, EVERY thread of the block calls it, at most once per kernel (the slots are not
// re-armed); the sums are meant for thread 0.  block_wave_sums_d returns the slots, block_sum_d adds them left to right,
// ((s0 + s1) + s2) + ..., block_sum_pairs_d as (s0 + s1) + (s2 + s3).
template <int NWAVES = 4>
__device__ __forceinline__ const double* block_wave_sums_d(double v) {
  __shared__ double slots[NWAVES];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  return slots;
}

template <int NWAVES = 4>
__device__ __forceinline__ double block_sum_d(double v) {
  const double* s = block_wave_sums_d<NWAVES>(v);
  double t = s[0];
#pragma unroll
  for (int w = 1; w < NWAVES; ++w) t += s[w];
  return t;
}

__device__ __forceinline__ double block_sum_pairs_d(double v) {
  const double* s = block_wave_sums_d<4>(v);
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// A thread's four channels (c4 * 4 ..) of a BatchNorm record bnp[256]: [0,64) mean, [64,128) invstd, [128,192) scale, [192,256) shift
struct BnRec4 { f32x4 mean, invstd, sc, sh; };
__device__ __forceinline__ BnRec4 load_bn_quads(const float* __restrict__ bnp, int c4) {
  return {*(const f32x4*)(bnp + c4 * 4), *(const f32x4*)(bnp + 64 + c4 * 4), *(const f32x4*)(bnp + 128 + c4 * 4),
          *(const f32x4*)(bnp + 192 + c4 * 4)};
}

// Block combine of the BatchNorm-backward sums.  Contract: 256 threads, thread = (pixel row threadIdx.x >> 4, channel quad
// threadIdx.x & 15) holding the fp64 sums s1 (dz) and s2 (dz * xhat) of its 4 channels; EVERY thread calls it.  The 16 pixel rows are
// added in row order r = 0..15 (deterministic) and row[0..64) = s1, row[64..128) = s2 are stored as T.
// These sums feed dy = scale*(dz - mean(dz) - xhat*mean(dz*xhat)): an error in either mean is a per-channel CONSTANT added to every dy
// element, which the following weight-gradient sums coherently over all (non-negative, post-ReLU) inputs.  fp32 accumulation here costs
// 1e-3..1e-2 of relative accuracy in dW; fp64 is free in an HBM-bound kernel.
template <typename T>
__device__ __forceinline__ void bn_bwd_combine_store(const double (&s1)[4], const double (&s2)[4], T* __restrict__ row) {
  __shared__ double sm[16][128];
  const int c4 = threadIdx.x & 15, prow = threadIdx.x >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) { sm[prow][c4 * 4 + j] = s1[j]; sm[prow][64 + c4 * 4 + j] = s2[j]; }
  __syncthreads();
  if (threadIdx.x < 128) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += sm[r][threadIdx.x];
    row[threadIdx.x] = (T)s;
  }
}

// Grid-stride walk over n floats, four at a time: quad(i) for every whole f32x4 (elements 4i .. 4i+3), then one(i) for every element
// of the tail n & 3.  The buffers behind quad() must be 16-byte aligned.
template <class F4, class F1>
__device__ __forceinline__ void for_each_quad(long long n, F4 quad, F1 one) {
  const long long n4 = n >> 2, stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = first; i < n4; i += stride) quad(i);
  for (long long i = n4 * 4 + first; i < n; i += stride) one(i);
}
