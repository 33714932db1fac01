// supervised.hip — the two kernels the supervised baseline adds to the step (reference srl_baselines/supervised.py:85,101-105 and
// models/supervised.py:26): nn.MSELoss() of the predicted states against the ground-truth states with its gradient in the same
// launch, and F.dropout with a mask the caller drew.  Plain vector loads and stores; no atomics, so every result is bit-identical
// between runs.
#include "common.h"

namespace {

constexpr int MSE_THREADS = 1024;           // ONE workgroup: 16 waves, a fixed summation order, no hand-off between workgroups
constexpr long long MSE_MAX = 1LL << 20;    // B * S accepted (1024 elements per thread at the limit)

// loss[0] = fp32(sum_i (p_i - t_i)^2 / n) — fp64 from the first product on, one rounding — and dpred_unit_i = (p_i - t_i) * (2 / n)
__global__ __launch_bounds__(MSE_THREADS) void mse_target_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                 long long n, float two_over_n, float* __restrict__ loss,
                                                                 float* __restrict__ dpred_unit) {
  double acc = 0.0;
  const long long n4 = n >> 2;
  for (long long i = threadIdx.x; i < n4; i += MSE_THREADS) {
    const f32x4 p = *(const f32x4*)(pred + i * 4);
    const f32x4 t = *(const f32x4*)(target + i * 4);
    f32x4 g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = p[j] - t[j];
      acc += (double)d * (double)d;
      g[j] = d * two_over_n;
    }
    *(f32x4*)(dpred_unit + i * 4) = g;
  }
  for (long long i = n4 * 4 + threadIdx.x; i < n; i += MSE_THREADS) {
    const float d = pred[i] - target[i];
    acc += (double)d * (double)d;
    dpred_unit[i] = d * two_over_n;
  }
  const double s = block_sum_d<MSE_THREADS / 64>(acc);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}

// y = (x * mask) / keep, the fp32 operations of `x * mask / (1 - p)` in that order (mask: 0 or 1 per element)
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask, float keep,
                                                     float* __restrict__ y, long long n) {
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 v = *(const f32x4*)(x + i * 4);
    const uchar4 m = *(const uchar4*)(mask + i * 4);
    f32x4 o;
    o[0] = __fdiv_rn(v[0] * (m.x ? 1.f : 0.f), keep);
    o[1] = __fdiv_rn(v[1] * (m.y ? 1.f : 0.f), keep);
    o[2] = __fdiv_rn(v[2] * (m.z ? 1.f : 0.f), keep);
    o[3] = __fdiv_rn(v[3] * (m.w ? 1.f : 0.f), keep);
    *(f32x4*)(y + i * 4) = o;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = __fdiv_rn(x[i] * (mask[i] ? 1.f : 0.f), keep);
}

static int dropout_launch(const char* what, const float* x, const unsigned char* mask, float keep, float* y, int rows, int cols,
                          hipStream_t st) {
  SRLZ_REQUIRE(x && mask && y, SRLZ_ERR_NULL, "%s: null pointer", what);
  SRLZ_REQUIRE(rows >= 1 && cols >= 1, SRLZ_ERR_BAD_DESC, "%s: rows = %d, cols = %d", what, rows, cols);
  SRLZ_REQUIRE(keep > 0.f && keep <= 1.f, SRLZ_ERR_BAD_DESC, "%s: keep probability %g outside (0, 1]", what, (double)keep);
  SRLZ_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)mask & 3) == 0, SRLZ_ERR_BAD_DESC,
               "%s: x / y must be 16-byte aligned and the mask 4-byte aligned", what);
  const long long n = (long long)rows * cols;
  long long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  SRLZ_LAUNCH(dropout_kernel, dim3((int)blocks), dim3(256), 0, st, x, mask, keep, y, n);
  return 0;
}

}  // namespace

extern "C" int srlz_mse_target_fwd(const float* pred, const float* target, int B, int S, float* loss, float* dpred_unit,
                                   srlz_stream_t stream) {
  SRLZ_REQUIRE(pred && target && loss && dpred_unit, SRLZ_ERR_NULL, "mse_target_fwd: null pointer");
  SRLZ_REQUIRE(B >= 1 && S >= 1, SRLZ_ERR_BAD_DESC, "mse_target_fwd: B = %d, S = %d", B, S);
  const long long n = (long long)B * S;
  SRLZ_REQUIRE(n <= MSE_MAX, SRLZ_ERR_BAD_DESC, "mse_target_fwd: B * S = %lld exceeds the %lld elements one launch takes", n, MSE_MAX);
  SRLZ_REQUIRE((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred_unit) & 15) == 0, SRLZ_ERR_BAD_DESC,
               "mse_target_fwd: pred / target / dpred_unit must be 16-byte aligned");
  SRLZ_LAUNCH(mse_target_kernel, dim3(1), dim3(MSE_THREADS), 0, as_stream(stream), pred, target, n, 2.0f / (float)n, loss, dpred_unit);
  return 0;
}

extern "C" int srlz_dropout_fwd(const float* x, const unsigned char* mask, float keep, float* y, int rows, int cols,
                                srlz_stream_t stream) {
  return dropout_launch("dropout_fwd", x, mask, keep, y, rows, cols, as_stream(stream));
}

extern "C" int srlz_dropout_bwd(const float* dy, const unsigned char* mask, float keep, float* dx, int rows, int cols,
                                srlz_stream_t stream) {
  return dropout_launch("dropout_bwd", dy, mask, keep, dx, rows, cols, as_stream(stream));
}
