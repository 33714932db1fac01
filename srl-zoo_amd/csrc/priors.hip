// priors.hip — the reward-prior and episode-prior losses (reference losses/losses.py:290-359, losses/utils.py:120-134,
// models/priors.py:129-175) on gfx950, wave64.
//
// reward-prior: 1 - mean_j |clamp(corr[S, j], -1, 1)| over the S + 1 entries of the last row of the correlation matrix of
//   X = cat([states, r], 1)^T.  Only that row is ever read, so the forward needs each column's mean and variance and its covariance
//   with r: one workgroup of 16 waves, fp64 sums in a fixed order (rows strided over the waves, then the 16 partials in wave order).
//   The backward is elementwise on the statistics the forward leaves in `ws`:
//     d corr_k / d s[b,k] = inv_r * inv_k / (B-1) * (c_b - cov_k * inv_k^2 * a_bk),  a = s - mean_k, c = r - mean_r
//   (the mean-subtraction terms cancel because sum_b a_bk = sum_b c_b = 0).
//
// episode-prior: BCE(sum) of Discriminator(cat(s_i, s_{o_i})) against same_i, the discriminator
//   Linear(2S,64)-ReLU-Linear(64,64)-ReLU-Linear(64,1)-Sigmoid, with the gradient into the states reversed (ReverseLayerF, lambda 1).
//   forward: one launch, 16 rows per workgroup (4 per wave, lane = hidden unit).  W1 is staged through LDS 64 columns at a time,
//     transposed, together with the 16 gathered input rows (the concat is never written).  Per-row BCE in fp64; the workgroup that
//     finishes last (an integer ticket, reset by that workgroup) adds the B row terms in row order.
//   backward: two launches.  (1) per row: dz, dh2, dh1 and d input (2S) into the workspace.  (2) fixed-order reductions over the
//     rows: dW1 / dW2 / dW3 / db1 / db2 / db3 straight into the gradient buffers, and the reversed state gradient
//     dstates[i] = -(dx[i, :S] + sum_{j ascending, o_j == i} dx[j, S:]) — a scan over j, so repeated and missing indices of balanced
//     sampling need no host-side inverse list.
// No float atomics anywhere; every sum has one order, so results are bit-identical from run to run.
#include "common.h"

namespace {

constexpr int RP_THREADS = 1024;
constexpr int RP_WAVES = RP_THREADS / 64;
constexpr double RP_EPS = 1e-8;  // correlationMatrix(eps=1e-8)

// ws (doubles): [0] mean_r, [1] inv_r, [2] var_r, [3] unused, then 4 per column k: mean_k, inv_k, corr_k (before the clamp), cov_k
__global__ __launch_bounds__(RP_THREADS) void reward_prior_fwd_kernel(const float* __restrict__ s, const float* __restrict__ r,
                                                                      int B, int S, float* __restrict__ out,
                                                                      double* __restrict__ ws) {
  __shared__ double red[RP_WAVES][64];
  __shared__ double red2[RP_WAVES][64];
  __shared__ double colmean[64];
  __shared__ double rstat[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // reward statistics
  double acc = 0.0;
  for (int b = tid; b < B; b += RP_THREADS) acc += (double)r[b];
  acc = wave_sum_d(acc);
  if (lane == 0) red[wave][0] = __shfl(acc, 0, 64);
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < RP_WAVES; ++w) t += red[w][0];
    rstat[0] = t / (double)B;
  }
  __syncthreads();
  const double mr = rstat[0];
  acc = 0.0;
  for (int b = tid; b < B; b += RP_THREADS) {
    const double c = (double)r[b] - mr;
    acc += c * c;
  }
  acc = wave_sum_d(acc);
  __syncthreads();
  if (lane == 0) red[wave][0] = __shfl(acc, 0, 64);
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < RP_WAVES; ++w) t += red[w][0];
    const double var_r = t / (double)(B - 1);
    rstat[1] = 1.0 / sqrt(var_r + RP_EPS);
    ws[0] = mr;
    ws[1] = rstat[1];
    ws[2] = var_r;
    ws[3] = 0.0;
  }
  __syncthreads();
  const double inv_r = rstat[1];

  double total = 0.0;  // sum_k |clamp(corr_k)| (wave 0, every lane the same value)
  for (int c0 = 0; c0 < S; c0 += 64) {
    const int k = c0 + lane;
    const bool col = k < S;
    double s1 = 0.0;
    if (col)
      for (int b = wave; b < B; b += RP_WAVES) s1 += (double)s[(size_t)b * S + k];
    red[wave][lane] = s1;
    __syncthreads();
    if (wave == 0) {
      double t = 0.0;
      for (int w = 0; w < RP_WAVES; ++w) t += red[w][lane];
      colmean[lane] = t / (double)B;
    }
    __syncthreads();
    const double m = colmean[lane];
    double s2 = 0.0, s3 = 0.0;
    if (col)
      for (int b = wave; b < B; b += RP_WAVES) {
        const double a = (double)s[(size_t)b * S + k] - m;
        s2 += a * a;
        s3 += a * ((double)r[b] - mr);
      }
    red[wave][lane] = s2;
    red2[wave][lane] = s3;
    __syncthreads();
    if (wave == 0) {
      double v = 0.0, cv = 0.0;
      for (int w = 0; w < RP_WAVES; ++w) {
        v += red[w][lane];
        cv += red2[w][lane];
      }
      double contrib = 0.0;
      if (col) {
        const double var = v / (double)(B - 1), cov = cv / (double)(B - 1);
        const double inv = 1.0 / sqrt(var + RP_EPS);
        const double corr = cov * inv * inv_r;
        double* wk = ws + 4 + 4 * (size_t)k;
        wk[0] = m;
        wk[1] = inv;
        wk[2] = corr;
        wk[3] = cov;
        contrib = fabs(fmin(fmax(corr, -1.0), 1.0));
      }
      contrib = wave_sum_d(contrib);
      total += __shfl(contrib, 0, 64);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double var_r = ws[2];
    const double corr_rr = var_r * inv_r * inv_r;
    total += fabs(fmin(fmax(corr_rr, -1.0), 1.0));
    out[0] = (float)(1.0 - total / (double)(S + 1));
  }
}

__global__ __launch_bounds__(256) void reward_prior_bwd_kernel(const float* __restrict__ s, const float* __restrict__ r,
                                                               const double* __restrict__ ws, const float* __restrict__ g, int B,
                                                               int S, float* __restrict__ ds) {
  const long long n = (long long)B * S;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int b = (int)(e / S), k = (int)(e - (long long)b * S);
  const double* wk = ws + 4 + 4 * (size_t)k;
  const double corr = wk[2];
  // d(1 - mean|clamp(x)|)/dx: -sign(x) / (S+1) where -1 <= x <= 1 (torch: abs' = sign with sign(0) = 0, clamp' passes inclusive)
  double gk = 0.0;
  if (corr >= -1.0 && corr <= 1.0 && corr != 0.0) gk = (corr > 0.0 ? -1.0 : 1.0) / (double)(S + 1);
  gk *= (double)g[0];
  const double mr = ws[0], inv_r = ws[1];
  const double m = wk[0], inv = wk[1], cov = wk[3];
  const double a = (double)s[e] - m, c = (double)r[b] - mr;
  ds[e] = (float)(gk * inv_r * inv / (double)(B - 1) * (c - cov * inv * inv * a));
}

// ---- episode prior ----------------------------------------------------------------------------------------------------
constexpr int EP_H = 64;    // Discriminator hidden width (models/priors.py:146-153)
constexpr int EP_ROWS = 16; // rows per forward workgroup: 4 waves x 4 rows
constexpr int EP_RPW = 4;

__device__ __forceinline__ int ep_other(const int* __restrict__ others, int b, int B) {
  const int o = others[b];
  return (o >= 0 && o < B) ? o : b;  // an index outside the batch pairs the row with itself, in the forward and both backward passes
}

__global__ __launch_bounds__(256) void episode_prior_fwd_kernel(
    const float* __restrict__ st, const int* __restrict__ others, const float* __restrict__ same, int B, int S,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ h1o, float* __restrict__ h2o,
    float* __restrict__ po, double* __restrict__ rowloss, float* __restrict__ out, unsigned* __restrict__ ticket) {
  __shared__ float wt[64][EP_H + 1];
  __shared__ float xs[EP_ROWS][64];
  __shared__ float hs[EP_ROWS][EP_H];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * EP_ROWS;
  const int K = 2 * S;

  float acc[EP_RPW];
  const float bias1 = b1[lane];
#pragma unroll
  for (int q = 0; q < EP_RPW; ++q) acc[q] = bias1;
  for (int t0 = 0; t0 < K; t0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * EP_H; e += 256) {
      const int j = e >> 6, tt = e & 63, t = t0 + tt;
      wt[tt][j] = t < K ? w1[(size_t)j * K + t] : 0.f;
    }
    for (int e = tid; e < EP_ROWS * 64; e += 256) {
      const int rr = e >> 6, tt = e & 63, b = row0 + rr, t = t0 + tt;
      float v = 0.f;
      if (b < B && t < K) v = t < S ? st[(size_t)b * S + t] : st[(size_t)ep_other(others, b, B) * S + (t - S)];
      xs[rr][tt] = v;
    }
    __syncthreads();
    const int n = min(64, K - t0);
    for (int tt = 0; tt < n; ++tt) {
      const float w = wt[tt][lane];
#pragma unroll
      for (int q = 0; q < EP_RPW; ++q) acc[q] = fmaf(w, xs[wave * EP_RPW + q][tt], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < EP_RPW; ++q) {
    const int b = row0 + wave * EP_RPW + q;
    const float h = fmaxf(acc[q], 0.f);
    hs[wave * EP_RPW + q][lane] = h;
    if (b < B) h1o[(size_t)b * EP_H + lane] = h;
  }
  __syncthreads();
  for (int e = tid; e < EP_H * EP_H; e += 256) {
    const int j = e >> 6, k = e & 63;
    wt[k][j] = w2[e];
  }
  __syncthreads();
  const float bias2 = b2[lane], w3l = w3[lane], bias3 = b3[0];
#pragma unroll
  for (int q = 0; q < EP_RPW; ++q) {
    const int rr = wave * EP_RPW + q, b = row0 + rr;
    float a2 = bias2;
    for (int k = 0; k < EP_H; ++k) a2 = fmaf(wt[k][lane], hs[rr][k], a2);
    const float h2 = fmaxf(a2, 0.f);
    if (b < B) h2o[(size_t)b * EP_H + lane] = h2;
    const float z = __shfl(wave_sum(w3l * h2), 0, 64) + bias3;
    if (lane == 0 && b < B) {
      const float p = 1.f / (1.f + expf(-z));  // the fp32 sigmoid output: every use below sees this rounded value
      const double y = (double)same[b];
      const double lp = fmax(log((double)p), -100.0), lq = fmax(log((double)(1.f - p)), -100.0);
      po[b] = p;
      rowloss[b] = -(y * lp + (1.0 - y) * lq);
    }
  }
  // the last workgroup to finish adds the row terms, in row order
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (wave == 0) {
    double t = 0.0;
    for (int b = lane; b < B; b += 64) t += rowloss[b];
    t = __shfl(wave_sum_d(t), 0, 64);
    if (lane == 0) {
      out[0] = (float)t;
      atomicExch(ticket, 0u);
    }
  }
}

// (1) per row: one wave per row
__global__ __launch_bounds__(256) void episode_prior_bwd_rows_kernel(
    const float* __restrict__ same, const float* __restrict__ g, int B, int S, const float* __restrict__ w1,
    const float* __restrict__ w2, const float* __restrict__ w3, const float* __restrict__ h1, const float* __restrict__ h2,
    const float* __restrict__ po, float* __restrict__ dz_o, float* __restrict__ dh1_o, float* __restrict__ dh2_o,
    float* __restrict__ dx_o) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // (whole waves: no workgroup barrier below)
  const int K = 2 * S;
  const float p = po[b], y = same[b];
  // BCELoss backward (grad * (p - y) / max((1 - p) p, 1e-12)), then Sigmoid's grad * (1 - p) * p, in fp32 as torch forms them
  const float pq = (1.f - p) * p;
  const float dp = (g[0] * (p - y)) / fmaxf(pq, 1e-12f);
  const float dz = (dp * (1.f - p)) * p;
  const float dh2 = h2[(size_t)b * EP_H + lane] > 0.f ? dz * w3[lane] : 0.f;
  float a = 0.f;
  for (int k = 0; k < EP_H; ++k) a = fmaf(w2[k * EP_H + lane], __shfl(dh2, k, 64), a);
  const float dh1 = h1[(size_t)b * EP_H + lane] > 0.f ? a : 0.f;
  if (lane == 0) dz_o[b] = dz;
  dh1_o[(size_t)b * EP_H + lane] = dh1;
  dh2_o[(size_t)b * EP_H + lane] = dh2;
  for (int t0 = 0; t0 < K; t0 += 64) {
    const int t = t0 + lane;
    const int tc = t < K ? t : K - 1;
    float d = 0.f;
    for (int j = 0; j < EP_H; ++j) d = fmaf(w1[(size_t)j * K + tc], __shfl(dh1, j, 64), d);
    if (t < K) dx_o[(size_t)b * K + t] = d;
  }
}

// (2) fixed-order reductions over the rows.  Workgroup roles:
//   [0, B)                      reversed state gradient of row i
//   [B, B + 64 * nt)            dW1[j, t-chunk of 256]
//   [B + 64 * nt, ... + 64)     dW2[j, :], db2[j], db1[j], dW3[j] (and db3 in the first)
__global__ __launch_bounds__(256) void episode_prior_bwd_reduce_kernel(
    const float* __restrict__ st, const int* __restrict__ others, int B, int S, const float* __restrict__ h1,
    const float* __restrict__ h2, const float* __restrict__ dz, const float* __restrict__ dh1, const float* __restrict__ dh2,
    const float* __restrict__ dx, float* __restrict__ ds, float* __restrict__ dw1, float* __restrict__ db1,
    float* __restrict__ dw2, float* __restrict__ db2, float* __restrict__ dw3, float* __restrict__ db3) {
  __shared__ int os[256];
  const int tid = threadIdx.x;
  const int K = 2 * S, nt = (K + 255) / 256;
  const int blk = blockIdx.x;
  if (blk < B) {
    const int i = blk;
    for (int k0 = 0; k0 < S; k0 += 256) {
      const int k = k0 + tid;
      float a = k < S ? dx[(size_t)i * K + k] : 0.f;
      for (int j0 = 0; j0 < B; j0 += 256) {
        __syncthreads();
        os[tid] = j0 + tid < B ? ep_other(others, j0 + tid, B) : -1;  // (the partner the forward gathered)
        __syncthreads();
        const int n = min(256, B - j0);
        for (int jj = 0; jj < n; ++jj)
          if (os[jj] == i && k < S) a += dx[(size_t)(j0 + jj) * K + S + k];
      }
      if (k < S) ds[(size_t)i * S + k] = -a;
    }
    return;
  }
  const int r = blk - B;
  if (r < EP_H * nt) {
    const int j = r / nt, t = (r - j * nt) * 256 + tid;
    if (t >= K) return;
    float a = 0.f;
    for (int i = 0; i < B; ++i) {
      const float x = t < S ? st[(size_t)i * S + t] : st[(size_t)ep_other(others, i, B) * S + (t - S)];
      a = fmaf(dh1[(size_t)i * EP_H + j], x, a);
    }
    dw1[(size_t)j * K + t] = a;
    return;
  }
  const int j = r - EP_H * nt;
  if (tid < EP_H) {
    float a = 0.f;
    for (int i = 0; i < B; ++i) a = fmaf(dh2[(size_t)i * EP_H + j], h1[(size_t)i * EP_H + tid], a);
    dw2[j * EP_H + tid] = a;
  } else if (tid == EP_H) {
    float a = 0.f;
    for (int i = 0; i < B; ++i) a += dh2[(size_t)i * EP_H + j];
    db2[j] = a;
  } else if (tid == EP_H + 1) {
    float a = 0.f;
    for (int i = 0; i < B; ++i) a += dh1[(size_t)i * EP_H + j];
    db1[j] = a;
  } else if (tid == EP_H + 2) {
    float a = 0.f;
    for (int i = 0; i < B; ++i) a = fmaf(dz[i], h2[(size_t)i * EP_H + j], a);
    dw3[j] = a;
  } else if (tid == EP_H + 3 && j == 0) {
    float a = 0.f;
    for (int i = 0; i < B; ++i) a += dz[i];
    db3[0] = a;
  }
}

// episode workspace layout (bytes, every part 256-byte aligned): h1 [B,64], h2 [B,64], p [B], rowloss [B] (double), dz [B],
// dh1 [B,64], dh2 [B,64], dx [B,2S]
struct EpLayout {
  size_t h1, h2, p, rowloss, dz, dh1, dh2, dx, total;
};

size_t ep_align(size_t x) { return (x + 255) & ~(size_t)255; }

EpLayout ep_layout(int B, int S) {
  EpLayout L;
  size_t o = 0;
  L.h1 = o; o += ep_align((size_t)B * EP_H * 4);
  L.h2 = o; o += ep_align((size_t)B * EP_H * 4);
  L.p = o; o += ep_align((size_t)B * 4);
  L.rowloss = o; o += ep_align((size_t)B * 8);
  L.dz = o; o += ep_align((size_t)B * 4);
  L.dh1 = o; o += ep_align((size_t)B * EP_H * 4);
  L.dh2 = o; o += ep_align((size_t)B * EP_H * 4);
  L.dx = o; o += ep_align((size_t)B * 2 * S * 4);
  L.total = o;
  return L;
}

template <typename T>
T* at(void* base, size_t off) { return (T*)((char*)base + off); }

}  // namespace

extern "C" size_t srlz_reward_prior_workspace(int S) { return S > 0 ? (size_t)(4 + 4 * (size_t)S) * sizeof(double) : 0; }

extern "C" int srlz_reward_prior_fwd(const float* states, const float* rewards, int B, int S, float* out, double* ws,
                                     size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE(states && rewards && out && ws, SRLZ_ERR_NULL, "reward_prior_fwd: null pointer");
  SRLZ_REQUIRE(B >= 2 && S >= 1, SRLZ_ERR_BAD_DESC, "reward_prior_fwd: needs B >= 2 rows and S >= 1 columns (B=%d, S=%d)", B, S);
  SRLZ_REQUIRE(ws_bytes >= srlz_reward_prior_workspace(S), SRLZ_ERR_WORKSPACE, "reward_prior_fwd: workspace %zu < %zu bytes",
               ws_bytes, srlz_reward_prior_workspace(S));
  SRLZ_LAUNCH(reward_prior_fwd_kernel, dim3(1), dim3(RP_THREADS), 0, as_stream(stream), states, rewards, B, S, out, ws);
  return 0;
}

extern "C" int srlz_reward_prior_bwd(const float* states, const float* rewards, const double* ws, size_t ws_bytes, const float* g,
                                     int B, int S, float* dstates, srlz_stream_t stream) {
  SRLZ_REQUIRE(states && rewards && ws && g && dstates, SRLZ_ERR_NULL, "reward_prior_bwd: null pointer");
  SRLZ_REQUIRE(B >= 2 && S >= 1, SRLZ_ERR_BAD_DESC, "reward_prior_bwd: needs B >= 2 rows and S >= 1 columns (B=%d, S=%d)", B, S);
  SRLZ_REQUIRE(ws_bytes >= srlz_reward_prior_workspace(S), SRLZ_ERR_WORKSPACE, "reward_prior_bwd: workspace %zu < %zu bytes",
               ws_bytes, srlz_reward_prior_workspace(S));
  const long long n = (long long)B * S;
  SRLZ_LAUNCH(reward_prior_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), states, rewards, ws, g, B, S,
              dstates);
  return 0;
}

extern "C" size_t srlz_episode_prior_workspace(int B, int S) { return (B > 0 && S > 0) ? ep_layout(B, S).total : 0; }

extern "C" int srlz_episode_prior_fwd(const float* states, const int* others, const float* same, int B, int S, const float* w1,
                                      const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                                      float* out, void* ws, size_t ws_bytes, unsigned* ticket, srlz_stream_t stream) {
  SRLZ_REQUIRE(states && others && same && w1 && b1 && w2 && b2 && w3 && b3 && out && ws && ticket, SRLZ_ERR_NULL,
               "episode_prior_fwd: null pointer");
  SRLZ_REQUIRE(B >= 1 && S >= 1 && (long long)B * 2 * S < (1LL << 31), SRLZ_ERR_BAD_DESC, "episode_prior_fwd: bad shape B=%d S=%d",
               B, S);
  const EpLayout L = ep_layout(B, S);
  SRLZ_REQUIRE(ws_bytes >= L.total, SRLZ_ERR_WORKSPACE, "episode_prior_fwd: workspace %zu < %zu bytes", ws_bytes, L.total);
  const int grid = (B + EP_ROWS - 1) / EP_ROWS;
  SRLZ_LAUNCH(episode_prior_fwd_kernel, dim3(grid), dim3(256), 0, as_stream(stream), states, others, same, B, S, w1, b1, w2, b2, w3, b3,
              at<float>(ws, L.h1), at<float>(ws, L.h2), at<float>(ws, L.p), at<double>(ws, L.rowloss), out, ticket);
  return 0;
}

extern "C" int srlz_episode_prior_bwd(const float* states, const int* others, const float* same, const float* g, int B, int S,
                                      const float* w1, const float* w2, const float* w3, void* ws, size_t ws_bytes, float* dstates,
                                      float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3,
                                      srlz_stream_t stream) {
  SRLZ_REQUIRE(states && others && same && g && w1 && w2 && w3 && ws && dstates && dw1 && db1 && dw2 && db2 && dw3 && db3,
               SRLZ_ERR_NULL, "episode_prior_bwd: null pointer");
  SRLZ_REQUIRE(B >= 1 && S >= 1 && (long long)B * 2 * S < (1LL << 31), SRLZ_ERR_BAD_DESC, "episode_prior_bwd: bad shape B=%d S=%d",
               B, S);
  const EpLayout L = ep_layout(B, S);
  SRLZ_REQUIRE(ws_bytes >= L.total, SRLZ_ERR_WORKSPACE, "episode_prior_bwd: workspace %zu < %zu bytes", ws_bytes, L.total);
  SRLZ_LAUNCH(episode_prior_bwd_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), same, g, B, S, w1, w2, w3,
              at<float>(ws, L.h1), at<float>(ws, L.h2), at<float>(ws, L.p), at<float>(ws, L.dz), at<float>(ws, L.dh1), at<float>(ws, L.dh2),
              at<float>(ws, L.dx));
  const int nt = (2 * S + 255) / 256;
  SRLZ_LAUNCH(episode_prior_bwd_reduce_kernel, dim3(B + EP_H * nt + EP_H), dim3(256), 0, as_stream(stream), states, others, B, S,
              at<float>(ws, L.h1), at<float>(ws, L.h2), at<float>(ws, L.dz), at<float>(ws, L.dh1), at<float>(ws, L.dh2),
              at<float>(ws, L.dx), dstates, dw1, db1, dw2, db2, dw3, db3);
  return 0;
}
