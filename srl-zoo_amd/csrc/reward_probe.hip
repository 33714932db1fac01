// reward_probe.hip — the reward-prediction probe of evaluation/predict_reward.py on gfx950, wave64: the classifier
// Linear(2S,4)-ReLU-Linear(4,4)-ReLU-Linear(4,2) on [state ; next_state] (models/forward_inverse.py:78-95), cross-entropy, Adam
// (evaluation/predict_reward.py:106-141).  A minibatch is a few kFLOP, so the reference's loop is launch latency and nothing else;
// here a whole training phase of an epoch is ONE launch (reward_probe_fit_kernel) and a whole validation phase ONE more
// (reward_probe_eval_kernel).
//
// Contract (include/srlz.h).  Row b of a step is states[i .. i+1] with i = idx[step][b]: the two rows are neighbours in memory, so
// the concatenation is the 2S floats at states + i * S and is never written out.
//
// fit: ONE workgroup of 256 threads.  The 4 * 2S + 34 parameters, their Adam moments and the gradient live in LDS from the first
// step to the last (W1 transposed to [k][4], so one 16-byte read gives a column of it).  Per step, per chunk of at most R rows:
//   gather   16 lanes per row copy the 2S floats to LDS
//   layer 1  16 lanes per row: lane kk adds k = kk, kk + 16, ... in that order, then the 16 partial sums are added by a butterfly
//   head     thread = row: layers 2 and 3, the loss, the prediction and the row's backward down to d a1, all in registers -> a record
//   grads    thread = column k of W1 adds the chunk's rows in row order; 34 threads do the same for the small parameters;
//            one wave adds the row losses (fp64) and counts
// then Adam on all parameters (adam_update: the arithmetic of losses.hip).  Every sum over rows has one order, a function of
// (S, B) alone, there are no float atomics, and nothing but (parameters, m, v, statistics) is carried from step to step, all of it
// in the precision it is stored in: n steps in one launch and n launches of one step give the same bits.
//
// eval: 64 rows per workgroup, the same layer 1 straight from global memory and the same head with the row loss in fp64; the
// workgroup's loss goes to ws, its counts to integer atomics (exact in any order), and the workgroup that finishes last (an integer
// ticket, reset by that workgroup) adds the partial losses in workgroup order — the pattern of episode_prior_fwd_kernel.
#include <math.h>

#include "common.h"

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_SMALL = 34;          // b1[4] w2[4][4] b2[4] w3[2][4] b3[2], behind W1 in torch's order
constexpr int RP_MAX_S = 512;         // 4 copies of the parameters + a row chunk must fit in 160 KB of LDS
constexpr int RP_XS_FLOATS = 16384;   // the row chunk: 64 KB
constexpr int RP_MAX_ROWS = 128;      // rows of a chunk (the head runs one thread per row; counts are packed in 16 bits)
constexpr int RP_REC = 20;            // floats of a row record
constexpr int RP_TBL = 256;           // Adam's step scalars are computed for this many steps at a time
constexpr int RP_EV_ROWS = 64;        // rows of an eval workgroup

// offsets in the small block
constexpr int RP_B1 = 0, RP_W2 = 4, RP_B2 = 20, RP_W3 = 24, RP_B3 = 32;
// offsets in a row record: d a1[4], h1[4], d a2[4], h2[4], dz[2], 1.0
constexpr int RP_DA1 = 0, RP_H1 = 4, RP_DA2 = 8, RP_H2 = 12, RP_DZ = 16, RP_ONE = 18;

__host__ __device__ inline int rp_padded(int K) { return 4 * K + 36; }  // 4K + 34 rounded up to whole quads
__host__ __device__ inline int rp_row_stride(int K) { return K | 1; }    // odd: rows of a chunk start in different LDS banks

int rp_chunk_rows(int S) {
  const int r = RP_XS_FLOATS / rp_row_stride(2 * S);
  return r < RP_MAX_ROWS ? r : RP_MAX_ROWS;
}

// element e of the LDS layout ([k][4] of W1, then the small block) -> its place in torch's flat order (W1 [4][K] row-major first)
__device__ __forceinline__ int rp_global_index(int e, int K) { return e < 4 * K ? (e & 3) * K + (e >> 2) : e; }

// torch.optim.Adam, one element: the body of adam_update in losses.hip, so that this path and srlz_adam_step agree
__device__ __forceinline__ void rp_adam_update(float& p, float g, float& m, float& v, float step_size, float b1, float b2, float eps,
                                               float omb1, float omb2, float bc2_sqrt) {
  const float mi = b1 * m + omb1 * g;
  const float vi = b2 * v + omb2 * g * g;
  m = mi; v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p -= step_size * (mi / denom);
}

// 16 lanes of a row: a1[j] = sum_k W1[j][k] x[k], lane kk adds k = kk, kk + 16, ... in order, then a butterfly over the 16 lanes.
// Every lane of the wave calls it (the shuffles need them); an inactive row passes K = 0.
__device__ __forceinline__ f32x4 rp_layer1(const float* __restrict__ ps, const float* __restrict__ x, int K, int kk) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = kk; k < K; k += 16) {
    const f32x4 w = *(const f32x4*)(ps + 4 * k);
    const float xv = x[k];
    acc[0] = fmaf(w[0], xv, acc[0]);
    acc[1] = fmaf(w[1], xv, acc[1]);
    acc[2] = fmaf(w[2], xv, acc[2]);
    acc[3] = fmaf(w[3], xv, acc[3]);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
  }
  return acc;
}

// Layers 2 and 3 of one row from a1 (without its bias) and the small block sp (LDS): h1, h2 and the two logits
__device__ __forceinline__ void rp_head_fwd(const f32x4 a1, const float* __restrict__ sp, float (&h1)[4], float (&h2)[4],
                                            float (&z)[2]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) h1[i] = fmaxf(a1[i] + sp[RP_B1 + i], 0.f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float a = sp[RP_B2 + j];
#pragma unroll
    for (int i = 0; i < 4; ++i) a = fmaf(sp[RP_W2 + j * 4 + i], h1[i], a);
    h2[j] = fmaxf(a, 0.f);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float a = sp[RP_B3 + c];
#pragma unroll
    for (int i = 0; i < 4; ++i) a = fmaf(sp[RP_W3 + c * 4 + i], h2[i], a);
    z[c] = a;
  }
}

// (correct & class 0, correct & class 1, rows of class 0, rows of class 1) of one row, 16 bits each
__device__ __forceinline__ unsigned long long rp_pack_counts(int pred, int label) {
  const unsigned long long ok = pred == label;
  return label ? (ok << 16) | (1ull << 48) : ok | (1ull << 32);
}

__device__ __forceinline__ unsigned long long rp_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(RP_THREADS) void reward_probe_fit_kernel(
    const float* __restrict__ states, const int* __restrict__ labels, int S, const int* __restrict__ idx, int n_steps, int B, int R,
    float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, int t0, double lr, double beta1, double beta2, float eps,
    double* __restrict__ running_loss, long long* __restrict__ counts, double* __restrict__ step_loss) {
  extern __shared__ __attribute__((aligned(16))) float rp_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, kk = tid & 15;
  const int K = 2 * S, P = 4 * K + RP_SMALL, PP = rp_padded(K), KS = rp_row_stride(K);
  float* ps = rp_smem;
  float* ms = ps + PP;
  float* vs = ms + PP;
  float* gs = vs + PP;
  float* xs = gs + PP;                               // [R][KS]
  float* a1s = xs + ((R * KS + 3) & ~3);             // [R][4]
  float* rec = a1s + R * 4;                          // [R][RP_REC]
  float* lossr = rec + R * RP_REC;                   // [R]
  int* flag = (int*)(lossr + R);                     // [R]: prediction | label << 1
  int* labs = flag + R;                              // [R]
  float* tbl = (float*)(labs + R);                   // [RP_TBL][2]: step_size, sqrt(bias correction 2)
  const float* sp = ps + 4 * K;

  for (int e = tid; e < P; e += RP_THREADS) {
    const int g = rp_global_index(e, K);
    ps[e] = params[g];
    ms[e] = m[g];
    vs[e] = v[g];
    gs[e] = 0.f;
  }
  const float b1f = (float)beta1, b2f = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float invB = 1.f / (float)B;
  // the small parameter this thread sums (the top threads: they own the fewest columns of W1), as a product of two record slots
  const int se = RP_THREADS - 1 - tid;
  int sa = RP_ONE, sb = RP_ONE;
  if (se < RP_W2) { sa = RP_DA1 + se; }
  else if (se < RP_B2) { sa = RP_DA2 + ((se - RP_W2) >> 2); sb = RP_H1 + ((se - RP_W2) & 3); }
  else if (se < RP_W3) { sa = RP_DA2 + (se - RP_B2); }
  else if (se < RP_B3) { sa = RP_DZ + ((se - RP_W3) >> 2); sb = RP_H2 + ((se - RP_W3) & 3); }
  else if (se < RP_SMALL) { sa = RP_DZ + (se - RP_B3); }
  // statistics: lane 0 of wave 2
  double run = 0.0;
  long long c0 = 0, c1 = 0, n0 = 0, n1 = 0;
  if (tid == 128) run = running_loss[0];
  __syncthreads();

  for (int sbase = 0; sbase < n_steps; sbase += RP_TBL) {
    {
      // Adam's step scalars of the next RP_TBL steps, one per thread: evaluated in double and rounded once, as srlz_adam_step does
      // on the host; a function of t0 + step alone.  (The previous block's last read of tbl lies before that step's last barrier.)
      const double t = (double)t0 + (double)(sbase + tid) + 1.0;
      tbl[2 * tid] = (float)(lr / (1.0 - pow(beta1, t)));
      tbl[2 * tid + 1] = (float)sqrt(1.0 - pow(beta2, t));
    }
    const int send = min(n_steps, sbase + RP_TBL);
  for (int step = sbase; step < send; ++step) {
    double sl = 0.0;
    for (int r0 = 0; r0 < B; r0 += R) {
      const int rows = min(R, B - r0);
      const int* __restrict__ irow = idx + (size_t)step * B + r0;
      for (int rr = grp; rr < rows; rr += 16) {
        const int i = irow[rr];
        const float* __restrict__ src = states + (size_t)i * S;
        float* dst = xs + rr * KS;
#pragma unroll 4
        for (int k = kk; k < K; k += 16) dst[k] = src[k];
        if (kk == 0) labs[rr] = labels[i];
      }
      __syncthreads();
      for (int rb = 0; rb < rows; rb += 16) {
        const int rr = rb + grp;
        const bool on = rr < rows;
        const f32x4 a1 = rp_layer1(ps, xs + (on ? rr : 0) * KS, on ? K : 0, kk);
        if (on && kk == 0) *(f32x4*)(a1s + rr * 4) = a1;
      }
      __syncthreads();
      if (tid < rows) {
        float h1[4], h2[4], z[2];
        rp_head_fwd(*(const f32x4*)(a1s + tid * 4), sp, h1, h2, z);
        const int label = labs[tid] == 1;
        const int pred = z[1] > z[0];  // a tie goes to class 0, as th.max does
        // two classes: with d = z1 - z0 the loss is softplus(-d) for class 1 and softplus(d) for class 0 (the log-sum-exp form),
        // softmax = (1, e) / (1 + e) with e = exp(-|d|); d loss / d z1 = p1 - label, written without the cancellation at p1 -> 1
        const float d = z[1] - z[0];
        const float e = expf(-fabsf(d));
        const float inv = 1.f / (1.f + e);
        const float p1 = d >= 0.f ? inv : e * inv, p0 = d >= 0.f ? e * inv : inv;
        const float s = label ? -d : d;
        lossr[tid] = fmaxf(s, 0.f) + log1pf(e);
        flag[tid] = pred | (label << 1);
        float dz[2];
        dz[1] = (label ? -p0 : p1) * invB;
        dz[0] = -dz[1];
        float da2[4], da1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dh = fmaf(sp[RP_W3 + 4 + i], dz[1], sp[RP_W3 + i] * dz[0]);
          da2[i] = h2[i] > 0.f ? dh : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float dh = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) dh = fmaf(sp[RP_W2 + j * 4 + i], da2[j], dh);
          da1[i] = h1[i] > 0.f ? dh : 0.f;
        }
        float* r = rec + tid * RP_REC;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          r[RP_DA1 + i] = da1[i];
          r[RP_H1 + i] = h1[i];
          r[RP_DA2 + i] = da2[i];
          r[RP_H2 + i] = h2[i];
        }
        r[RP_DZ] = dz[0];
        r[RP_DZ + 1] = dz[1];
        r[RP_ONE] = 1.f;
      }
      __syncthreads();
      // gradients: rows in row order, chunk after chunk
      for (int k = tid; k < K; k += RP_THREADS) {
        f32x4 g = *(const f32x4*)(gs + 4 * k);
        for (int rr = 0; rr < rows; ++rr) {
          const f32x4 dd = *(const f32x4*)(rec + rr * RP_REC + RP_DA1);
          const float xv = xs[rr * KS + k];
          g[0] = fmaf(dd[0], xv, g[0]);
          g[1] = fmaf(dd[1], xv, g[1]);
          g[2] = fmaf(dd[2], xv, g[2]);
          g[3] = fmaf(dd[3], xv, g[3]);
        }
        *(f32x4*)(gs + 4 * k) = g;
      }
      if (se < RP_SMALL) {
        float g = gs[4 * K + se];
        for (int rr = 0; rr < rows; ++rr) g = fmaf(rec[rr * RP_REC + sa], rec[rr * RP_REC + sb], g);
        gs[4 * K + se] = g;
      }
      if (wave == 2) {
        double l = 0.0;
        unsigned long long pk = 0;
        for (int rr = lane; rr < rows; rr += 64) {
          l += (double)lossr[rr];
          pk += rp_pack_counts(flag[rr] & 1, flag[rr] >> 1);
        }
        l = wave_sum_d(l);
        pk = rp_wave_sum_u64(pk);
        sl += l;
        c0 += (long long)(pk & 0xffff);
        c1 += (long long)((pk >> 16) & 0xffff);
        n0 += (long long)((pk >> 32) & 0xffff);
        n1 += (long long)(pk >> 48);
      }
      __syncthreads();
    }
    const float step_size = tbl[2 * (step & (RP_TBL - 1))], bc2_sqrt = tbl[2 * (step & (RP_TBL - 1)) + 1];
    for (int e = tid; e < P; e += RP_THREADS) {
      rp_adam_update(ps[e], gs[e], ms[e], vs[e], step_size, b1f, b2f, eps, omb1, omb2, bc2_sqrt);
      gs[e] = 0.f;
    }
    if (tid == 128) {
      const double mean = sl / (double)B;  // the reference: running_loss += loss.item() * inputs.size(0)
      run += mean * (double)B;
      if (step_loss) step_loss[step] = mean;
    }
    __syncthreads();
  }
  }

  for (int e = tid; e < P; e += RP_THREADS) {
    const int g = rp_global_index(e, K);
    params[g] = ps[e];
    m[g] = ms[e];
    v[g] = vs[e];
  }
  if (tid == 128) {
    running_loss[0] = run;
    counts[0] += c0 + c1;
    counts[1] += c0;
    counts[2] += c1;
    counts[3] += n0;
    counts[4] += n1;
  }
}

__global__ __launch_bounds__(RP_THREADS) void reward_probe_eval_kernel(
    const float* __restrict__ states, const int* __restrict__ labels, int S, const int* __restrict__ idx, int total,
    const float* __restrict__ params, double* __restrict__ partial, double* __restrict__ running_loss,
    unsigned long long* __restrict__ counts, unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float rp_smem[];
  __shared__ __attribute__((aligned(16))) float a1s[RP_EV_ROWS * 4];
  __shared__ int labs[RP_EV_ROWS];
  __shared__ double slots[4];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, kk = tid & 15;
  const int K = 2 * S, P = 4 * K + RP_SMALL;
  float* ps = rp_smem;
  const float* sp = ps + 4 * K;
  for (int e = tid; e < P; e += RP_THREADS) ps[e] = params[rp_global_index(e, K)];
  __syncthreads();
  const int row0 = blockIdx.x * RP_EV_ROWS, rows = min(RP_EV_ROWS, total - row0);
#pragma unroll
  for (int rb = 0; rb < RP_EV_ROWS; rb += 16) {
    const int rr = rb + grp;
    const bool on = rr < rows;
    const int i = on ? idx[row0 + rr] : 0;
    const f32x4 a1 = rp_layer1(ps, states + (size_t)i * S, on ? K : 0, kk);
    if (on && kk == 0) {
      *(f32x4*)(a1s + rr * 4) = a1;
      labs[rr] = labels[i];
    }
  }
  __syncthreads();
  if (wave == 0) {
    double l = 0.0;
    unsigned long long pk = 0;
    if (lane < rows) {
      float h1[4], h2[4], z[2];
      rp_head_fwd(*(const f32x4*)(a1s + lane * 4), sp, h1, h2, z);
      const int label = labs[lane] == 1;
      const double z0 = (double)z[0], z1 = (double)z[1], mx = fmax(z0, z1);
      l = mx + log(exp(z0 - mx) + exp(z1 - mx)) - (label ? z1 : z0);
      pk = rp_pack_counts(z[1] > z[0], label);
    }
    l = wave_sum_d(l);
    pk = rp_wave_sum_u64(pk);
    if (lane == 0) partial[blockIdx.x] = l;
    const unsigned long long f0 = pk & 0xffff, f1 = (pk >> 16) & 0xffff, f2 = (pk >> 32) & 0xffff, f3 = pk >> 48;
    // integers: exact in any order
    if (lane < 5) atomicAdd(counts + lane, lane == 0 ? f0 + f1 : lane == 1 ? f0 : lane == 2 ? f1 : lane == 3 ? f2 : f3);
  }
  // the last workgroup to finish adds the partial losses, in workgroup order
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  double t = 0.0;
  for (int w = tid; w < (int)gridDim.x; w += RP_THREADS) t += partial[w];
  t = wave_sum_d(t);
  if (lane == 0) slots[wave] = t;
  __syncthreads();
  if (tid == 0) {
    running_loss[0] += ((slots[0] + slots[1]) + slots[2]) + slots[3];
    atomicExch(ticket, 0u);
  }
}

size_t rp_fit_lds_bytes(int S, int R) {
  const int K = 2 * S;
  return sizeof(float) * ((size_t)4 * rp_padded(K) + ((R * rp_row_stride(K) + 3) & ~3) + (size_t)R * (4 + RP_REC + 3) + 2 * RP_TBL);
}

// the checks both entry points share; `who` names the entry point in the error text
int rp_check(const char* who, const void* states, const void* labels, int N, int S, const void* idx, const int* idx_host, long long n,
             int B, const void* params) {
  SRLZ_REQUIRE(states && labels && idx && idx_host && params, SRLZ_ERR_NULL, "%s: null pointer", who);
  SRLZ_REQUIRE(N >= 2, SRLZ_ERR_BAD_DESC, "%s: needs N >= 2 rows of states (N=%d)", who, N);
  SRLZ_REQUIRE(S >= 1 && S <= RP_MAX_S, SRLZ_ERR_BAD_DESC,
               "%s: the state dimension must lie in [1, %d] (S=%d): the parameters and their Adam moments stay in LDS", who, RP_MAX_S, S);
  SRLZ_REQUIRE(n >= 1 && B >= 1 && n * (long long)B < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "%s: needs at least one minibatch of at least one row and fewer than 2^31 rows in all (%lld x %d)", who, n, B);
  const long long rows = n * (long long)B;
  for (long long q = 0; q < rows; ++q)
    SRLZ_REQUIRE(idx_host[q] >= 0 && idx_host[q] <= N - 2, SRLZ_ERR_BAD_DESC,
                 "%s: index %d at position %lld lies outside [0, N - 2] (N=%d): row i is read together with row i + 1", who,
                 idx_host[q], q, N);
  return 0;
}

}  // namespace

extern "C" int srlz_reward_probe_chunk_rows(int S) { return (S >= 1 && S <= RP_MAX_S) ? rp_chunk_rows(S) : 0; }

extern "C" int srlz_reward_probe_fit(const float* states, const int* labels, int N, int S, const int* idx, const int* idx_host,
                                     int n_steps, int B, float* params, float* m, float* v, int t0, double lr, double beta1,
                                     double beta2, double eps, double* running_loss, long long* counts, double* step_loss,
                                     srlz_stream_t stream) {
  const int rc = rp_check("reward_probe_fit", states, labels, N, S, idx, idx_host, n_steps, B, params);
  if (rc) return rc;
  SRLZ_REQUIRE(m && v && running_loss && counts, SRLZ_ERR_NULL, "reward_probe_fit: null pointer");
  SRLZ_REQUIRE(t0 >= 0 && (long long)t0 + n_steps < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "reward_probe_fit: t0 counts the Adam steps already taken (t0=%d, n_steps=%d)", t0, n_steps);
  const int R = rp_chunk_rows(S) < B ? rp_chunk_rows(S) : B;
  const size_t lds = rp_fit_lds_bytes(S, R);
  SRLZ_MAX_LDS(reward_probe_fit_kernel, lds);
  SRLZ_LAUNCH(reward_probe_fit_kernel, dim3(1), dim3(RP_THREADS), lds, as_stream(stream), states, labels, S, idx, n_steps, B, R, params,
              m, v, t0, lr, beta1, beta2, (float)eps, running_loss, counts, step_loss);
  return 0;
}

extern "C" size_t srlz_reward_probe_eval_workspace(int n_batches, int B) {
  if (n_batches < 1 || B < 1 || (long long)n_batches * B >= (1LL << 31)) return 0;
  const long long rows = (long long)n_batches * B;
  return (size_t)((rows + RP_EV_ROWS - 1) / RP_EV_ROWS) * sizeof(double);
}

extern "C" int srlz_reward_probe_eval(const float* states, const int* labels, int N, int S, const int* idx, const int* idx_host,
                                      int n_batches, int B, const float* params, double* running_loss, long long* counts, void* ws,
                                      size_t ws_bytes, unsigned* ticket, srlz_stream_t stream) {
  const int rc = rp_check("reward_probe_eval", states, labels, N, S, idx, idx_host, n_batches, B, params);
  if (rc) return rc;
  SRLZ_REQUIRE(running_loss && counts && ws && ticket, SRLZ_ERR_NULL, "reward_probe_eval: null pointer");
  const size_t need = srlz_reward_probe_eval_workspace(n_batches, B);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "reward_probe_eval: workspace %zu < %zu bytes", ws_bytes, need);
  const int total = n_batches * B;
  const unsigned wgs = (unsigned)((total + RP_EV_ROWS - 1) / RP_EV_ROWS);
  SRLZ_LAUNCH(reward_probe_eval_kernel, dim3(wgs), dim3(RP_THREADS), sizeof(float) * rp_padded(2 * S), as_stream(stream), states,
              labels, S, idx, total, params, (double*)ws, running_loss, (unsigned long long*)counts, ticket);
  return 0;
}
