// invfit.hip — the inverse head of the deployment objects, trained on a recording (srlz/invfit.py, LatentDynamics.refit_inverse):
// the classifier Linear(2S, A) on [state ; next_state] (models/forward_inverse.py inverseModel, --inverse-model-type linear) under
// the cross-entropy of losses/losses.py:117-129, Adam as the learner's loop runs it.  Multinomial logistic regression; the shape of
// headfit.hip: a minibatch is a few kFLOP, so an epoch of minibatches is ONE launch (invfit_fit_kernel) and a validation phase ONE
// more (invfit_eval_kernel).  The small helpers both files need (the Adam element, the 16-lane quad) are restated here and not moved
// into a header: headfit.hip's tests pin its bits, and its translation unit stays as it is.
//
// Contract (include/srlz.h).  Row b of a step is states[i .. i+1] with i = idx[step][b] clamped to [0, N - 2]: the concatenation is
// the 2S floats at states + i * S and is never written out; its label is labels[i].  With K = 2S, AP = A rounded up to a multiple
// of 4 and APAD = AP | 4 (a multiple of 4 that is 4 mod 8, so a stride of APAD floats meets only 4 of the LDS banks' 4-word groups):
//
// fit: ONE workgroup of 256 threads.  Parameters and gradient live in LDS from the first step to the last as [K + 1][APAD] (row k < K
// is W[:, k], row K the bias; one 16-byte read gives four outputs of a column; the entries beyond A are zero and stay zero), the Adam
// moments stay in global memory in state_dict order (each is read and written once per step, coalesced; two more copies in LDS would
// halve the envelope).  Per step, per chunk of at most R rows, with a barrier after each stage:
//   gather   16 lanes per row copy the 2S floats to LDS
//   logits   16 lanes per row and quad of outputs: lane kk adds k = kk, kk + 16, ... in that order, the 16 partial sums are added
//            by a butterfly; + bias -> z in the row's record
//   softmax  thread = row: max and argmax (j ascending, a tie to the lowest class), e_j = exp(z_j - max), the sum of the e_j beside
//            the label's (j ascending) + the label's; loss; dz_j = e_j / sum / B, the label's -(sum of the others) / sum / B, which
//            has no cancellation at p -> 1; a label outside [0, A): loss 0, dz 0, counted in `bad`
//   grads    thread = (row k of the image, quad of outputs): rows in row order, chunk after chunk (the bias row multiplies by 1);
//            one wave adds the row losses (fp64) and the counts
// then Adam on every parameter (the arithmetic of losses.hip adam_update).  Every sum has one order, a function of (S, A, B) alone;
// no float atomics (the per-action counters are integer atomics in LDS, exact in any order); nothing but (parameters, m, v,
// statistics) is carried from step to step, all in the precision it is stored in: n steps in one launch and n launches of one step
// give the same bits.
//
// eval: 64 rows per workgroup, 16 at a time: the same logits straight from global memory, the row loss in fp64 (log-sum-exp, j
// ascending); the workgroup's loss goes to ws, its counts to integer atomics (exact in any order), and the workgroup that finishes
// last (an integer ticket, reset by that workgroup) adds the partial losses in workgroup order — the pattern of headfit_eval_kernel.
#include <math.h>

#include "common.h"

namespace {

constexpr int IF_THREADS = 256;
constexpr int IF_LDS_BYTES = 160 * 1024;
constexpr int IF_MAX_ROWS = 128;         // rows of a chunk (the softmax stage runs one thread per row)
constexpr int IF_MIN_ROWS = 16;          // a shape whose chunk would be shorter is refused
constexpr int IF_TBL = 256;              // Adam's step scalars are computed for this many steps at a time
constexpr int IF_EV_ROWS = 64;           // rows of an eval workgroup
constexpr int IF_EV_PASS = 16;           // of which this many are in LDS at a time (one per group of 16 lanes)

struct IfLayout {
  int K, A, AP, APAD, Q;                 // Q: quads of outputs
  int PL, KS;                            // floats of the LDS image (a multiple of 4); stride of a gathered row
};

__host__ __device__ inline IfLayout if_layout(int S, int A) {
  IfLayout L;
  L.K = 2 * S; L.A = A; L.AP = (A + 3) & ~3; L.APAD = L.AP | 4; L.Q = L.AP >> 2;
  L.PL = (L.K + 1) * L.APAD;
  L.KS = L.K | 1;                        // odd: rows of a chunk start in different LDS banks
  return L;
}

// rows of a chunk: as many as fit beside the parameters, the gradient, the per-action counters (2 * APAD) and Adam's table, at
// most IF_MAX_ROWS; 0 where fewer than IF_MIN_ROWS fit, S < 1 or A < 2.  This IS the predicate srlz_invfit_supported:
//   min(128, floor((40444 - 2 * (K + 2) * APAD) / ((K | 1) + APAD + 3)))
// (a row costs itself, its record z / dz [APAD], loss, flag and label; 4 floats are kept back for the rounding of the rows' block).
int if_chunk_rows(int S, int A) {
  if (S < 1 || A < 2 || S > IF_LDS_BYTES || A > IF_LDS_BYTES) return 0;  // (the upper ends: far beyond the budget, before 2S wraps)
  const long long K = 2LL * S, APAD = ((A + 3) & ~3) | 4;
  const long long room = IF_LDS_BYTES / 4 - 4 - 2 * (K + 2) * APAD - 2 * IF_TBL;
  if (room < 0) return 0;
  const long long r = room / ((K | 1) + APAD + 3);
  if (r < IF_MIN_ROWS) return 0;
  return (int)(r < IF_MAX_ROWS ? r : IF_MAX_ROWS);
}

size_t if_fit_lds_bytes(const IfLayout& L, int R) {
  return sizeof(float) * (size_t)(2 * L.PL + 2 * L.APAD + 2 * IF_TBL + ((R * L.KS + 3) & ~3) + R * (L.APAD + 3));
}

size_t if_eval_lds_bytes(const IfLayout& L) { return sizeof(float) * (size_t)(L.PL + IF_EV_PASS * L.APAD); }

// parameters in state_dict order (weight [A, K], bias [A]) -> the LDS image (pads zeroed)
__device__ __forceinline__ void if_load_params(float* __restrict__ ps, const float* __restrict__ params, const IfLayout& L, int tid) {
  for (int e = tid; e < L.PL; e += IF_THREADS) ps[e] = 0.f;
  __syncthreads();
  for (int g = tid; g < L.K * L.A; g += IF_THREADS) {
    const int j = g / L.K, k = g - j * L.K;
    ps[k * L.APAD + j] = params[g];
  }
  for (int j = tid; j < L.A; j += IF_THREADS) ps[L.K * L.APAD + j] = params[L.K * L.A + j];
}

// torch.optim.Adam, one element: the body of adam_update in losses.hip and of hf_adam_update, so that the paths agree
__device__ __forceinline__ void if_adam_update(float& p, float g, float& m, float& v, float step_size, float b1, float b2, float eps,
                                               float omb1, float omb2, float bc2_sqrt) {
  const float mi = b1 * m + omb1 * g;
  const float vi = b2 * v + omb2 * g * g;
  m = mi; v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p -= step_size * (mi / denom);
}

// 16 lanes of a row, four outputs: a[j] = sum_k W[k][j] x[k], lane kk adds k = kk, kk + 16, ... in order, then a butterfly over the
// 16 lanes.  w points at the quad in row 0.  Every lane of the wave calls it (the shuffles need them); an inactive row passes K = 0.
__device__ __forceinline__ f32x4 if_quad(const float* __restrict__ w, int APAD, const float* __restrict__ x, int K, int kk) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = kk; k < K; k += 16) {
    const f32x4 wv = *(const f32x4*)(w + k * APAD);
    const float xv = x[k];
    acc[0] = fmaf(wv[0], xv, acc[0]);
    acc[1] = fmaf(wv[1], xv, acc[1]);
    acc[2] = fmaf(wv[2], xv, acc[2]);
    acc[3] = fmaf(wv[3], xv, acc[3]);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
  }
  return acc;
}

// the logits of the rows rb .. rb + 15 (group grp of 16 lanes = row rb + grp): z = W x + b into rec[slot(row)][APAD].  x_of(row)
// gives the row's 2S floats.  Every thread of the block calls it.
template <class XOf>
__device__ __forceinline__ void if_logits_rows(const float* __restrict__ ps, float* __restrict__ rec, const IfLayout& L, int rb, int rows,
                                               int slot0, int grp, int kk, XOf x_of) {
  const int rr = rb + grp;
  const bool on = rr < rows;
  const float* __restrict__ x = x_of(on ? rr : 0);
  const int Kon = on ? L.K : 0;
  for (int q = 0; q < L.AP; q += 4) {
    const f32x4 a = if_quad(ps + q, L.APAD, x, Kon, kk);
    if (on && kk == 0) {
      const f32x4 b = *(const f32x4*)(ps + L.K * L.APAD + q);
      *(f32x4*)(rec + (slot0 + grp) * L.APAD + q) = a + b;
    }
  }
}

__device__ __forceinline__ int if_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int if_clamp_index(int i, int N) { return min(max(i, 0), N - 2); }

// flag of a row: 1 predicted right, 0 wrong, 2 a label outside [0, A)
constexpr int IF_BAD = 2;

__global__ __launch_bounds__(IF_THREADS) void invfit_fit_kernel(
    const float* __restrict__ states, const int* __restrict__ labels, int N, int S, int A, const int* __restrict__ idx, int n_steps, int B,
    int R, float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, int t0, double lr, double beta1, double beta2,
    float eps, double* __restrict__ running_loss, long long* __restrict__ counts, double* __restrict__ step_loss,
    float* __restrict__ last_grad) {
  extern __shared__ __attribute__((aligned(16))) float if_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, kk = tid & 15;
  const IfLayout L = if_layout(S, A);
  const int K = L.K, KS = L.KS, APAD = L.APAD, Q = L.Q;
  float* ps = if_smem;
  float* gs = ps + L.PL;
  int* cnt = (int*)(gs + L.PL);                       // support[APAD], hits[APAD]
  float* tbl = (float*)(cnt + 2 * APAD);              // [IF_TBL][2]: step_size, sqrt(bias correction 2)
  float* xs = tbl + 2 * IF_TBL;                       // [R][KS]
  float* rec = xs + ((R * KS + 3) & ~3);              // [R][APAD]: z, then dz
  float* lossr = rec + R * APAD;                      // [R]
  int* flag = (int*)(lossr + R);                      // [R]
  int* labs = flag + R;                               // [R]

  if_load_params(ps, params, L, tid);
  for (int e = tid; e < L.PL; e += IF_THREADS) gs[e] = 0.f;
  for (int e = tid; e < 2 * APAD; e += IF_THREADS) cnt[e] = 0;
  const float b1f = (float)beta1, b2f = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float invB = 1.f / (float)B;
  const int nW = (K + 1) * Q, nP = K * A;
  // statistics: lane 0 of wave 2
  double run = 0.0;
  long long c_rows = 0, c_ok = 0, c_bad = 0;
  if (tid == 128) run = running_loss[0];
  __syncthreads();

  for (int sbase = 0; sbase < n_steps; sbase += IF_TBL) {
    {
      // Adam's step scalars of the next IF_TBL steps, one per thread: evaluated in double and rounded once, as srlz_adam_step does
      // on the host; a function of t0 + step alone.  (The previous block's last read of tbl lies before that step's last barrier.)
      const double t = (double)t0 + (double)(sbase + tid) + 1.0;
      tbl[2 * tid] = (float)(lr / (1.0 - pow(beta1, t)));
      tbl[2 * tid + 1] = (float)sqrt(1.0 - pow(beta2, t));
    }
    const int send = min(n_steps, sbase + IF_TBL);
    for (int step = sbase; step < send; ++step) {
      double sl = 0.0;
      for (int r0 = 0; r0 < B; r0 += R) {
        const int rows = min(R, B - r0);
        const int* __restrict__ irow = idx + (size_t)step * B + r0;
        for (int rr = grp; rr < rows; rr += 16) {
          const int i = if_clamp_index(irow[rr], N);
          const float* __restrict__ src = states + (size_t)i * S;
          float* dst = xs + rr * KS;
#pragma unroll 4
          for (int k = kk; k < K; k += 16) dst[k] = src[k];
          if (kk == 0) labs[rr] = labels[i];
        }
        __syncthreads();
        for (int rb = 0; rb < rows; rb += 16)
          if_logits_rows(ps, rec, L, rb, rows, rb, grp, kk, [&](int rr) { return (const float*)(xs + rr * KS); });
        __syncthreads();
        if (tid < rows) {
          float* z = rec + tid * APAD;
          const int label = labs[tid];
          const bool good = (unsigned)label < (unsigned)A;  // nothing is indexed by a label that fails this
          float mx = z[0];
          int pred = 0;
          for (int j = 1; j < A; ++j)
            if (z[j] > mx) { mx = z[j]; pred = j; }  // strictly greater: a tie goes to the lowest class, as th.max does
          float loss = 0.f;
          if (good) {
            const float zl = z[label];
            float other = 0.f;
            for (int j = 0; j < A; ++j) {
              const float e = expf(z[j] - mx);
              z[j] = e;
              if (j != label) other += e;
            }
            const float total = other + z[label];
            // the label at the maximum: e = 1 and the loss is log(1 + others), exact where the others vanish
            loss = zl == mx ? log1pf(other) : logf(total) - (zl - mx);
            const float inv = invB / total;
            for (int j = 0; j < A; ++j) z[j] *= inv;
            z[label] = -other * inv;
            atomicAdd(cnt + label, 1);
            if (pred == label) atomicAdd(cnt + APAD + label, 1);
          } else {
            for (int j = 0; j < A; ++j) z[j] = 0.f;
          }
          lossr[tid] = loss;
          flag[tid] = good ? (pred == label) : IF_BAD;
        }
        __syncthreads();
        // gradients: rows in row order, chunk after chunk; row K of the image is the bias, whose input is 1
        for (int w = tid; w < nW; w += IF_THREADS) {
          const int q = w / (K + 1), k = w - q * (K + 1);
          float* gp = gs + k * APAD + 4 * q;
          f32x4 g = *(const f32x4*)gp;
          if (k < K) {
            for (int rr = 0; rr < rows; ++rr) {
              const f32x4 dd = *(const f32x4*)(rec + rr * APAD + 4 * q);
              const float xv = xs[rr * KS + k];
              g[0] = fmaf(dd[0], xv, g[0]);
              g[1] = fmaf(dd[1], xv, g[1]);
              g[2] = fmaf(dd[2], xv, g[2]);
              g[3] = fmaf(dd[3], xv, g[3]);
            }
          } else {
            for (int rr = 0; rr < rows; ++rr) g += *(const f32x4*)(rec + rr * APAD + 4 * q);
          }
          *(f32x4*)gp = g;
        }
        if (wave == 2) {
          double l = 0.0;
          int ok = 0, bad = 0;
          for (int rr = lane; rr < rows; rr += 64) {
            l += (double)lossr[rr];
            ok += flag[rr] == 1;
            bad += flag[rr] == IF_BAD;
          }
          l = wave_sum_d(l);
          sl += l;
          c_rows += rows;
          c_ok += if_wave_sum_i(ok);
          c_bad += if_wave_sum_i(bad);
        }
        __syncthreads();
      }
      const float step_size = tbl[2 * (step & (IF_TBL - 1))], bc2_sqrt = tbl[2 * (step & (IF_TBL - 1)) + 1];
      float* __restrict__ lg = (last_grad && step == n_steps - 1) ? last_grad : nullptr;
      for (int g = tid; g < nP + A; g += IF_THREADS) {
        int e;
        if (g < nP) {
          const int j = g / K;
          e = (g - j * K) * APAD + j;
        } else {
          e = K * APAD + (g - nP);
        }
        float mi = m[g], vi = v[g];
        const float gv = gs[e];
        if_adam_update(ps[e], gv, mi, vi, step_size, b1f, b2f, eps, omb1, omb2, bc2_sqrt);
        m[g] = mi; v[g] = vi;
        gs[e] = 0.f;
        if (lg) lg[g] = gv;
      }
      if (tid == 128) {
        const double mean = sl / (double)B;  // the reference: running_loss += loss.item() * inputs.size(0)
        run += mean * (double)B;
        if (step_loss) step_loss[step] = mean;
      }
      __syncthreads();
    }
  }

  for (int g = tid; g < nP; g += IF_THREADS) {
    const int j = g / K;
    params[g] = ps[(g - j * K) * APAD + j];
  }
  for (int j = tid; j < A; j += IF_THREADS) {
    params[nP + j] = ps[K * APAD + j];
    counts[3 + j] += cnt[j];
    counts[3 + A + j] += cnt[APAD + j];
  }
  if (tid == 128) {
    running_loss[0] = run;
    counts[0] += c_rows;
    counts[1] += c_ok;
    counts[2] += c_bad;
  }
}

__global__ __launch_bounds__(IF_THREADS) void invfit_eval_kernel(
    const float* __restrict__ states, const int* __restrict__ labels, int N, int S, int A, const int* __restrict__ idx, int total,
    const float* __restrict__ params, double* __restrict__ partial, double* __restrict__ running_loss,
    unsigned long long* __restrict__ counts, unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float if_smem[];
  __shared__ double lossd[IF_EV_ROWS];
  __shared__ int flag[IF_EV_ROWS];
  __shared__ double slots[4];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, kk = tid & 15;
  const IfLayout L = if_layout(S, A);
  float* ps = if_smem;
  float* rec = ps + L.PL;                             // [IF_EV_PASS][APAD]
  if_load_params(ps, params, L, tid);
  const int row0 = blockIdx.x * IF_EV_ROWS, rows = min(IF_EV_ROWS, total - row0);
  __syncthreads();
  for (int rb = 0; rb < rows; rb += IF_EV_PASS) {
    if_logits_rows(ps, rec, L, rb, rows, 0, grp, kk,
                   [&](int rr) { return states + (size_t)if_clamp_index(idx[row0 + rr], N) * S; });
    __syncthreads();
    if (tid < IF_EV_PASS && rb + tid < rows) {
      const float* z = rec + tid * L.APAD;
      const int label = labels[if_clamp_index(idx[row0 + rb + tid], N)];
      const bool good = (unsigned)label < (unsigned)A;
      float mx = z[0];
      int pred = 0;
      for (int j = 1; j < A; ++j)
        if (z[j] > mx) { mx = z[j]; pred = j; }
      double l = 0.0;
      if (good) {
        double sum = 0.0;
        for (int j = 0; j < A; ++j) sum += exp((double)z[j] - (double)mx);
        l = (double)mx + log(sum) - (double)z[label];
        // integers: exact in any order
        atomicAdd(counts + 3 + label, 1ull);
        if (pred == label) atomicAdd(counts + 3 + A + label, 1ull);
      }
      lossd[rb + tid] = l;
      flag[rb + tid] = good ? (pred == label) : IF_BAD;
    }
    __syncthreads();
  }
  if (wave == 0) {
    double l = 0.0;
    int ok = 0, bad = 0;
    if (lane < rows) {
      l = lossd[lane];
      ok = flag[lane] == 1;
      bad = flag[lane] == IF_BAD;
    }
    l = wave_sum_d(l);
    ok = if_wave_sum_i(ok);
    bad = if_wave_sum_i(bad);
    if (lane == 0) partial[blockIdx.x] = l;
    if (lane < 3) atomicAdd(counts + lane, (unsigned long long)(lane == 0 ? rows : lane == 1 ? ok : bad));
  }
  // the last workgroup to finish adds the partial losses, in workgroup order
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  double t = 0.0;
  for (int w = tid; w < (int)gridDim.x; w += IF_THREADS) t += partial[w];
  t = wave_sum_d(t);
  if (lane == 0) slots[wave] = t;
  __syncthreads();
  if (tid == 0) {
    running_loss[0] += ((slots[0] + slots[1]) + slots[2]) + slots[3];
    atomicExch(ticket, 0u);
  }
}

// the checks both entry points share; `who` names the entry point in the error text
int if_check(const char* who, const void* states, const void* labels, int N, int S, int A, const void* idx, const int* idx_host,
             long long n, int B, const void* params) {
  SRLZ_REQUIRE(states && labels && idx && idx_host && params, SRLZ_ERR_NULL, "%s: null pointer", who);
  SRLZ_REQUIRE(if_chunk_rows(S, A) > 0, SRLZ_ERR_BAD_DESC,
               "%s: state dimension %d with %d actions is outside srlz_invfit_supported: S >= 1, A >= 2, and the parameters, the "
               "gradient and a chunk of %d rows must fit in %d bytes of LDS",
               who, S, A, IF_MIN_ROWS, IF_LDS_BYTES);
  SRLZ_REQUIRE(N >= 2 && (long long)N * S < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "%s: needs N >= 2 rows of states and N * S < 2^31 (N=%d, S=%d)", who, N, S);
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

extern "C" int srlz_invfit_chunk_rows(int S, int A) { return if_chunk_rows(S, A); }

extern "C" int srlz_invfit_supported(int S, int A) { return if_chunk_rows(S, A) > 0; }

extern "C" long long srlz_invfit_n_params(int S, int A) {
  if (S < 1 || A < 2) return 0;
  return 2LL * S * A + A;
}

extern "C" int srlz_invfit_fit(const float* states, const int* labels, int N, int S, int A, const int* idx, const int* idx_host,
                               int n_steps, int B, float* params, float* m, float* v, int t0, double lr, double beta1, double beta2,
                               double eps, double* running_loss, long long* counts, double* step_loss, float* last_grad,
                               srlz_stream_t stream) {
  const int rc = if_check("invfit_fit", states, labels, N, S, A, idx, idx_host, n_steps, B, params);
  if (rc) return rc;
  SRLZ_REQUIRE(m && v && running_loss && counts, SRLZ_ERR_NULL, "invfit_fit: null pointer");
  SRLZ_REQUIRE(t0 >= 0 && (long long)t0 + n_steps < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "invfit_fit: t0 counts the Adam steps already taken (t0=%d, n_steps=%d)", t0, n_steps);
  const IfLayout L = if_layout(S, A);
  const int R = if_chunk_rows(S, A) < B ? if_chunk_rows(S, A) : B;
  const size_t lds = if_fit_lds_bytes(L, R);
  SRLZ_MAX_LDS(invfit_fit_kernel, lds);
  SRLZ_LAUNCH(invfit_fit_kernel, dim3(1), dim3(IF_THREADS), lds, as_stream(stream), states, labels, N, S, A, idx, n_steps, B, R, params,
              m, v, t0, lr, beta1, beta2, (float)eps, running_loss, counts, step_loss, last_grad);
  return 0;
}

extern "C" size_t srlz_invfit_eval_workspace(int n_batches, int B) {
  if (n_batches < 1 || B < 1 || (long long)n_batches * B >= (1LL << 31)) return 0;
  const long long rows = (long long)n_batches * B;
  return (size_t)((rows + IF_EV_ROWS - 1) / IF_EV_ROWS) * sizeof(double);
}

extern "C" int srlz_invfit_eval(const float* states, const int* labels, int N, int S, int A, const int* idx, const int* idx_host,
                                int n_batches, int B, const float* params, double* running_loss, long long* counts, void* ws,
                                size_t ws_bytes, unsigned* ticket, srlz_stream_t stream) {
  const int rc = if_check("invfit_eval", states, labels, N, S, A, idx, idx_host, n_batches, B, params);
  if (rc) return rc;
  SRLZ_REQUIRE(running_loss && counts && ws && ticket, SRLZ_ERR_NULL, "invfit_eval: null pointer");
  const size_t need = srlz_invfit_eval_workspace(n_batches, B);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "invfit_eval: workspace %zu < %zu bytes", ws_bytes, need);
  const IfLayout L = if_layout(S, A);
  const int total = n_batches * B;
  const unsigned wgs = (unsigned)((total + IF_EV_ROWS - 1) / IF_EV_ROWS);
  const size_t lds = if_eval_lds_bytes(L);
  SRLZ_MAX_LDS(invfit_eval_kernel, lds);
  SRLZ_LAUNCH(invfit_eval_kernel, dim3(wgs), dim3(IF_THREADS), lds, as_stream(stream), states, labels, N, S, A, idx, total, params,
              (double*)ws, running_loss, (unsigned long long*)counts, ticket);
  return 0;
}
