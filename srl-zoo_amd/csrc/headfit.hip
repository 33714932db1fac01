// headfit.hip — the reward head of the deployment objects, trained on a recording (srlz/headfit.py, LatentDynamics.refit_reward):
// the classifier Linear(2S,H)-ReLU-Linear(H,H)-ReLU-Linear(H,2) on [state ; next_state] (models/forward_inverse.py:78-95) for any
// H <= 32, cross-entropy, Adam.  The general form of reward_probe.hip (H = 4, everything in LDS), which keeps its own bits: a
// minibatch is a few hundred kFLOP at the most, so an epoch of minibatches is ONE launch (headfit_fit_kernel) and a validation
// phase ONE more (headfit_eval_kernel).
//
// Contract (include/srlz.h).  Row b of a step is states[i .. i+1] with i = idx[step][b] clamped to [0, N - 2]: the concatenation is
// the 2S floats at states + i * S and is never written out.  With K = 2S, HP = H rounded up to a multiple of 4 and HPAD = HP | 4
// (a multiple of 4 that is 4 mod 8, so a stride of HPAD floats meets only 4 of the LDS banks' 4-word groups):
//
// fit: ONE workgroup of 256 threads.  Parameters and gradient live in LDS from the first step to the last, the Adam moments stay in
// global memory in state_dict order (each is read and written once per step, coalesced over k; two more copies in LDS would halve
// the envelope).  LDS image of the parameters (hf_layout): W1 as [k][HPAD] (one 16-byte read gives four outputs of a column),
// b1[HPAD], W2 transposed [i][HPAD], b2[HPAD], W3 [2][HPAD], b3[4]; the entries beyond H are zero and stay zero.
// Per step, per chunk of at most R rows, with a barrier after each stage:
//   gather   16 lanes per row copy the 2S floats to LDS
//   layer 1  16 lanes per row and quad of outputs: lane kk adds k = kk, kk + 16, ... in that order, the 16 partial sums are added
//            by a butterfly; + b1, ReLU -> h1 in the row's record
//   layer 2  thread = (row, j): b2[j] + sum over i ascending -> h2
//   logits   thread = row: z (sum over i ascending), loss, prediction, dz, d a2
//   d a1     thread = (row, i): sum over j ascending
//   grads    thread = (column k, quad of outputs) of W1, then one thread per small parameter: rows in row order, chunk after chunk;
//            one wave adds the row losses (fp64) and counts
// then Adam on every parameter (the arithmetic of losses.hip adam_update).  Every sum has one order, a function of (S, H, B) alone;
// no float atomics; nothing but (parameters, m, v, statistics) is carried from step to step, all in the precision it is stored in:
// n steps in one launch and n launches of one step give the same bits.
//
// eval: 64 rows per workgroup, the same layer 1 straight from global memory, the same layer 2 and logits with the row loss in fp64;
// the workgroup's loss goes to ws, its counts to integer atomics (exact in any order), and the workgroup that finishes last (an
// integer ticket, reset by that workgroup) adds the partial losses in workgroup order — the pattern of reward_probe_eval_kernel.
#include <math.h>

#include "common.h"

namespace {

constexpr int HF_THREADS = 256;
constexpr int HF_MAX_S = 512;            // the rollout tile's limits (srlz_rollout_supported)
constexpr int HF_MAX_H = 32;
constexpr int HF_LDS_BYTES = 160 * 1024;
constexpr int HF_MAX_ROWS = 128;         // rows of a chunk (the logits stage runs one thread per row; counts are packed in 16 bits)
constexpr int HF_MIN_ROWS = 16;          // a shape whose chunk would be shorter is refused
constexpr int HF_TBL = 256;              // Adam's step scalars are computed for this many steps at a time
constexpr int HF_EV_ROWS = 64;           // rows of an eval workgroup

struct HfLayout {
  int K, H, HP, HPAD, hs;                // hs: log2 of the item stride of a row, the power of two >= HP
  int b1, w2, b2, w3, b3, PL;            // offsets in the LDS image and its length (a multiple of 4)
  int RS, h1, da2, h2, dz;               // row record: d a1 at 0, h1, d a2, h2 (HPAD each), dz[2], 1.0, pad
  int P, nS;                             // parameters in all, and those behind W1
};

__host__ __device__ inline HfLayout hf_layout(int S, int H) {
  HfLayout L;
  L.K = 2 * S; L.H = H; L.HP = (H + 3) & ~3; L.HPAD = L.HP | 4;
  L.hs = 2;
  while ((1 << L.hs) < L.HP) ++L.hs;
  L.b1 = L.K * L.HPAD; L.w2 = L.b1 + L.HPAD; L.b2 = L.w2 + H * L.HPAD; L.w3 = L.b2 + L.HPAD; L.b3 = L.w3 + 2 * L.HPAD;
  L.PL = L.b3 + 4;
  L.h1 = L.HPAD; L.da2 = 2 * L.HPAD; L.h2 = 3 * L.HPAD; L.dz = 4 * L.HPAD; L.RS = 4 * L.HPAD + 4;
  L.nS = H + H * H + H + 2 * H + 2;
  L.P = L.K * H + L.nS;
  return L;
}

__host__ __device__ inline int hf_row_stride(int K) { return K | 1; }  // odd: rows of a chunk start in different LDS banks

// floats of the fit kernel's LDS that do not grow with the chunk: parameters, gradient, Adam's table
inline long long hf_fixed_floats(const HfLayout& L) { return 2LL * L.PL + 2 * HF_TBL; }
// floats per row of the chunk: the row, its record, loss, flag, label (+ 1: the rounding of the rows' block to whole quads)
inline long long hf_row_floats(const HfLayout& L) { return hf_row_stride(L.K) + L.RS + 3; }

// rows of a chunk: as many as fit beside the fixed part, at most HF_MAX_ROWS; 0 where fewer than HF_MIN_ROWS fit or (S, H) lies
// outside [1, 512] x [1, 32].  This IS the predicate srlz_headfit_supported.
int hf_chunk_rows(int S, int H) {
  if (S < 1 || S > HF_MAX_S || H < 1 || H > HF_MAX_H) return 0;
  const HfLayout L = hf_layout(S, H);
  const long long room = HF_LDS_BYTES / 4 - hf_fixed_floats(L) - 4;
  if (room < 0) return 0;
  const long long r = room / hf_row_floats(L);
  if (r < HF_MIN_ROWS) return 0;
  return (int)(r < HF_MAX_ROWS ? r : HF_MAX_ROWS);
}

size_t hf_fit_lds_bytes(const HfLayout& L, int R) {
  return sizeof(float) * (size_t)(hf_fixed_floats(L) + ((R * hf_row_stride(L.K) + 3) & ~3) + (long long)R * (L.RS + 3));
}

size_t hf_eval_lds_bytes(const HfLayout& L) { return sizeof(float) * (size_t)(L.PL + HF_EV_ROWS * L.RS); }

// parameter s behind W1, in state_dict order (b1, W2 [H,H], b2, W3 [2,H], b3) -> its place in the LDS image
__device__ __forceinline__ int hf_small_lds(int s, const HfLayout& L) {
  const int H = L.H;
  if (s < H) return L.b1 + s;
  s -= H;
  if (s < H * H) { const int j = s / H; return L.w2 + (s - j * H) * L.HPAD + j; }
  s -= H * H;
  if (s < H) return L.b2 + s;
  s -= H;
  if (s < 2 * H) { const int c = s >= H; return L.w3 + c * L.HPAD + (s - c * H); }
  return L.b3 + (s - 2 * H);
}

// the same parameter's gradient as a sum over rows of record[a] * record[b]
__device__ __forceinline__ void hf_small_slots(int s, const HfLayout& L, int& a, int& b) {
  const int H = L.H, one = L.dz + 2;
  b = one;
  if (s < H) { a = s; return; }
  s -= H;
  if (s < H * H) { const int j = s / H; a = L.da2 + j; b = L.h1 + (s - j * H); return; }
  s -= H * H;
  if (s < H) { a = L.da2 + s; return; }
  s -= H;
  if (s < 2 * H) { const int c = s >= H; a = L.dz + c; b = L.h2 + (s - c * H); return; }
  a = L.dz + (s - 2 * H);
}

// parameters in state_dict order -> the LDS image (pads zeroed)
__device__ __forceinline__ void hf_load_params(float* __restrict__ ps, const float* __restrict__ params, const HfLayout& L, int tid) {
  for (int e = tid; e < L.PL; e += HF_THREADS) ps[e] = 0.f;
  __syncthreads();
  for (int j = 0; j < L.H; ++j)
    for (int k = tid; k < L.K; k += HF_THREADS) ps[k * L.HPAD + j] = params[j * L.K + k];
  for (int s = tid; s < L.nS; s += HF_THREADS) ps[hf_small_lds(s, L)] = params[L.K * L.H + s];
}

// torch.optim.Adam, one element: the body of adam_update in losses.hip and of rp_adam_update, so that the three paths agree
__device__ __forceinline__ void hf_adam_update(float& p, float g, float& m, float& v, float step_size, float b1, float b2, float eps,
                                               float omb1, float omb2, float bc2_sqrt) {
  const float mi = b1 * m + omb1 * g;
  const float vi = b2 * v + omb2 * g * g;
  m = mi; v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p -= step_size * (mi / denom);
}

// 16 lanes of a row, four outputs: a[j] = sum_k W1[k][j] x[k], lane kk adds k = kk, kk + 16, ... in order, then a butterfly over the
// 16 lanes.  w points at the quad in column 0.  Every lane of the wave calls it (the shuffles need them); an inactive row passes K = 0.
__device__ __forceinline__ f32x4 hf_layer1_quad(const float* __restrict__ w, int HPAD, const float* __restrict__ x, int K, int kk) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = kk; k < K; k += 16) {
    const f32x4 wv = *(const f32x4*)(w + k * HPAD);
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

// layer 1 of the 16 rows rb .. rb + 15 (group grp of 16 lanes = row rb + grp): h1 = relu(W1 x + b1) into the rows' records.
// x_of(row) gives the row's 2S floats.  Every thread of the block calls it.
template <class XOf>
__device__ __forceinline__ void hf_layer1_rows(const float* __restrict__ ps, float* __restrict__ rec, const HfLayout& L, int rb, int rows,
                                               int grp, int kk, XOf x_of) {
  const int rr = rb + grp;
  const bool on = rr < rows;
  const float* __restrict__ x = x_of(on ? rr : 0);
  const int Kon = on ? L.K : 0;
  for (int q = 0; q < L.HP; q += 4) {
    const f32x4 a = hf_layer1_quad(ps + q, L.HPAD, x, Kon, kk);
    if (on && kk == 0) {
      const f32x4 b = *(const f32x4*)(ps + L.b1 + q);
      f32x4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = fmaxf(a[j] + b[j], 0.f);
      *(f32x4*)(rec + rr * L.RS + L.h1 + q) = h;
    }
  }
}

// layer 2 of `rows` rows, thread = (row, j): h2[j] = relu(b2[j] + sum_i W2[j][i] h1[i]), i ascending
__device__ __forceinline__ void hf_layer2_rows(const float* __restrict__ ps, float* __restrict__ rec, const HfLayout& L, int rows, int tid) {
  for (int w = tid; w < (rows << L.hs); w += HF_THREADS) {
    const int r = w >> L.hs, j = w & ((1 << L.hs) - 1);
    if (j >= L.H) continue;
    const float* __restrict__ h1 = rec + r * L.RS + L.h1;
    float a = ps[L.b2 + j];
    for (int i = 0; i < L.H; ++i) a = fmaf(ps[L.w2 + i * L.HPAD + j], h1[i], a);
    rec[r * L.RS + L.h2 + j] = fmaxf(a, 0.f);
  }
}

// the two logits of a row from its h2, i ascending
__device__ __forceinline__ void hf_logits(const float* __restrict__ ps, const float* __restrict__ h2, const HfLayout& L, float (&z)[2]) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float a = ps[L.b3 + c];
    for (int i = 0; i < L.H; ++i) a = fmaf(ps[L.w3 + c * L.HPAD + i], h2[i], a);
    z[c] = a;
  }
}

// (correct & class 0, correct & class 1, rows of class 0, rows of class 1) of one row, 16 bits each
__device__ __forceinline__ unsigned long long hf_pack_counts(int pred, int label) {
  const unsigned long long ok = pred == label;
  return label ? (ok << 16) | (1ull << 48) : ok | (1ull << 32);
}

__device__ __forceinline__ unsigned long long hf_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int hf_clamp_index(int i, int N) { return min(max(i, 0), N - 2); }

__global__ __launch_bounds__(HF_THREADS) void headfit_fit_kernel(
    const float* __restrict__ states, const int* __restrict__ labels, int N, int S, int H, const int* __restrict__ idx, int n_steps, int B,
    int R, float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, int t0, double lr, double beta1, double beta2,
    float eps, double* __restrict__ running_loss, long long* __restrict__ counts, double* __restrict__ step_loss,
    float* __restrict__ last_grad) {
  extern __shared__ __attribute__((aligned(16))) float hf_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, kk = tid & 15;
  const HfLayout L = hf_layout(S, H);
  const int K = L.K, KS = hf_row_stride(K), RS = L.RS, HPAD = L.HPAD, Q = L.HP >> 2;
  float* ps = hf_smem;
  float* gs = ps + L.PL;
  float* xs = gs + L.PL;                              // [R][KS]
  float* rec = xs + ((R * KS + 3) & ~3);              // [R][RS]
  float* lossr = rec + R * RS;                        // [R]
  int* flag = (int*)(lossr + R);                      // [R]: prediction | label << 1
  int* labs = flag + R;                               // [R]
  float* tbl = (float*)(labs + R);                    // [HF_TBL][2]: step_size, sqrt(bias correction 2)

  hf_load_params(ps, params, L, tid);
  for (int e = tid; e < L.PL; e += HF_THREADS) gs[e] = 0.f;
  const float b1f = (float)beta1, b2f = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float invB = 1.f / (float)B;
  const int nW1 = K * Q;
  // statistics: lane 0 of wave 2
  double run = 0.0;
  long long c0 = 0, c1 = 0, n0 = 0, n1 = 0;
  if (tid == 128) run = running_loss[0];
  __syncthreads();

  for (int sbase = 0; sbase < n_steps; sbase += HF_TBL) {
    {
      // Adam's step scalars of the next HF_TBL steps, one per thread: evaluated in double and rounded once, as srlz_adam_step does
      // on the host; a function of t0 + step alone.  (The previous block's last read of tbl lies before that step's last barrier.)
      const double t = (double)t0 + (double)(sbase + tid) + 1.0;
      tbl[2 * tid] = (float)(lr / (1.0 - pow(beta1, t)));
      tbl[2 * tid + 1] = (float)sqrt(1.0 - pow(beta2, t));
    }
    const int send = min(n_steps, sbase + HF_TBL);
    for (int step = sbase; step < send; ++step) {
      double sl = 0.0;
      for (int r0 = 0; r0 < B; r0 += R) {
        const int rows = min(R, B - r0);
        const int* __restrict__ irow = idx + (size_t)step * B + r0;
        for (int rr = grp; rr < rows; rr += 16) {
          const int i = hf_clamp_index(irow[rr], N);
          const float* __restrict__ src = states + (size_t)i * S;
          float* dst = xs + rr * KS;
#pragma unroll 4
          for (int k = kk; k < K; k += 16) dst[k] = src[k];
          if (kk == 0) labs[rr] = labels[i];
        }
        __syncthreads();
        for (int rb = 0; rb < rows; rb += 16)
          hf_layer1_rows(ps, rec, L, rb, rows, grp, kk, [&](int rr) { return (const float*)(xs + rr * KS); });
        __syncthreads();
        hf_layer2_rows(ps, rec, L, rows, tid);
        __syncthreads();
        if (tid < rows) {
          float* r = rec + tid * RS;
          float z[2];
          hf_logits(ps, r + L.h2, L, z);
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
          const float dz1 = (label ? -p0 : p1) * invB, dz0 = -dz1;
          for (int i = 0; i < H; ++i) {
            const float dh = fmaf(ps[L.w3 + HPAD + i], dz1, ps[L.w3 + i] * dz0);
            r[L.da2 + i] = r[L.h2 + i] > 0.f ? dh : 0.f;
          }
          r[L.dz] = dz0;
          r[L.dz + 1] = dz1;
          r[L.dz + 2] = 1.f;
        }
        __syncthreads();
        for (int w = tid; w < (rows << L.hs); w += HF_THREADS) {
          const int rr = w >> L.hs, i = w & ((1 << L.hs) - 1);
          if (i >= L.HP) continue;
          float* r = rec + rr * RS;
          float dh = 0.f;
          if (i < H) {
            for (int j = 0; j < H; ++j) dh = fmaf(ps[L.w2 + i * HPAD + j], r[L.da2 + j], dh);
            dh = r[L.h1 + i] > 0.f ? dh : 0.f;
          }
          r[i] = dh;
        }
        __syncthreads();
        // gradients: rows in row order, chunk after chunk
        for (int w = tid; w < nW1 + L.nS; w += HF_THREADS) {
          if (w < nW1) {
            const int q = w / K, k = w - q * K;
            float* gp = gs + k * HPAD + 4 * q;
            f32x4 g = *(const f32x4*)gp;
            for (int rr = 0; rr < rows; ++rr) {
              const f32x4 dd = *(const f32x4*)(rec + rr * RS + 4 * q);
              const float xv = xs[rr * KS + k];
              g[0] = fmaf(dd[0], xv, g[0]);
              g[1] = fmaf(dd[1], xv, g[1]);
              g[2] = fmaf(dd[2], xv, g[2]);
              g[3] = fmaf(dd[3], xv, g[3]);
            }
            *(f32x4*)gp = g;
          } else {
            const int se = w - nW1;
            int sa, sb;
            hf_small_slots(se, L, sa, sb);
            float* gp = gs + hf_small_lds(se, L);
            float g = *gp;
            for (int rr = 0; rr < rows; ++rr) g = fmaf(rec[rr * RS + sa], rec[rr * RS + sb], g);
            *gp = g;
          }
        }
        if (wave == 2) {
          double l = 0.0;
          unsigned long long pk = 0;
          for (int rr = lane; rr < rows; rr += 64) {
            l += (double)lossr[rr];
            pk += hf_pack_counts(flag[rr] & 1, flag[rr] >> 1);
          }
          l = wave_sum_d(l);
          pk = hf_wave_sum_u64(pk);
          sl += l;
          c0 += (long long)(pk & 0xffff);
          c1 += (long long)((pk >> 16) & 0xffff);
          n0 += (long long)((pk >> 32) & 0xffff);
          n1 += (long long)(pk >> 48);
        }
        __syncthreads();
      }
      const float step_size = tbl[2 * (step & (HF_TBL - 1))], bc2_sqrt = tbl[2 * (step & (HF_TBL - 1)) + 1];
      float* __restrict__ lg = (last_grad && step == n_steps - 1) ? last_grad : nullptr;
      for (int j = 0; j < H; ++j) {
        for (int k = tid; k < K; k += HF_THREADS) {
          const int g = j * K + k, e = k * HPAD + j;
          float mi = m[g], vi = v[g];
          const float gv = gs[e];
          hf_adam_update(ps[e], gv, mi, vi, step_size, b1f, b2f, eps, omb1, omb2, bc2_sqrt);
          m[g] = mi; v[g] = vi;
          gs[e] = 0.f;
          if (lg) lg[g] = gv;
        }
      }
      for (int s = tid; s < L.nS; s += HF_THREADS) {
        const int g = K * H + s, e = hf_small_lds(s, L);
        float mi = m[g], vi = v[g];
        const float gv = gs[e];
        hf_adam_update(ps[e], gv, mi, vi, step_size, b1f, b2f, eps, omb1, omb2, bc2_sqrt);
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

  for (int j = 0; j < H; ++j)
    for (int k = tid; k < K; k += HF_THREADS) params[j * K + k] = ps[k * HPAD + j];
  for (int s = tid; s < L.nS; s += HF_THREADS) params[K * H + s] = ps[hf_small_lds(s, L)];
  if (tid == 128) {
    running_loss[0] = run;
    counts[0] += c0 + c1;
    counts[1] += c0;
    counts[2] += c1;
    counts[3] += n0;
    counts[4] += n1;
  }
}

__global__ __launch_bounds__(HF_THREADS) void headfit_eval_kernel(
    const float* __restrict__ states, const int* __restrict__ labels, int N, int S, int H, const int* __restrict__ idx, int total,
    const float* __restrict__ params, double* __restrict__ partial, double* __restrict__ running_loss,
    unsigned long long* __restrict__ counts, unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float hf_smem[];
  __shared__ int labs[HF_EV_ROWS];
  __shared__ double slots[4];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, kk = tid & 15;
  const HfLayout L = hf_layout(S, H);
  float* ps = hf_smem;
  float* rec = ps + L.PL;                             // [HF_EV_ROWS][RS]
  hf_load_params(ps, params, L, tid);
  const int row0 = blockIdx.x * HF_EV_ROWS, rows = min(HF_EV_ROWS, total - row0);
  if (tid < rows) labs[tid] = labels[hf_clamp_index(idx[row0 + tid], N)];
  __syncthreads();
  for (int rb = 0; rb < rows; rb += 16)
    hf_layer1_rows(ps, rec, L, rb, rows, grp, kk,
                   [&](int rr) { return states + (size_t)hf_clamp_index(idx[row0 + rr], N) * S; });
  __syncthreads();
  hf_layer2_rows(ps, rec, L, rows, tid);
  __syncthreads();
  if (wave == 0) {
    double l = 0.0;
    unsigned long long pk = 0;
    if (lane < rows) {
      float z[2];
      hf_logits(ps, rec + lane * L.RS + L.h2, L, z);
      const int label = labs[lane] == 1;
      const double z0 = (double)z[0], z1 = (double)z[1], mx = fmax(z0, z1);
      l = mx + log(exp(z0 - mx) + exp(z1 - mx)) - (label ? z1 : z0);
      pk = hf_pack_counts(z[1] > z[0], label);
    }
    l = wave_sum_d(l);
    pk = hf_wave_sum_u64(pk);
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
  for (int w = tid; w < (int)gridDim.x; w += HF_THREADS) t += partial[w];
  t = wave_sum_d(t);
  if (lane == 0) slots[wave] = t;
  __syncthreads();
  if (tid == 0) {
    running_loss[0] += ((slots[0] + slots[1]) + slots[2]) + slots[3];
    atomicExch(ticket, 0u);
  }
}

// the checks both entry points share; `who` names the entry point in the error text
int hf_check(const char* who, const void* states, const void* labels, int N, int S, int H, const void* idx, const int* idx_host,
             long long n, int B, const void* params) {
  SRLZ_REQUIRE(states && labels && idx && idx_host && params, SRLZ_ERR_NULL, "%s: null pointer", who);
  SRLZ_REQUIRE(hf_chunk_rows(S, H) > 0, SRLZ_ERR_BAD_DESC,
               "%s: state dimension %d with %d hidden units is outside srlz_headfit_supported: 1 <= S <= %d, 1 <= H <= %d, and the "
               "parameters, the gradient and a chunk of %d rows must fit in %d bytes of LDS",
               who, S, H, HF_MAX_S, HF_MAX_H, HF_MIN_ROWS, HF_LDS_BYTES);
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

extern "C" int srlz_headfit_chunk_rows(int S, int H) { return hf_chunk_rows(S, H); }

extern "C" int srlz_headfit_supported(int S, int H) { return hf_chunk_rows(S, H) > 0; }

extern "C" long long srlz_headfit_n_params(int S, int H) {
  if (S < 1 || H < 1) return 0;
  return 2LL * S * H + H + (long long)H * H + H + 2LL * H + 2;
}

extern "C" int srlz_headfit_fit(const float* states, const int* labels, int N, int S, int H, const int* idx, const int* idx_host,
                                int n_steps, int B, float* params, float* m, float* v, int t0, double lr, double beta1, double beta2,
                                double eps, double* running_loss, long long* counts, double* step_loss, float* last_grad,
                                srlz_stream_t stream) {
  const int rc = hf_check("headfit_fit", states, labels, N, S, H, idx, idx_host, n_steps, B, params);
  if (rc) return rc;
  SRLZ_REQUIRE(m && v && running_loss && counts, SRLZ_ERR_NULL, "headfit_fit: null pointer");
  SRLZ_REQUIRE(t0 >= 0 && (long long)t0 + n_steps < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "headfit_fit: t0 counts the Adam steps already taken (t0=%d, n_steps=%d)", t0, n_steps);
  const HfLayout L = hf_layout(S, H);
  const int R = hf_chunk_rows(S, H) < B ? hf_chunk_rows(S, H) : B;
  const size_t lds = hf_fit_lds_bytes(L, R);
  SRLZ_MAX_LDS(headfit_fit_kernel, lds);
  SRLZ_LAUNCH(headfit_fit_kernel, dim3(1), dim3(HF_THREADS), lds, as_stream(stream), states, labels, N, S, H, idx, n_steps, B, R, params,
              m, v, t0, lr, beta1, beta2, (float)eps, running_loss, counts, step_loss, last_grad);
  return 0;
}

extern "C" size_t srlz_headfit_eval_workspace(int n_batches, int B) {
  if (n_batches < 1 || B < 1 || (long long)n_batches * B >= (1LL << 31)) return 0;
  const long long rows = (long long)n_batches * B;
  return (size_t)((rows + HF_EV_ROWS - 1) / HF_EV_ROWS) * sizeof(double);
}

extern "C" int srlz_headfit_eval(const float* states, const int* labels, int N, int S, int H, const int* idx, const int* idx_host,
                                 int n_batches, int B, const float* params, double* running_loss, long long* counts, void* ws,
                                 size_t ws_bytes, unsigned* ticket, srlz_stream_t stream) {
  const int rc = hf_check("headfit_eval", states, labels, N, S, H, idx, idx_host, n_batches, B, params);
  if (rc) return rc;
  SRLZ_REQUIRE(running_loss && counts && ws && ticket, SRLZ_ERR_NULL, "headfit_eval: null pointer");
  const size_t need = srlz_headfit_eval_workspace(n_batches, B);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "headfit_eval: workspace %zu < %zu bytes", ws_bytes, need);
  const HfLayout L = hf_layout(S, H);
  const int total = n_batches * B;
  const unsigned wgs = (unsigned)((total + HF_EV_ROWS - 1) / HF_EV_ROWS);
  const size_t lds = hf_eval_lds_bytes(L);
  SRLZ_MAX_LDS(headfit_eval_kernel, lds);
  SRLZ_LAUNCH(headfit_eval_kernel, dim3(wgs), dim3(HF_THREADS), lds, as_stream(stream), states, labels, N, S, H, idx, total, params,
              (double*)ws, running_loss, (unsigned long long*)counts, ticket);
  return 0;
}
