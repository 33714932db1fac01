// robotic.hip — the four robotic priors of roboticPriorsLoss (reference losses/losses.py:62-99) on one minibatch of states:
// temporal coherence, causality, proportionality, repeatability (Jonschkowski & Brock), and a LINEAR state map s = W x + b fitted
// on a recording by these four terms alone (srlz/priorsfit.py).  csrc/priors.hip holds the reward and the episode prior; this file
// is the loss the reference calls `priors`.
//
// With D_b = next_states[b] - states[b], n_b = |D_b|, e_ij = exp(-|s_i - s_j|^2), the dissimilar pairs `dis` and the same-action
// pairs `same` (positions inside the minibatch, as losses/utils.py findPriorsPairs returns them):
//   temporal coherence = mean_b n_b^2            causality     = mean_dis  e_ij
//   proportionality    = mean_same (n_i - n_j)^2  repeatability = mean_same e_ij |D_i - D_j|^2
//
// Contract (include/srlz.h).
// terms (rb_terms): a workgroup of 256 threads.  Thread t takes rows t, t + 256, .. and then pairs t, t + 256, .. of each list,
// ascending; a row's or pair's value is fp32 (k ascending, fma), every thread adds its values in fp64, a wave adds by a butterfly,
// the four wave sums are added left to right, then the division by the count.  The norms n_b are kept for the gradient.
// gradient (rb_grad): thread = (row r, component c).  Both pair terms' derivatives are symmetric in the two ends of a pair, so a row
// needs only the list of its partners: the incidence table (offsets [B + 1], then partners) the host builds from the pair list, in
// pair order, a pair [i, j] giving row i the partner j and row j the partner i.  The thread walks the same-action partners, then
// the dissimilar ones, and adds in fp64 in that order; the pair scalars are recomputed per thread (k ascending), so the S threads
// of a row hold the same bits.  Where n_r = 0 the proportionality term adds nothing (torch.norm's backward).  No atomics; every
// element of both gradients is written by exactly one thread.
// Every index read from a table is clamped to the tensor it addresses: no table can make a kernel read outside.
//
// srlz_robotic_fwd / _bwd run the two on tensors in global memory (ops.RoboticPriorsFn).  srlz_robotic_fit runs every Adam step of
// a training phase in ONE launch of one persistent workgroup, the shape of invfit.hip: parameters and gradient stay in LDS as
// [D + 1][SPAD] (row d < D is W[:, d], row D the bias; one 16-byte read gives four outputs; the pads are zero and stay zero), Adam's
// moments in global memory in state_dict order.  Per step, with a barrier after each stage:
//   states   16 lanes per feature row (x_i and x_{i+1} of the minibatch's B transitions, straight from global memory): lane kk adds
//            d = kk, kk + 16, .. in that order, a butterfly over the 16 lanes, + bias -> the two state tiles [B][SPAD] in LDS
//   terms    rb_terms on the tiles; gradient: rb_grad into two more tiles
//   grads    thread = (row d of the image, quad of outputs): b ascending, the x_i product before the x_{i+1} product
//   Adam     the arithmetic of losses.hip adam_update, the step scalars evaluated in double as srlz_adam_step does
// Nothing but (parameters, m, v, running sums) is carried from step to step, all in the precision it is stored in: n steps in one
// launch and n launches of one step give the same bits.  srlz_robotic_eval: one workgroup per minibatch, the same states and terms;
// the workgroup that finishes last (an integer ticket it resets) adds the minibatches' terms in list order.
#include <math.h>

#include "common.h"

namespace {

constexpr int RB_THREADS = 256;
constexpr int RB_LDS_BYTES = 160 * 1024;
constexpr int RB_TBL = 256;  // Adam's step scalars are computed for this many steps at a time
constexpr int RB_DIR = 6;    // ints of a minibatch's directory entry: dis offset, n_dis, same offset, n_same, dis incidence, same incidence

__device__ __forceinline__ int rb_clamp(int i, int hi) { return min(max(i, 0), hi); }

// |a - b|^2 over S floats, k ascending
__device__ __forceinline__ float rb_dist2(const float* __restrict__ a, const float* __restrict__ b, int S) {
  float d2 = 0.f;
  for (int k = 0; k < S; ++k) {
    const float d = a[k] - b[k];
    d2 = fmaf(d, d, d2);
  }
  return d2;
}

// |(na - a) - (nb - b)|^2 over S floats, k ascending
__device__ __forceinline__ float rb_ddist2(const float* __restrict__ a, const float* __restrict__ na, const float* __restrict__ b,
                                           const float* __restrict__ nb, int S) {
  float d2 = 0.f;
  for (int k = 0; k < S; ++k) {
    const float d = (na[k] - a[k]) - (nb[k] - b[k]);
    d2 = fmaf(d, d, d2);
  }
  return d2;
}

// The four means of a minibatch whose states are s / ns [B] rows of `ld` floats -> every thread's return value is meaningless but
// thread q < 4 returns term q.  EVERY thread of the 256 calls it; it holds two barriers.  norms [B] is written (before the first).
__device__ __forceinline__ double rb_terms(const float* __restrict__ s, const float* __restrict__ ns, int ld, int B, int S,
                                           const int* __restrict__ dis, int nD, const int* __restrict__ same, int nP,
                                           float* __restrict__ norms, double (*slots)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = tid; b < B; b += RB_THREADS) {
    const float* __restrict__ a = s + (size_t)b * ld;
    const float* __restrict__ na = ns + (size_t)b * ld;
    float n2 = 0.f;
    for (int k = 0; k < S; ++k) {
      const float d = na[k] - a[k];
      n2 = fmaf(d, d, n2);
    }
    norms[b] = sqrtf(n2);
    acc[0] += (double)n2;
  }
  __syncthreads();  // the norms are read by other threads below
  for (int p = tid; p < nD; p += RB_THREADS) {
    const int i = rb_clamp(dis[2 * p], B - 1), j = rb_clamp(dis[2 * p + 1], B - 1);
    acc[1] += (double)expf(-rb_dist2(s + (size_t)i * ld, s + (size_t)j * ld, S));
  }
  for (int p = tid; p < nP; p += RB_THREADS) {
    const int i = rb_clamp(same[2 * p], B - 1), j = rb_clamp(same[2 * p + 1], B - 1);
    const float* __restrict__ a = s + (size_t)i * ld;
    const float* __restrict__ b = s + (size_t)j * ld;
    const float e = expf(-rb_dist2(a, b, S));
    const float dd2 = rb_ddist2(a, ns + (size_t)i * ld, b, ns + (size_t)j * ld, S);
    const float dn = norms[i] - norms[j];
    acc[2] += (double)(dn * dn);
    acc[3] += (double)(e * dd2);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double w = wave_sum_d(acc[q]);
    if (lane == 0) slots[q][wave] = w;
  }
  __syncthreads();
  double mean = 0.0;
  if (tid < 4) {
    const double total = ((slots[tid][0] + slots[tid][1]) + slots[tid][2]) + slots[tid][3];
    mean = total / (tid == 0 ? (double)B : tid == 1 ? (double)nD : (double)nP);
  }
  return mean;
}

// incidence table: offsets [B + 1], then the partners
struct RbIncidence {
  const int* tbl;
  int n;  // partners in all (twice the pairs)
};

struct RbWeights { double tc, ca, pr, re; };  // upstream gradient of each term times 2 / its count

// element (r, c) of both gradients: d / d next_states into dn, d / d states into dsv
__device__ __forceinline__ void rb_grad(const float* __restrict__ s, const float* __restrict__ ns, int ld, const float* __restrict__ norms,
                                        int B, int S, const RbIncidence& same, const RbIncidence& dis, const RbWeights& w, int r, int c,
                                        float& dsv, float& dn) {
  const float* __restrict__ sr = s + (size_t)r * ld;
  const float* __restrict__ nsr = ns + (size_t)r * ld;
  const float src = sr[c], drc = nsr[c] - src, nr = norms[r];
  double acc_d = w.tc * (double)drc;  // d loss / d D_r[c]
  double acc_s = 0.0;                 // what reaches states[r][c] through the similarities
  int o0 = rb_clamp(same.tbl[r], same.n), o1 = min(max(same.tbl[r + 1], o0), same.n);
  const int* __restrict__ part = same.tbl + B + 1;
  for (int t = o0; t < o1; ++t) {
    const int q = rb_clamp(part[t], B - 1);
    const float* __restrict__ sq = s + (size_t)q * ld;
    const float* __restrict__ nsq = ns + (size_t)q * ld;
    const float sim = expf(-rb_dist2(sr, sq, S));
    const float dd2 = rb_ddist2(sr, nsr, sq, nsq, S);
    const float dqc = nsq[c] - sq[c];
    if (nr > 0.f) acc_d += w.pr * (double)((nr - norms[q]) / nr) * (double)drc;
    acc_d += w.re * (double)sim * (double)(drc - dqc);
    acc_s -= w.re * (double)(sim * dd2) * (double)(src - sq[c]);
  }
  o0 = rb_clamp(dis.tbl[r], dis.n);
  o1 = min(max(dis.tbl[r + 1], o0), dis.n);
  part = dis.tbl + B + 1;
  for (int t = o0; t < o1; ++t) {
    const int q = rb_clamp(part[t], B - 1);
    const float* __restrict__ sq = s + (size_t)q * ld;
    const float sim = expf(-rb_dist2(sr, sq, S));
    acc_s -= w.ca * (double)sim * (double)(src - sq[c]);
  }
  dn = (float)acc_d;
  dsv = (float)(acc_s - acc_d);
}

__global__ __launch_bounds__(RB_THREADS) void robotic_fwd_kernel(const float* __restrict__ s, const float* __restrict__ ns, int B, int S,
                                                                 const int* __restrict__ dis, int nD, const int* __restrict__ same,
                                                                 int nP, float* __restrict__ norms, double* __restrict__ terms,
                                                                 float* __restrict__ terms32) {
  __shared__ double slots[4][4];
  const double mean = rb_terms(s, ns, S, B, S, dis, nD, same, nP, norms, slots);
  if (threadIdx.x < 4) {
    terms[threadIdx.x] = mean;
    terms32[threadIdx.x] = (float)mean;
  }
}

__global__ __launch_bounds__(RB_THREADS) void robotic_bwd_kernel(const float* __restrict__ s, const float* __restrict__ ns,
                                                                 const float* __restrict__ norms, int B, int S, RbIncidence same,
                                                                 RbIncidence dis, const float* __restrict__ g_tc,
                                                                 const float* __restrict__ g_ca, const float* __restrict__ g_pr,
                                                                 const float* __restrict__ g_re, float* __restrict__ ds,
                                                                 float* __restrict__ dns) {
  const long long e = (long long)blockIdx.x * RB_THREADS + threadIdx.x;
  if (e >= (long long)B * S) return;
  const int r = (int)(e / S), c = (int)(e - (long long)r * S);
  RbWeights w;
  w.tc = 2.0 * (double)g_tc[0] / (double)B;
  w.pr = 2.0 * (double)g_pr[0] / (double)(same.n >> 1);
  w.re = 2.0 * (double)g_re[0] / (double)(same.n >> 1);
  w.ca = 2.0 * (double)g_ca[0] / (double)(dis.n >> 1);
  float a, b;
  rb_grad(s, ns, S, norms, B, S, same, dis, w, r, c, a, b);
  ds[e] = a;
  dns[e] = b;
}

// ---------------------------------------------------------------------------------------------------------------- the fit

struct RbLayout {
  int D, S, SPAD, Q;  // Q: quads of outputs
  int PL;             // floats of the LDS image of the parameters (a multiple of 4)
};

__host__ __device__ inline RbLayout rb_layout(int D, int S) {
  RbLayout L;
  L.D = D; L.S = S; L.SPAD = ((S + 3) & ~3) | 4; L.Q = (S + 3) >> 2;
  L.PL = (D + 1) * L.SPAD;
  return L;
}

// floats of LDS srlz_robotic_fit needs: the parameters and the gradient, Adam's table, four tiles [B][SPAD] (states, next states and
// their gradients), the norms [B] (rounded up to 4) and the 32 of the block sums' slots (static, so they are not part of the dynamic
// request but count against the same 160 KB).  This IS the predicate srlz_robotic_supported:
//   2 * (D + 1) * SPAD + 512 + 4 * B * SPAD + ((B + 3) & ~3) + 32 <= 40960     with SPAD = (S rounded up to a multiple of 4) | 4
constexpr int RB_STATIC_FLOATS = 32;
long long rb_fit_floats(int D, int S, int B) {
  if (D < 1 || S < 1 || B < 1 || D > RB_LDS_BYTES || S > RB_LDS_BYTES || B > RB_LDS_BYTES) return -1;  // (before anything wraps)
  const long long SPAD = ((S + 3) & ~3) | 4;
  return 2LL * (D + 1) * SPAD + 2 * RB_TBL + 4LL * B * SPAD + ((B + 3) & ~3) + RB_STATIC_FLOATS;
}

bool rb_supported(int D, int S, int B) {
  const long long f = rb_fit_floats(D, S, B);
  return f > 0 && f * 4 <= RB_LDS_BYTES;
}

// parameters in state_dict order (weight [S, D], bias [S]) -> the LDS image (pads zeroed)
__device__ __forceinline__ void rb_load_params(float* __restrict__ ps, const float* __restrict__ params, const RbLayout& L, int tid) {
  for (int e = tid; e < L.PL; e += RB_THREADS) ps[e] = 0.f;
  __syncthreads();
  for (int g = tid; g < L.S * L.D; g += RB_THREADS) {
    const int k = g / L.D, d = g - k * L.D;
    ps[d * L.SPAD + k] = params[g];
  }
  for (int k = tid; k < L.S; k += RB_THREADS) ps[L.D * L.SPAD + k] = params[L.S * L.D + k];
}

// torch.optim.Adam, one element: the body of adam_update in losses.hip, of hf_adam_update and if_adam_update, so that the paths agree
__device__ __forceinline__ void rb_adam_update(float& p, float g, float& m, float& v, float step_size, float b1, float b2, float eps,
                                               float omb1, float omb2, float bc2_sqrt) {
  const float mi = b1 * m + omb1 * g;
  const float vi = b2 * v + omb2 * g * g;
  m = mi; v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p -= step_size * (mi / denom);
}

// the two state tiles of a minibatch: feature row xr = 2 b + h is x[idx[b] + h]; group grp of 16 lanes takes the rows grp, grp + 16,
// ..; lane kk adds d = kk, kk + 16, .. ascending, then a butterfly over the 16 lanes, + bias.  EVERY thread calls it (the shuffles
// need whole groups; a group without a row passes D = 0).  The pads of a tile row receive 0 (the image's pads are 0).
__device__ __forceinline__ void rb_states(const float* __restrict__ ps, const RbLayout& L, const float* __restrict__ x, int N,
                                          const int* __restrict__ irow, int B, float* __restrict__ st, float* __restrict__ nst) {
  const int grp = threadIdx.x >> 4, kk = threadIdx.x & 15;
  for (int xb = 0; xb < 2 * B; xb += 16) {
    const int xr = xb + grp;
    const bool on = xr < 2 * B;
    const int b = on ? xr >> 1 : 0, h = xr & 1;
    const int i = rb_clamp(irow[b], N - 2) + h;
    const float* __restrict__ xv = x + (size_t)i * L.D;
    const int Don = on ? L.D : 0;
    float* out = (h ? nst : st) + b * L.SPAD;
    for (int q = 0; q < L.SPAD; q += 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (q < 4 * L.Q) {
#pragma unroll 4
        for (int d = kk; d < Don; d += 16) {
          const f32x4 wv = *(const f32x4*)(ps + d * L.SPAD + q);
          const float v = xv[d];
          acc[0] = fmaf(wv[0], v, acc[0]);
          acc[1] = fmaf(wv[1], v, acc[1]);
          acc[2] = fmaf(wv[2], v, acc[2]);
          acc[3] = fmaf(wv[3], v, acc[3]);
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
      }
      if (on && kk == 0) *(f32x4*)(out + q) = acc + *(const f32x4*)(ps + L.D * L.SPAD + q);
    }
  }
}

// a minibatch's four tables out of the one buffer, every offset and count clamped so that all of it lies inside [0, len)
struct RbTables {
  const int* dis; int nD;
  const int* same; int nP;
  RbIncidence dis_inc, same_inc;
};

__device__ __forceinline__ RbTables rb_tables(const int* __restrict__ tables, int len, const int* __restrict__ dir, int mb, int B) {
  const int* e = dir + (size_t)mb * RB_DIR;
  RbTables t;
  const int od = rb_clamp(e[0], len), os = rb_clamp(e[2], len);
  t.nD = rb_clamp(e[1], (len - od) >> 1);
  t.nP = rb_clamp(e[3], (len - os) >> 1);
  t.dis = tables + od;
  t.same = tables + os;
  // an incidence table that does not fit is read as one without partners (offsets clamped to n = 0 are never followed)
  const int oid = rb_clamp(e[4], max(len - (B + 1), 0)), ois = rb_clamp(e[5], max(len - (B + 1), 0));
  t.dis_inc.tbl = tables + oid;
  t.dis_inc.n = len >= B + 1 ? min(2 * t.nD, len - (B + 1) - oid) : 0;
  t.same_inc.tbl = tables + ois;
  t.same_inc.n = len >= B + 1 ? min(2 * t.nP, len - (B + 1) - ois) : 0;
  return t;
}

__global__ __launch_bounds__(RB_THREADS) void robotic_fit_kernel(
    const float* __restrict__ x, int N, int D, int S, const int* __restrict__ idx, int n_mb, int B, const int* __restrict__ tables,
    int tables_len, const int* __restrict__ dir, const int* __restrict__ order, int n_steps, float* __restrict__ params,
    float* __restrict__ m, float* __restrict__ v, int t0, double lr, double beta1, double beta2, float eps,
    double* __restrict__ running, double* __restrict__ step_terms, float* __restrict__ last_grad) {
  extern __shared__ __attribute__((aligned(16))) float rb_smem[];
  __shared__ double slots[4][4];
  const int tid = threadIdx.x;
  const RbLayout L = rb_layout(D, S);
  const int SPAD = L.SPAD, Q = L.Q;
  float* ps = rb_smem;
  float* gs = ps + L.PL;
  float* tbl = gs + L.PL;                // [RB_TBL][2]: step_size, sqrt(bias correction 2)
  float* st = tbl + 2 * RB_TBL;          // [B][SPAD]
  float* nst = st + B * SPAD;
  float* dst = nst + B * SPAD;
  float* dnst = dst + B * SPAD;
  float* norms = dnst + B * SPAD;        // [B]

  rb_load_params(ps, params, L, tid);
  for (int e = tid; e < L.PL; e += RB_THREADS) gs[e] = 0.f;
  for (int e = tid; e < 2 * B * SPAD; e += RB_THREADS) dst[e] = 0.f;  // (both gradient tiles: their pads stay 0)
  const float b1f = (float)beta1, b2f = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const int nW = (D + 1) * Q, nP = S * D;
  double run = 0.0;  // threads 0 .. 3: the running sum of term tid
  if (tid < 4) run = running[tid];
  __syncthreads();

  for (int sbase = 0; sbase < n_steps; sbase += RB_TBL) {
    {
      // Adam's step scalars of the next RB_TBL steps, one per thread: evaluated in double and rounded once, as srlz_adam_step does
      // on the host; a function of t0 + step alone.  (The previous block's last read of tbl lies before that step's last barrier.)
      const double t = (double)t0 + (double)(sbase + tid) + 1.0;
      tbl[2 * tid] = (float)(lr / (1.0 - pow(beta1, t)));
      tbl[2 * tid + 1] = (float)sqrt(1.0 - pow(beta2, t));
    }
    const int send = min(n_steps, sbase + RB_TBL);
    for (int step = sbase; step < send; ++step) {
      const int mb = rb_clamp(order[step], n_mb - 1);
      const int* __restrict__ irow = idx + (size_t)mb * B;
      const RbTables T = rb_tables(tables, tables_len, dir, mb, B);
      rb_states(ps, L, x, N, irow, B, st, nst);
      __syncthreads();
      const double mean = rb_terms(st, nst, SPAD, B, S, T.dis, T.nD, T.same, T.nP, norms, slots);
      if (tid < 4) {
        run += mean;
        if (step_terms) step_terms[(size_t)step * 4 + tid] = mean;
      }
      {
        RbWeights w;
        w.tc = 2.0 / (double)B;
        w.ca = 2.0 / (double)max(T.nD, 1);
        w.pr = w.re = 2.0 / (double)max(T.nP, 1);
        for (int e = tid; e < B * S; e += RB_THREADS) {
          const int r = e / S, c = e - r * S;
          rb_grad(st, nst, SPAD, norms, B, S, T.same_inc, T.dis_inc, w, r, c, dst[r * SPAD + c], dnst[r * SPAD + c]);
        }
      }
      __syncthreads();
      // gradients: b ascending, the x_i product before the x_{i+1} product; row D of the image is the bias, whose input is 1
      for (int wq = tid; wq < nW; wq += RB_THREADS) {
        const int q = wq / (D + 1), d = wq - q * (D + 1);
        float* gp = gs + d * SPAD + 4 * q;
        f32x4 g = *(const f32x4*)gp;
        if (d < D) {
#pragma unroll 4
          for (int b = 0; b < B; ++b) {
            const float* __restrict__ xr = x + (size_t)rb_clamp(irow[b], N - 2) * D + d;
            const float x0 = xr[0], x1 = xr[D];
            const f32x4 d0 = *(const f32x4*)(dst + b * SPAD + 4 * q);
            const f32x4 d1 = *(const f32x4*)(dnst + b * SPAD + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = fmaf(d1[j], x1, fmaf(d0[j], x0, g[j]));
          }
        } else {
          for (int b = 0; b < B; ++b)
            g += *(const f32x4*)(dst + b * SPAD + 4 * q) + *(const f32x4*)(dnst + b * SPAD + 4 * q);
        }
        *(f32x4*)gp = g;
      }
      __syncthreads();
      const float step_size = tbl[2 * (step & (RB_TBL - 1))], bc2_sqrt = tbl[2 * (step & (RB_TBL - 1)) + 1];
      float* __restrict__ lg = (last_grad && step == n_steps - 1) ? last_grad : nullptr;
      for (int g = tid; g < nP + S; g += RB_THREADS) {
        int e;
        if (g < nP) {
          const int k = g / D;
          e = (g - k * D) * SPAD + k;
        } else {
          e = D * SPAD + (g - nP);
        }
        float mi = m[g], vi = v[g];
        const float gv = gs[e];
        rb_adam_update(ps[e], gv, mi, vi, step_size, b1f, b2f, eps, omb1, omb2, bc2_sqrt);
        m[g] = mi; v[g] = vi;
        gs[e] = 0.f;
        if (lg) lg[g] = gv;
      }
      __syncthreads();
    }
  }

  for (int g = tid; g < nP; g += RB_THREADS) {
    const int k = g / D;
    params[g] = ps[(g - k * D) * SPAD + k];
  }
  for (int k = tid; k < S; k += RB_THREADS) params[nP + k] = ps[D * SPAD + k];
  if (tid < 4) running[tid] = run;
}

__global__ __launch_bounds__(RB_THREADS) void robotic_eval_kernel(
    const float* __restrict__ x, int N, int D, int S, const int* __restrict__ idx, int n_mb, int B, const int* __restrict__ tables,
    int tables_len, const int* __restrict__ dir, const int* __restrict__ order, const float* __restrict__ params,
    double* __restrict__ partial, double* __restrict__ running, unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float rb_smem[];
  __shared__ double slots[4][4];
  __shared__ int last;
  const int tid = threadIdx.x;
  const RbLayout L = rb_layout(D, S);
  float* ps = rb_smem;
  float* st = ps + L.PL;
  float* nst = st + B * L.SPAD;
  float* norms = nst + B * L.SPAD;
  rb_load_params(ps, params, L, tid);
  __syncthreads();
  const int mb = rb_clamp(order[blockIdx.x], n_mb - 1);
  const RbTables T = rb_tables(tables, tables_len, dir, mb, B);
  rb_states(ps, L, x, N, idx + (size_t)mb * B, B, st, nst);
  __syncthreads();
  const double mean = rb_terms(st, nst, L.SPAD, B, S, T.dis, T.nD, T.same, T.nP, norms, slots);
  if (tid < 4) partial[(size_t)blockIdx.x * 4 + tid] = mean;
  // the last workgroup to finish adds the minibatches' terms, in list order
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (tid < 4) {
    double t = running[tid];
    for (unsigned w = 0; w < gridDim.x; ++w) t += partial[(size_t)w * 4 + tid];
    running[tid] = t;
  }
  if (tid == 0) atomicExch(ticket, 0u);
}

int rb_check(const char* who, const void* s, const void* ns, int B, int S, int nD, int nP) {
  SRLZ_REQUIRE(s && ns, SRLZ_ERR_NULL, "%s: null pointer", who);
  SRLZ_REQUIRE(B >= 1 && S >= 1 && (long long)B * S < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "%s: needs B >= 1 rows of S >= 1 floats and B * S < 2^31 (B=%d, S=%d)", who, B, S);
  SRLZ_REQUIRE(nD >= 1 && nP >= 1 && nD < (1 << 30) && nP < (1 << 30), SRLZ_ERR_BAD_DESC,
               "%s: needs at least one dissimilar and one same-action pair, fewer than 2^30 each (a mean of nothing is NaN): got %d "
               "and %d", who, nD, nP);
  return 0;
}

// the checks the fit and the eval share; `who` names the entry point in the error text
int rb_fit_check(const char* who, const void* x, int N, int D, int S, const void* idx, const int* idx_host, int n_mb, int B,
                 const void* tables, int tables_len, const void* dir, const int* dir_host, const void* order, const int* order_host,
                 int n, const void* params) {
  SRLZ_REQUIRE(x && idx && idx_host && tables && dir && dir_host && order && order_host && params, SRLZ_ERR_NULL, "%s: null pointer",
               who);
  SRLZ_REQUIRE(rb_supported(D, S, B), SRLZ_ERR_BAD_DESC,
               "%s: %d features, state dimension %d and minibatches of %d are outside srlz_robotic_supported: the parameters, the "
               "gradient and four state tiles must fit in %d bytes of LDS", who, D, S, B, RB_LDS_BYTES);
  SRLZ_REQUIRE(N >= 2 && (long long)N * D < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "%s: needs N >= 2 rows of features and N * D < 2^31 (N=%d, D=%d)", who, N, D);
  SRLZ_REQUIRE(n_mb >= 1 && n >= 1 && (long long)n_mb * B < (1LL << 31) && tables_len >= 1, SRLZ_ERR_BAD_DESC,
               "%s: needs at least one minibatch, one step and fewer than 2^31 rows in all (%d minibatches of %d, %d steps)", who, n_mb,
               B, n);
  const long long rows = (long long)n_mb * B;
  for (long long q = 0; q < rows; ++q)
    SRLZ_REQUIRE(idx_host[q] >= 0 && idx_host[q] <= N - 2, SRLZ_ERR_BAD_DESC,
                 "%s: index %d at position %lld lies outside [0, N - 2] (N=%d): row i is read together with row i + 1", who,
                 idx_host[q], q, N);
  for (int s = 0; s < n; ++s)
    SRLZ_REQUIRE(order_host[s] >= 0 && order_host[s] < n_mb, SRLZ_ERR_BAD_DESC, "%s: minibatch id %d at position %d lies outside [0, %d)",
                 who, order_host[s], s, n_mb);
  for (int k = 0; k < n_mb; ++k) {
    const int* e = dir_host + (size_t)k * RB_DIR;
    const long long len = tables_len;
    SRLZ_REQUIRE(e[1] >= 1 && e[3] >= 1 && e[0] >= 0 && e[2] >= 0 && e[4] >= 0 && e[5] >= 0 && e[0] + 2LL * e[1] <= len &&
                     e[2] + 2LL * e[3] <= len && e[4] + (B + 1) + 2LL * e[1] <= len && e[5] + (B + 1) + 2LL * e[3] <= len,
                 SRLZ_ERR_BAD_DESC,
                 "%s: the directory entry of minibatch %d (offsets %d, %d, %d, %d; %d dissimilar and %d same-action pairs) names an empty "
                 "pair list or reaches outside the %d table entries", who, k, e[0], e[2], e[4], e[5], e[1], e[3], tables_len);
  }
  return 0;
}

size_t rb_eval_lds_bytes(const RbLayout& L, int B) { return sizeof(float) * (size_t)(L.PL + 2 * B * L.SPAD + ((B + 3) & ~3)); }

}  // namespace

extern "C" int srlz_robotic_fwd(const float* states, const float* next_states, int B, int S, const int* dis, int n_dis,
                                const int* same, int n_same, float* norms, double* terms, float* terms32, srlz_stream_t stream) {
  const int rc = rb_check("robotic_fwd", states, next_states, B, S, n_dis, n_same);
  if (rc) return rc;
  SRLZ_REQUIRE(dis && same && norms && terms && terms32, SRLZ_ERR_NULL, "robotic_fwd: null pointer");
  SRLZ_LAUNCH(robotic_fwd_kernel, dim3(1), dim3(RB_THREADS), 0, as_stream(stream), states, next_states, B, S, dis, n_dis, same, n_same,
              norms, terms, terms32);
  return 0;
}

extern "C" int srlz_robotic_bwd(const float* states, const float* next_states, const float* norms, int B, int S,
                                const int* same_incidence, int n_same, const int* dis_incidence, int n_dis, const float* g_tc,
                                const float* g_ca, const float* g_pr, const float* g_re, float* dstates, float* dnext_states,
                                srlz_stream_t stream) {
  const int rc = rb_check("robotic_bwd", states, next_states, B, S, n_dis, n_same);
  if (rc) return rc;
  SRLZ_REQUIRE(norms && same_incidence && dis_incidence && g_tc && g_ca && g_pr && g_re && dstates && dnext_states, SRLZ_ERR_NULL,
               "robotic_bwd: null pointer");
  const long long total = (long long)B * S;
  const unsigned wgs = (unsigned)((total + RB_THREADS - 1) / RB_THREADS);
  SRLZ_LAUNCH(robotic_bwd_kernel, dim3(wgs), dim3(RB_THREADS), 0, as_stream(stream), states, next_states, norms, B, S,
              RbIncidence{same_incidence, 2 * n_same}, RbIncidence{dis_incidence, 2 * n_dis}, g_tc, g_ca, g_pr, g_re, dstates,
              dnext_states);
  return 0;
}

extern "C" int srlz_robotic_supported(int D, int S, int B) { return rb_supported(D, S, B) ? 1 : 0; }

extern "C" long long srlz_robotic_n_params(int D, int S) {
  if (D < 1 || S < 1) return 0;
  return (long long)S * D + S;
}

extern "C" int srlz_robotic_fit(const float* features, int N, int D, int S, const int* idx, const int* idx_host, int n_minibatches,
                                int B, const int* tables, int tables_len, const int* dir, const int* dir_host, const int* order,
                                const int* order_host, int n_steps, float* params, float* m, float* v, int t0, double lr, double beta1,
                                double beta2, double eps, double* running, double* step_terms, float* last_grad,
                                srlz_stream_t stream) {
  const int rc = rb_fit_check("robotic_fit", features, N, D, S, idx, idx_host, n_minibatches, B, tables, tables_len, dir, dir_host,
                              order, order_host, n_steps, params);
  if (rc) return rc;
  SRLZ_REQUIRE(m && v && running, SRLZ_ERR_NULL, "robotic_fit: null pointer");
  SRLZ_REQUIRE(t0 >= 0 && (long long)t0 + n_steps < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "robotic_fit: t0 counts the Adam steps already taken (t0=%d, n_steps=%d)", t0, n_steps);
  const size_t lds = sizeof(float) * (size_t)(rb_fit_floats(D, S, B) - RB_STATIC_FLOATS);
  SRLZ_MAX_LDS(robotic_fit_kernel, lds);
  SRLZ_LAUNCH(robotic_fit_kernel, dim3(1), dim3(RB_THREADS), lds, as_stream(stream), features, N, D, S, idx, n_minibatches, B, tables,
              tables_len, dir, order, n_steps, params, m, v, t0, lr, beta1, beta2, (float)eps, running, step_terms, last_grad);
  return 0;
}

extern "C" size_t srlz_robotic_eval_workspace(int n) {
  if (n < 1) return 0;
  return (size_t)n * 4 * sizeof(double);
}

extern "C" int srlz_robotic_eval(const float* features, int N, int D, int S, const int* idx, const int* idx_host, int n_minibatches,
                                 int B, const int* tables, int tables_len, const int* dir, const int* dir_host, const int* order,
                                 const int* order_host, int n, const float* params, double* running, void* ws, size_t ws_bytes,
                                 unsigned* ticket, srlz_stream_t stream) {
  const int rc = rb_fit_check("robotic_eval", features, N, D, S, idx, idx_host, n_minibatches, B, tables, tables_len, dir, dir_host,
                              order, order_host, n, params);
  if (rc) return rc;
  SRLZ_REQUIRE(running && ws && ticket, SRLZ_ERR_NULL, "robotic_eval: null pointer");
  const size_t need = srlz_robotic_eval_workspace(n);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "robotic_eval: workspace %zu < %zu bytes", ws_bytes, need);
  const RbLayout L = rb_layout(D, S);
  const size_t lds = rb_eval_lds_bytes(L, B);
  SRLZ_MAX_LDS(robotic_eval_kernel, lds);
  SRLZ_LAUNCH(robotic_eval_kernel, dim3((unsigned)n), dim3(RB_THREADS), lds, as_stream(stream), features, N, D, S, idx, n_minibatches,
              B, tables, tables_len, dir, order, params, (double*)ws, running, ticket);
  return 0;
}
