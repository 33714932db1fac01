// rollout_tile.h — the 32-row state tile of the deployment dynamics, shared by rollout.hip (plans the caller brings), plan.hip (plans
// sampled on the device) and horizon.hip (the recorded actions of a dataset, each step compared with the recorded state): one text of
// the MFMA helper, the step loop and the reward head, instantiated once per source of rows.
// A row source says which rows of the tile exist, which environment's state a row starts from, where its outputs go and which action
// it takes at each step; everything else — every sum's order, every rounding — is the same text, so the kernels leave the same
// bits for the same plans.  Internal to csrc/: included after common.h.
#pragma once
#include <math.h>
#include "common.h"

namespace rollout_tile {

constexpr int RO_ROWS = 32;     // rows a workgroup owns
constexpr int RO_LD = 33;       // floats between two k of the state tile / two rows of the small tiles
constexpr int RO_MAX_S = 512;
constexpr int RO_MAX_H = 32;
constexpr int RO_MAX_A = 65536;
constexpr int RO_WAVES = 8;
constexpr int RO_THREADS = 64 * RO_WAVES;
constexpr int RO_KC = 32;       // k of a chunk: the B-operand loads in flight ahead of its 16 MFMAs
constexpr int RO_GOAL_Q = RO_THREADS / RO_ROWS;  // partial sums of a row's goal distance: one per column group
constexpr size_t RO_LDS_CAP = 160 * 1024;        // LDS of a CU

// What the tile reads and writes, whatever the source of its rows.
struct TileArgs {
  const float* states;   // [N,S]
  const float *wf, *bf;  // [S,S+A], [S]
  const float *w1, *b1, *w2, *b2, *w3, *b3;  // [H,2S],[H],[H,H],[H],[2,H],[2]; w1 == NULL: no reward head
  float *final_states, *returns, *trajectory, *logits;  // by output row; each may be NULL
  int T, S, A, H;
  float gamma;
};

// The goal term of the score (ro_tile<Rows, true> alone takes one): ret += g * (prob - w * c_t), or g * -(w * c_t) without a reward
// head.  A kernel argument of its own, so that the kernels without a goal keep the arguments — and the code — they had.
struct GoalArgs {
  const float* goal;  // [N,S], or one [S] with stride 0
  long long stride;   // floats between two environments' goals
  float w;
  int final;          // c_t = d_t at every step (0) or at t == T-1 alone (1)
  float* dist;        // by output row, [T] each; may be NULL
};

// The third mode of the tile (ro_tile<Rows, RO_TRACK>, csrc/horizon.hip): no score; the reduction's target moves with the step — row
// rows.target(i, t) of p.states itself, the recorded state that the imagined s_{t+1} is compared with — and next to that error the
// distance the row's start state has to the same target.  A kernel argument of its own, as GoalArgs is.
struct TrackArgs {
  float *err, *base;  // by output row, [T] each: |s_{t+1} - target|^2 and |s_0 - target|^2; NaN where the row has no step t
};

// The tile's compile-time modes: the bare score, the goal term in the score (these two are the `Goal = false / true` the tile had,
// and convert from it), the moving target.
constexpr int RO_SCORE = 0, RO_GOAL = 1, RO_TRACK = 2;

__host__ __device__ inline int ro_sp(int S) { return (S + RO_KC - 1) & ~(RO_KC - 1); }  // the tile's k, whole chunks

// floats of LDS: state tile, 8 partial blocks, h1, h2, W2, W3, b1, b2, b3 (+2 pad), the goal distance's 16 partials a row, then
// 2 * 32 ints
__host__ __device__ inline size_t ro_lds_bytes(int S, bool reward, bool goal = false) {
  size_t fl = (size_t)ro_sp(S) * RO_LD;
  if (reward) fl += RO_WAVES * RO_ROWS * RO_LD + 2 * RO_ROWS * RO_LD + RO_MAX_H * RO_MAX_H + 2 * RO_MAX_H + 2 * RO_MAX_H + 4;
  if (goal) fl += RO_GOAL_Q * RO_LD;
  return (fl + 2 * RO_ROWS) * 4;
}

// RO_TRACK: two reductions a step, the goal term's partials twice.
__host__ __device__ inline size_t ro_track_lds_bytes(int S, bool reward) {
  return ro_lds_bytes(S, reward, true) + (size_t)RO_GOAL_Q * RO_LD * 4;
}

inline int ro_supported(int S, int A, int H, int n_rewards) {
  return S >= 1 && S <= RO_MAX_S && A >= 1 && A <= RO_MAX_A && H >= 1 && H <= RO_MAX_H && n_rewards == 2;
}

// With the goal term (srlz_rollout_goal_supported is this; the planner adds its own LDS on top): the head's limits — none without a
// head — and the tile with the goal's partials inside the CU's LDS.
inline int ro_goal_supported(int S, int A, int H, int n_rewards, int has_reward) {
  return ro_supported(S, A, has_reward ? H : 1, has_reward ? n_rewards : 2) && ro_lds_bytes(S, has_reward != 0, true) <= RO_LDS_CAP;
}

// With the moving target (srlz_horizon_supported is this): the same limits, the tile with both reductions' partials inside the LDS.
inline int ro_track_supported(int S, int A, int H, int n_rewards, int has_reward) {
  return ro_supported(S, A, has_reward ? H : 1, has_reward ? n_rewards : 2) && ro_track_lds_bytes(S, has_reward != 0) <= RO_LDS_CAP;
}

// acc += st[32 x k-range] . W[j][koff + k]^T over the chunks c0, c0 + cstep, .. of 32 k each.  w (uniform) + woff (this lane's row
// and koff, below 2^30 floats at the limits; a row inside the matrix when the lane's column does not exist: jok = false zeroes what
// it reads).  The k-order inside an MFMA is free as long as both operands agree: lanes 0-31 take k = 32c .. 32c+15 of a chunk, lanes
// 32-63 k = 32c+16 .. 32c+31, so a lane's share of the B operand is 64 contiguous bytes of its row — four 16-byte loads (rows are only
// 4-byte aligned: S + A is arbitrary) instead of sixteen dwords from sixteen different cache-line visits.  Whole chunks need no mask;
// the chunk that holds k = S (if S is no multiple of 32) is read dword by dword, branch-free: a k outside [0, S) reads element 0 of
// the row and is zeroed.  Its loads are issued first and its MFMAs run last.
__device__ __forceinline__ void ro_gemm(f32x16& acc, const float* st, const float* __restrict__ w, unsigned woff, bool jok, int S,
                                        int c0, int cstep, int h, int l31) {
  constexpr int NK = RO_KC / 2;  // k of a chunk per lane = MFMAs per chunk
  const int nfull = S / RO_KC;
  const bool tail = (S % RO_KC) != 0 && nfull >= c0 && (nfull - c0) % cstep == 0;
  float bt[NK], bn[NK], bc[NK];
  if (tail) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int k = RO_KC * nfull + NK * h + i;
      const bool ok = jok && k < S;
      const float v = w[woff + (ok ? k : 0)];
      bt[i] = ok ? v : 0.f;
    }
  }
  auto fetch = [&](int c) {
    const float* src = w + woff + (RO_KC * c + NK * h);
#pragma unroll
    for (int q = 0; q < NK / 4; ++q) {
      f32x4 v;
      __builtin_memcpy(&v, src + 4 * q, 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) bn[4 * q + e] = v[e];
    }
  };
  auto mfmas = [&](int c, const float (&b)[NK]) {
    const float* a = st + (RO_KC * c + NK * h) * RO_LD + l31;
#pragma unroll
    for (int i = 0; i < NK; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i * RO_LD], b[i], acc, 0, 0, 0);
  };
  if (c0 < nfull) {
    fetch(c0);
    for (int c = c0; c < nfull; c += cstep) {
#pragma unroll
      for (int i = 0; i < NK; ++i) bc[i] = jok ? bn[i] : 0.f;
      fetch(c + cstep < nfull ? c + cstep : c);  // (behind the last whole chunk: read it again, dropped)
      mfmas(c, bc);
    }
  }
  if (tail) mfmas(nfull, bt);
}

__device__ __forceinline__ float ro_relu(float v) { return v < 0.f ? 0.f : v; }  // NaN stays NaN

// One step of the score with the goal term, as include/srlz.h states it: fl(w * c), fl(prob - .), fl(g * term), fl(ret + .), fl(g * gamma),
// each rounded on its own.  Plain operators under contract(off): the __fmul_rn / __fadd_rn of this toolchain are plain operators that
// the default contraction mode fuses into one FMA (as it does in the reward branch's ret + g * prob, whose bits stand as they are).
__device__ __forceinline__ void ro_goal_step(float& ret, float& g, float prob, bool reward, float w, float c, float gamma) {
#pragma clang fp contract(off)
  const float wc = w * c;
  const float term = reward ? prob - wc : -wc;
  const float gt = g * term;
  ret = ret + gt;
  g = g * gamma;
}

// A row's squared distance to its goal: 16 partial sums, each an fma chain over its columns in ascending order, added in group order.
__device__ __forceinline__ float ro_goal_sum(const float* gq, int row) {
#pragma clang fp contract(off)
  float d = gq[row];
#pragma unroll
  for (int q = 1; q < RO_GOAL_Q; ++q) d = d + gq[q * RO_LD + row];
  return d;
}

// The tile for all T steps.  `lds`: ro_lds_bytes(S, reward) bytes, 16-byte aligned.  Rows: a row source with
//   bool exists(int i)          row i of the tile is a row of the call (asked by any thread)
//   long long env(int i)        the row of p.states row i starts from (an existing row)
//   long long out(int i)        the row of every output that row i writes (an existing row)
//   void begin(int i)           called once by thread i < 32 of an existing row, before its first action is asked for
//   int action(int i, int t)    row i's action at step t: asked once per step, in step order, by thread i < 32 alone and only
//                               for an existing row — one step ahead of the step that uses it
// Mode (compile time).  RO_GOAL: the goal-distance term of include/srlz.h joins the score; gp is then given and `lds` is
// ro_lds_bytes(S, reward, true) bytes.  RO_TRACK: tp is given, `lds` is ro_track_lds_bytes(S, reward) bytes, and the row source has
//   long long target(int i, int t)   the row of p.states that row i's s_{t+1} is compared with, -1: the row has no step t (asked by
//                                    any thread of an existing row)
// Without a mode not one instruction of it exists.
// Ends behind a workgroup barrier: every output of the tile has been issued by its thread.
template <class Rows, int Mode = RO_SCORE>
__device__ __forceinline__ void ro_tile(const TileArgs& p, float* lds, Rows& rows, const GoalArgs* gp = nullptr,
                                        const TrackArgs* tp = nullptr) {
  constexpr bool Goal = Mode == RO_GOAL, Track = Mode == RO_TRACK;
  const int S = p.S, A = p.A, H = p.H, T = p.T;
  const bool reward = p.w1 != nullptr;
  const int sp = ro_sp(S), nblk = (S + 31) >> 5;
  float* st = lds;
  float* fp = st + sp * RO_LD;
  float *red = nullptr, *h1 = nullptr, *h2 = nullptr, *w2s = nullptr, *w3s = nullptr, *b1s = nullptr, *b2s = nullptr, *b3s = nullptr;
  if (reward) {
    red = fp; fp += RO_WAVES * RO_ROWS * RO_LD;
    h1 = fp; fp += RO_ROWS * RO_LD;
    h2 = fp; fp += RO_ROWS * RO_LD;
    w2s = fp; fp += RO_MAX_H * RO_MAX_H;
    w3s = fp; fp += 2 * RO_MAX_H;
    b1s = fp; fp += RO_MAX_H;
    b2s = fp; fp += RO_MAX_H;
    b3s = fp; fp += 4;
  }
  float* gq = nullptr;  // the goal distance's partials: gq[q * RO_LD + row]
  if constexpr (Goal) { gq = fp; fp += RO_GOAL_Q * RO_LD; }
  [[maybe_unused]] float* bq = nullptr;  // (Track) the start state's distance to the same target, as gq
  if constexpr (Track) { gq = fp; fp += RO_GOAL_Q * RO_LD; bq = fp; fp += RO_GOAL_Q * RO_LD; }
  int* act = (int*)fp;        // this step's action of each row, -1 = outside [0, A)
  int* bad = act + RO_ROWS;   // sticky: the row met an action outside [0, A)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h_ = lane >> 5, l31_ = lane & 31;
  const int ldw = S + A;
  const float nanf_ = __int_as_float(0x7fc00000);

  // ---- step 0: the rows' states (rows that do not exist and k >= S: zeros), the small reward-head operands, the first actions ----
  for (int e = tid; e < RO_ROWS * sp; e += RO_THREADS) {
    const int i = e / sp, k = e - i * sp;
    float v = 0.f;
    if (rows.exists(i) && k < S) v = p.states[rows.env(i) * S + k];
    st[k * RO_LD + i] = v;
  }
  if (reward) {
    for (int e = tid; e < H * H; e += RO_THREADS) w2s[e] = p.w2[e];
    for (int e = tid; e < 2 * H; e += RO_THREADS) w3s[e] = p.w3[e];
    for (int e = tid; e < H; e += RO_THREADS) { b1s[e] = p.b1[e]; b2s[e] = p.b2[e]; }
    if (tid < 2) b3s[tid] = p.b3[tid];
  }
  bool mine = false;  // threads 0..31: row tid exists, its actions are asked for here
  float ret = 0.f, g = 1.f;
  if (tid < RO_ROWS) {
    bad[tid] = 0;
    mine = rows.exists(tid);
    if (mine) {
      rows.begin(tid);
      const int a = rows.action(tid, 0);
      const bool ok = (unsigned)a < (unsigned)A;
      act[tid] = ok ? a : -1;
      if (!ok) bad[tid] = 1;
    } else {
      act[tid] = 0;
    }
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    // ---- forward model GEMM on s_t, and the s_t half of reward layer 1 ----
    // (an opaque zero in this step's lane coordinates: without it the compiler computes every GEMM's first addresses and masks once,
    // outside the step loop, and keeps ~100 registers of them alive through it)
    int tz = 0;
    asm volatile("" : "+v"(tz));
    const int h = h_ + tz, l31 = l31_ + tz;
    f32x16 acc[2], racc;
#pragma unroll
    for (int r = 0; r < 16; ++r) racc[r] = 0.f;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bi][r] = 0.f;
      const int blk = wave + RO_WAVES * bi;
      if (blk < nblk) {
        const int j = blk * 32 + l31;
        const bool jok = j < S;
        const unsigned woff = (unsigned)(jok ? j : 0) * (unsigned)ldw;
        // the one-hot's column of each of the lane's 16 rows: requested here, added behind the block's k-loop
        float wa[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int a = act[(r & 3) + 8 * (r >> 2) + 4 * h];
          const float v = p.wf[woff + (unsigned)(S + (a >= 0 ? a : 0))];
          wa[r] = a >= 0 ? v : nanf_;
        }
        ro_gemm(acc[bi], st, p.wf, woff, jok, S, 0, 1, h, l31);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[bi][r] = __fadd_rn(acc[bi][r], wa[r]);
      }
    }
    if (reward) ro_gemm(racc, st, p.w1, (unsigned)(l31 < H ? l31 : 0) * (unsigned)(2 * S), l31 < H, S, wave, RO_WAVES, h, l31);
    __syncthreads();  // every wave has read s_t

    // ---- epilogue: s_{t+1} into the tile ----
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int blk = wave + RO_WAVES * bi;
      const int j = blk * 32 + l31;
      if (blk < nblk && j < S) {
        const float bj = p.bf[j];
        float* sj = st + j * RO_LD;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
          const float sn = __fadd_rn(sj[i], __fadd_rn(acc[bi][r], bj));
          sj[i] = bad[i] ? nanf_ : sn;
        }
      }
    }
    __syncthreads();  // s_{t+1} is in the tile

    // ---- goal distance: thread (row i, column group q) sums fl(s_{t+1}[j] - goal[j])^2 over j = q, q + 16, .. in ascending order ----
    if constexpr (Goal) {
      const int i = tid & 31, q = tid >> 5;
      float part = 0.f;
      if (rows.exists(i)) {  // (a tile may straddle environments: each row reads its own environment's goal)
        const float* gl = gp->goal + rows.env(i) * gp->stride;
        for (int j = q; j < S; j += RO_GOAL_Q) {
          const float e = __fsub_rn(st[j * RO_LD + i], gl[j]);
          part = fmaf(e, e, part);
        }
      }
      gq[q * RO_LD + i] = part;
      if (!reward) __syncthreads();  // (with a reward head its barriers stand between these writes and the row's sum)
    }

    // ---- moving target: thread (row i, column group q), the goal distance's order twice — the tile and the row's start state
    // against row target(i, t) of the states ----
    if constexpr (Track) {
      const int i = tid & 31, q = tid >> 5;
      float part = 0.f, bpart = 0.f;
      const long long tg = rows.exists(i) ? rows.target(i, t) : -1;
      if (tg >= 0) {
        const float* tl = p.states + tg * S;
        const float* s0 = p.states + rows.env(i) * S;
        for (int j = q; j < S; j += RO_GOAL_Q) {
          const float x = tl[j];
          const float e = __fsub_rn(st[j * RO_LD + i], x);
          const float b = __fsub_rn(s0[j], x);
          part = fmaf(e, e, part);
          bpart = fmaf(b, b, bpart);
        }
      }
      gq[q * RO_LD + i] = part;
      bq[q * RO_LD + i] = bpart;
      if (!reward) __syncthreads();  // (as above)
    }

    // ---- s_{t+1} out: wave w writes rows 4w .. 4w+3 of the tile, a row's S floats along the lanes ----
    if (p.trajectory || (t == T - 1 && p.final_states)) {
      for (int i = wave * (RO_ROWS / RO_WAVES); i < (wave + 1) * (RO_ROWS / RO_WAVES); ++i) {
        if (!rows.exists(i)) break;  // (the rows that exist come first)
        const long long rg = rows.out(i);
        float* tr = p.trajectory ? p.trajectory + (rg * T + t) * S : nullptr;
        float* fin = t == T - 1 && p.final_states ? p.final_states + rg * S : nullptr;
        for (int j = lane; j < S; j += 64) {
          const float v = st[j * RO_LD + i];
          if (tr) tr[j] = v;
          if (fin) fin[j] = v;
        }
      }
    }

    if (reward) {
      // ---- the s_{t+1} half of layer 1, partial blocks to LDS ----
      ro_gemm(racc, st, p.w1, (unsigned)(l31 < H ? l31 : 0) * (unsigned)(2 * S) + (unsigned)S, l31 < H, S, wave, RO_WAVES, h, l31);
      if (l31 < H) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
          red[(wave * RO_ROWS + i) * RO_LD + l31] = racc[r];
        }
      }
      __syncthreads();
      const int i = tid & 31, jg = tid >> 5;
      for (int j = jg; j < H; j += RO_THREADS / 32) {
        const float* q = red + i * RO_LD + j;
        float s = q[0];
#pragma unroll
        for (int w = 1; w < RO_WAVES; ++w) s = __fadd_rn(s, q[w * RO_ROWS * RO_LD]);
        h1[i * RO_LD + j] = ro_relu(__fadd_rn(s, b1s[j]));
      }
      __syncthreads();
      for (int j = jg; j < H; j += RO_THREADS / 32) {
        float s = 0.f;
        for (int m = 0; m < H; ++m) s = fmaf(h1[i * RO_LD + m], w2s[j * H + m], s);
        h2[i * RO_LD + j] = ro_relu(__fadd_rn(s, b2s[j]));
      }
      __syncthreads();
    }
    if (tid < RO_ROWS) {
      [[maybe_unused]] float pgoal = 0.f;  // (Goal) this step's prob, kept for the goal step below
      if (reward) {
        float l0 = 0.f, l1 = 0.f;
        for (int m = 0; m < H; ++m) {
          const float v = h2[tid * RO_LD + m];
          l0 = fmaf(v, w3s[m], l0);
          l1 = fmaf(v, w3s[H + m], l1);
        }
        l0 = __fadd_rn(l0, b3s[0]);
        l1 = __fadd_rn(l1, b3s[1]);
        if (bad[tid]) l0 = l1 = nanf_;
        const float prob = 1.f / (1.f + expf(l0 - l1));
        if constexpr (Goal) {
          pgoal = prob;
        } else {
          ret = __fadd_rn(ret, __fmul_rn(g, prob));
          g = __fmul_rn(g, p.gamma);
        }
        if (mine) {
          const long long rg = rows.out(tid);
          if (p.logits) {
            float* o = p.logits + (rg * T + t) * 2;
            o[0] = l0;
            o[1] = l1;
          }
          if (!Goal && t == T - 1 && p.returns) p.returns[rg] = ret;
        }
      }
      if constexpr (Goal) {
        const float d = ro_goal_sum(gq, tid);
        ro_goal_step(ret, g, pgoal, reward, gp->w, (!gp->final || t == T - 1) ? d : 0.f, p.gamma);
        if (mine) {
          const long long rg = rows.out(tid);
          if (gp->dist) gp->dist[rg * T + t] = d;
          if (t == T - 1 && p.returns) p.returns[rg] = ret;
        }
      }
      if constexpr (Track) {
        if (mine) {
          const long long rg = rows.out(tid);
          const bool has = rows.target(tid, t) >= 0;
          const float e = ro_goal_sum(gq, tid), b = ro_goal_sum(bq, tid);
          tp->err[rg * T + t] = has ? e : nanf_;
          tp->base[rg * T + t] = has ? b : nanf_;
        }
      }
      if (t + 1 < T && mine) {  // the next step's action (read by the epilogue, two barriers from here)
        const int a = rows.action(tid, t + 1);
        const bool ok = (unsigned)a < (unsigned)A;
        act[tid] = ok ? a : -1;
        if (!ok) bad[tid] = 1;
      }
    }
    __syncthreads();
  }
}

}  // namespace rollout_tile
