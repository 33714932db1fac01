// beam.hip — deployment tree search: exact enumeration or a beam of width W over the discrete action sequences of the learned
// dynamics, ONE launch per level of the tree, no plan and no frontier ever on the host.  Composes, per expanded node, the reference's
// models/forward_inverse.py:21-31 (forwardModel) and :78-95 (rewardModel) exactly as rollout.hip does: the step is the text of
// rollout_tile.h.  Sequences that share a prefix share its states: every prefix is expanded once, A + A^2 + .. + A^T forward steps
// for all A^T leaves where a rollout over the enumerated plans runs T * A^T.
//
// A level (include/srlz.h states the algorithm).  The frontier of level t has F_t nodes per environment; child c = f * A + a of node
// f and action a, C_t = F_t * A children.  Grid N x ceil(C_t / 32) workgroups of 512 threads; a workgroup owns 32 children of ONE
// environment (tiles do not straddle environments, so the goal pointer handed to the tile is already the environment's, stride 0)
// and runs the 32-row state tile for ONE step through a row source of its own: a child's start row is its parent's row in the
// previous level's child-state buffer (level 0: the caller's state), its action c % A, its output row its own in this level's
// buffer.  Two ping-pong state buffers and two return buffers in the workspace; a selected child's state is read in place by the
// next level, nothing is copied.  The last level writes no states.
// The return.  A one-step tile call starts from ret = 0, g = 1 and so leaves the step's term itself: prob (fl(1 * prob + 0)) without
// a goal, fl(prob - fl(w * c)) or -fl(w * c) with one.  The child's ret continues its parent's with that term under the tile's own
// expression and contraction mode — ret + g * prob (one FMA, as in ro_tile's score branch) or ro_goal_step's two separately rounded
// operations — with g_t = fl(g_{t-1} * gamma) computed by the launcher in fp32.  A leaf's ret is therefore, bit for bit, what
// srlz_rollout / srlz_rollout_goal return for the leaf's plan.  Goal mode "final": the distance enters at level T-1 alone, so the
// levels before it run the tile without its goal term (c = 0: term = fl(prob - 0) = prob, or -0 without a head).
// Finisher.  The workgroup that takes an environment's last ticket of the level (plan.hip's integer ticket: __threadfence,
// atomicAdd, no spinning, no grid barrier; it resets the ticket) selects the next frontier when C_t > W: 64-bit words
// (~monotone(key) << 32 | c) — key = ret, NaN read as -inf, -0 as +0 — sorted ascending by a bitonic network in the LDS the tile
// no longer needs (C_t <= 8192: 64 KB of the 160), integer compares only; the first W words are the frontier, in (key descending, c
// ascending) order.  Levels that prune nothing take no ticket: the next frontier is the identity.  At the last level the finisher
// takes the minimum word (the greatest key, the lowest c), reads the plan back through the parents and, when asked, every leaf's.
// No float atomics, every loop bounded: two runs are bit-identical.
// LDS: max(tile, sort) — tile 117 KB at the limits (S = 512, H = 32, goal), sort 8 * 2^ceil(log2 C_t) <= 64 KB — + 0.3 KB static.
// 168 VGPRs (186 with the goal term), no scratch (tools/isa_audit.py): the tile's step is rollout_kernel's, 128 MFMAs a step.
#include <math.h>
#include "common.h"
#include "rollout_tile.h"

using namespace rollout_tile;

namespace {

constexpr int BM_MAX_T = 32;
constexpr int BM_MAX_C = 8192;  // children of a level per environment: W * A

struct BeamArgs {
  TileArgs tile;          // states: the parents' rows; final_states: this level's child states (NULL at the last level); T = 1
  float* ret;             // this level's child returns, by output row
  const float* pret;      // the parents' returns, by parent row (level 0: unused)
  const int* sel;         // this level's frontier [N,W]: node f is child sel[n][f] of the level before; NULL = the identity
  int* sel_out;           // finish 1: the next level's frontier [N,W]
  const int* sel_all;     // every level's frontier [T-1,N,W] (level t at t-1), read back by the last level
  unsigned* tickets;      // [N]
  int* best_plan;         // [N,T]
  float* best_return;     // [N]
  int* leaf_plans;        // [N,L,T] or NULL
  float* leaf_returns;    // [N,L] or NULL
  long long pstride, ostride;  // rows between two environments in the parents' / this level's buffers
  unsigned pruned;        // bit t: level t's frontier came from a selection (sel_all holds it); else the identity
  int N, W, C, tiles, level, horizon;
  float g;                // g_t
  int has_val;            // the tile left this step's term in ret (else the term is -0: goal mode final before T-1, no head)
  int finish;             // 0: nothing; 1: select the next frontier; 2: the last level
};

// Rows of one environment's tile: row i is child c0 + i of environment n.
struct BeamRows {
  const BeamArgs& p;
  const long long* prow;  // LDS: the 32 rows' parent rows
  const int n, c0;
  __device__ __forceinline__ bool exists(int i) const { return c0 + i < p.C; }
  __device__ __forceinline__ long long env(int i) const { return prow[i]; }
  __device__ __forceinline__ long long out(int i) const { return (long long)n * p.ostride + c0 + i; }
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ int action(int i, int) const { return (c0 + i) % p.tile.A; }
};

template <class T>
__device__ __forceinline__ T load_agent(const T* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ret continued by one step's term: the score branch of ro_tile (one expression, the default contraction mode) ...
__device__ __forceinline__ float bm_continue(float ret, float g, float prob) { return __fadd_rn(ret, __fmul_rn(g, prob)); }

// ... and ro_goal_step's last two operations, each rounded on its own.
__device__ __forceinline__ float bm_continue_goal(float ret, float g, float term) {
#pragma clang fp contract(off)
  const float gt = g * term;
  ret = ret + gt;
  return ret;
}

// (~monotone(key) << 32) | c: ascending words are (key descending, c ascending).  NaN reads as -inf, -0 as +0.
__device__ __forceinline__ unsigned long long bm_word(float v, int c) {
  if (v != v) v = -INFINITY;
  unsigned u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;
  const unsigned mono = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)(~mono) << 32) | (unsigned)c;
}

// The plan of child c of the last level, read back through the parents.
__device__ __forceinline__ void bm_walk(const BeamArgs& p, int n, int c, int* dst) {
  const int A = p.tile.A;
  int cur = c;
  for (int t = p.horizon - 1; t >= 0; --t) {
    const int f = cur / A, act = cur - f * A;
    // (the parent is asked for before the action is stored: the wait for it then leaves the store in flight)
    if (t > 0) cur = ((p.pruned >> t) & 1u) ? p.sel_all[((long long)(t - 1) * p.N + n) * p.W + f] : f;
    dst[t] = act;
  }
}

// One level for one tile of one environment.  Goal: the tile's goal term is compiled in.  Strict: the call has a goal, so the
// continuation is ro_goal_step's (a compile-time switch: behind a run-time one the compiler merges the two continuations into one
// unfused multiply and add, and the call without a goal loses the FMA its rollout has).
template <bool Goal, bool Strict>
__global__ __launch_bounds__(RO_THREADS) void beam_level_kernel(const BeamArgs p, const GoalArgs gin) {
  extern __shared__ __attribute__((aligned(16))) float bm_lds[];
  __shared__ long long prow[RO_ROWS];
  __shared__ int last;
  const int tid = threadIdx.x, A = p.tile.A;
  const int n = blockIdx.x / p.tiles, c0 = (blockIdx.x - n * p.tiles) * RO_ROWS;

  if (tid < RO_ROWS) {
    long long r = n;  // (level 0: the environment's own state; a row that does not exist is never asked for)
    if (p.level > 0 && c0 + tid < p.C) {
      const int f = (c0 + tid) / A;
      r = (long long)n * p.pstride + (p.sel ? p.sel[(long long)n * p.W + f] : f);
    }
    prow[tid] = r;
  }
  __syncthreads();

  BeamRows rows{p, prow, n, c0};
  if constexpr (Goal) {
    const GoalArgs ga{gin.goal + (long long)n * gin.stride, 0, gin.w, gin.final, nullptr};
    ro_tile<BeamRows, RO_GOAL>(p.tile, bm_lds, rows, &ga);
  } else {
    ro_tile(p.tile, bm_lds, rows);
  }

  // ---- the child's ret: its parent's, continued by this step's term (the tile ended behind a barrier; thread i wrote row i's term) ----
  if (tid < RO_ROWS && c0 + tid < p.C) {
    const long long rg = rows.out(tid);
    const float val = p.has_val ? p.ret[rg] : -0.f;
    const float pr = p.level > 0 ? p.pret[prow[tid]] : 0.f;
    if constexpr (Strict) p.ret[rg] = bm_continue_goal(pr, p.g, val);
    else p.ret[rg] = bm_continue(pr, p.g, val);
  }
  if (p.finish == 0) return;

  // ---- the environment's last workgroup of the level goes on ----
  __syncthreads();  // (the returns above are issued: thread 0's fence releases them all)
  if (tid == 0) {
    __threadfence();
    last = atomicAdd(p.tickets + n, 1u) == (unsigned)p.tiles - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();

  const float* rets = p.ret + (long long)n * p.ostride;
  unsigned long long* words = (unsigned long long*)bm_lds;
  if (p.finish == 1) {
    int cpad = 1;
    while (cpad < p.C) cpad <<= 1;  // C <= 8192: at most 13 rounds
    for (int c = tid; c < cpad; c += RO_THREADS) words[c] = c < p.C ? bm_word(load_agent(rets + c), c) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= cpad; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < cpad; i += RO_THREADS) {
          const int l = i ^ j;
          if (l > i) {
            const unsigned long long a = words[i], b = words[l];
            const bool up = (i & k) == 0;
            if ((a > b) == up) { words[i] = b; words[l] = a; }
          }
        }
        __syncthreads();
      }
    }
    for (int r = tid; r < p.W; r += RO_THREADS) p.sel_out[(long long)n * p.W + r] = (int)(unsigned)(words[r] & 0xffffffffull);
    if (tid == 0) atomicExch(p.tickets + n, 0u);
    return;
  }

  // the last level: the best leaf, its plan, and the leaves when asked for
  unsigned long long m = ~0ull;
  for (int c = tid; c < p.C; c += RO_THREADS) {
    const unsigned long long w = bm_word(load_agent(rets + c), c);
    m = w < m ? w : m;
  }
  words[tid] = m;
  __syncthreads();
  for (int h = RO_THREADS >> 1; h > 0; h >>= 1) {
    if (tid < h) {
      const unsigned long long a = words[tid], b = words[tid + h];
      words[tid] = b < a ? b : a;
    }
    __syncthreads();
  }
  const int top = (int)(unsigned)(words[0] & 0xffffffffull);
  if (tid == 0) {
    bm_walk(p, n, top, p.best_plan + (long long)n * p.horizon);
    p.best_return[n] = load_agent(rets + top);  // the true return, NaN included
    atomicExch(p.tickets + n, 0u);
  }
  if (p.leaf_plans) {
    for (int c = tid; c < p.C; c += RO_THREADS) {
      bm_walk(p, n, c, p.leaf_plans + ((long long)n * p.C + c) * p.horizon);
      p.leaf_returns[(long long)n * p.C + c] = load_agent(rets + c);
    }
  }
}

// The tree's sizes: C[t] = children of level t per environment; returns L = C[T-1] (0: outside the limits).
int bm_sizes(int W, int A, int T, int* C) {
  if (W < 1 || A < 1 || T < 1 || T > BM_MAX_T || (long long)W * A > BM_MAX_C) return 0;
  int f = 1, c = 0;
  for (int t = 0; t < T; ++t) {
    c = f * A;  // f <= W: c <= 8192
    if (C) C[t] = c;
    f = c < W ? c : W;
  }
  return c;
}

int bm_supported(int S, int A, int H, int n_rewards, int has_reward, int W, int T) {
  return ro_goal_supported(S, A, H, n_rewards, has_reward) && bm_sizes(W, A, T, nullptr) > 0;
}

bool bm_rows_ok(long long N, int L) { return N >= 1 && N * L <= 0x7fffffffLL - RO_ROWS; }

// tickets [N] u32 (padded to 16 bytes), two return buffers [N,L], the frontiers [T-1,N,W], two state buffers [N,C_{T-2},S]
size_t bm_workspace(long long N, int W, int T, int S, int A) {
  int C[BM_MAX_T];
  const int L = bm_sizes(W, A, T, C);
  const size_t cs = T >= 2 ? (size_t)C[T - 2] : 0;
  return (((size_t)N + 3) & ~(size_t)3) * 4 + 2 * (size_t)N * L * 4 + (size_t)(T - 1) * N * W * 4 + 2 * (size_t)N * cs * S * 4;
}

}  // namespace

extern "C" int srlz_beam_supported(int S, int A, int H, int n_rewards, int has_reward, int W, int T) {
  return bm_supported(S, A, H, n_rewards, has_reward, W, T);
}

extern "C" int srlz_beam_leaves(int W, int A, int T) { return bm_sizes(W, A, T, nullptr); }

extern "C" size_t srlz_beam_workspace(int N, int W, int T, int S, int A) {
  const int L = bm_sizes(W, A, T, nullptr);
  if (L < 1 || S < 1 || S > RO_MAX_S || !bm_rows_ok(N, L)) return 0;
  return bm_workspace(N, W, T, S, A);
}

extern "C" int srlz_beam_search(const float* states, const float* wf, const float* bf, const float* w1, const float* b1,
                                const float* w2, const float* b2, const float* w3, const float* b3, int* best_plan,
                                float* best_return, int* leaf_plans, float* leaf_returns, void* ws, size_t ws_bytes, int N, int W,
                                int T, int S, int A, int H, int n_rewards, float gamma, const float* goal, long long goal_env_stride,
                                float goal_weight, int goal_mode, srlz_stream_t stream) {
  const int n_head = (w1 != nullptr) + (b1 != nullptr) + (w2 != nullptr) + (b2 != nullptr) + (w3 != nullptr) + (b3 != nullptr);
  SRLZ_REQUIRE(n_head == 0 || n_head == 6, SRLZ_ERR_BAD_DESC,
               "beam_search: the reward head is given whole (six pointers) or not at all, got %d of them", n_head);
  const bool reward = n_head == 6, has_goal = goal != nullptr;
  SRLZ_REQUIRE(reward || has_goal, SRLZ_ERR_BAD_DESC, "beam_search: without a goal the search scores by the reward head: all six pointers");
  SRLZ_REQUIRE(bm_supported(S, A, H, n_rewards, reward, W, T), SRLZ_ERR_BAD_DESC,
               "beam_search: S=%d A=%d H=%d n_rewards=%d W=%d T=%d outside the limits 1 <= S <= %d, 1 <= A <= %d, 1 <= H <= %d, "
               "n_rewards == 2, W >= 1, W * A <= %d, 1 <= T <= %d", S, A, H, n_rewards, W, T, RO_MAX_S, RO_MAX_A, RO_MAX_H, BM_MAX_C,
               BM_MAX_T);
  int C[BM_MAX_T];
  const int L = bm_sizes(W, A, T, C);
  SRLZ_REQUIRE(bm_rows_ok(N, L), SRLZ_ERR_BAD_DESC, "beam_search: N=%d with %d leaves each: at least one environment, N * L below 2^31 - %d",
               N, L, RO_ROWS);
  SRLZ_REQUIRE((leaf_plans != nullptr) == (leaf_returns != nullptr), SRLZ_ERR_BAD_DESC,
               "beam_search: the leaves are kept whole (leaf_plans and leaf_returns) or not at all");
  if (has_goal) {
    SRLZ_REQUIRE(isfinite(goal_weight) && goal_weight > 0.f, SRLZ_ERR_BAD_DESC, "beam_search: goal_weight=%g must be finite and > 0",
                 (double)goal_weight);
    SRLZ_REQUIRE(goal_mode == 0 || goal_mode == 1, SRLZ_ERR_BAD_DESC, "beam_search: goal_mode=%d is neither 0 (running) nor 1 (final)",
                 goal_mode);
    SRLZ_REQUIRE(goal_env_stride == 0 || goal_env_stride == (long long)S, SRLZ_ERR_BAD_DESC,
                 "beam_search: goals are [N,S] (environment stride S = %d) or one shared [S] (stride 0), got stride %lld", S,
                 goal_env_stride);
  }
  SRLZ_REQUIRE(states && wf && bf && best_plan && best_return && ws, SRLZ_ERR_NULL, "beam_search: null pointer");
  const size_t need = bm_workspace(N, W, T, S, A);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "beam_search: workspace of %zu bytes, %zu needed", ws_bytes, need);

  unsigned* tickets = (unsigned*)ws;
  float* retb[2];
  retb[0] = (float*)(tickets + (((size_t)N + 3) & ~(size_t)3));
  retb[1] = retb[0] + (size_t)N * L;
  int* sel_all = (int*)(retb[1] + (size_t)N * L);
  float* stb[2];
  const size_t cs = T >= 2 ? (size_t)C[T - 2] : 0;
  stb[0] = (float*)(sel_all + (size_t)(T - 1) * N * W);
  stb[1] = stb[0] + (size_t)N * cs * S;
  SRLZ_HIP(hipMemsetAsync(tickets, 0, (size_t)N * 4, as_stream(stream)));  // (a call cut short must not leave the next one a ticket)

  // a level's launch: which tile (the goal term enters at every level, or in mode final at the last alone), how much LDS
  size_t lds_max[3] = {0, 0, 0};  // beam_level_kernel<false, false>, <false, true>, <true, true>
  for (int t = 0; t < T; ++t) {
    const bool gk = has_goal && (goal_mode == 0 || t == T - 1);
    int cpad = 1;
    while (cpad < C[t]) cpad <<= 1;
    const size_t fin = t == T - 1 ? (size_t)RO_THREADS * 8 : C[t] > W ? (size_t)cpad * 8 : 0;
    const size_t lds = ro_lds_bytes(S, reward, gk) > fin ? ro_lds_bytes(S, reward, gk) : fin;
    const int which = gk ? 2 : has_goal ? 1 : 0;
    if (lds > lds_max[which]) lds_max[which] = lds;
  }
  if (lds_max[0]) SRLZ_MAX_LDS((beam_level_kernel<false, false>), lds_max[0]);
  if (lds_max[1]) SRLZ_MAX_LDS((beam_level_kernel<false, true>), lds_max[1]);
  if (lds_max[2]) SRLZ_MAX_LDS((beam_level_kernel<true, true>), lds_max[2]);

  unsigned pruned = 0;
  for (int t = 1; t < T; ++t)
    if (C[t - 1] > W) pruned |= 1u << t;
  const GoalArgs ga{goal, goal_env_stride, goal_weight, goal_mode, nullptr};
  float g = 1.f;
  for (int t = 0; t < T; ++t) {
    const bool lastl = t == T - 1, gk = has_goal && (goal_mode == 0 || lastl);
    const bool has_val = reward || gk;
    const int tiles = (C[t] + RO_ROWS - 1) / RO_ROWS;
    float* ret = retb[t & 1];
    const long long ostride = lastl ? L : (long long)cs, pstride = (long long)cs;
    const int finish = lastl ? 2 : C[t] > W ? 1 : 0;
    BeamArgs a{{t == 0 ? states : stb[(t - 1) & 1], wf, bf, w1, b1, w2, b2, w3, b3, lastl ? nullptr : stb[t & 1],
                has_val ? ret : nullptr, nullptr, nullptr, 1, S, A, reward ? H : 0, gamma},
               ret, t == 0 ? nullptr : retb[(t - 1) & 1], ((pruned >> t) & 1u) ? sel_all + (size_t)(t - 1) * N * W : nullptr,
               finish == 1 ? sel_all + (size_t)t * N * W : nullptr, sel_all, tickets, best_plan, best_return, leaf_plans, leaf_returns,
               pstride, ostride, pruned, N, W, C[t], tiles, t, T, g, has_val ? 1 : 0, finish};
    int cpad = 1;
    while (cpad < C[t]) cpad <<= 1;
    const size_t fin = finish == 2 ? (size_t)RO_THREADS * 8 : finish == 1 ? (size_t)cpad * 8 : 0;
    const size_t tile_lds = ro_lds_bytes(S, reward, gk);
    const size_t lds = tile_lds > fin ? tile_lds : fin;
    const dim3 grid((unsigned)(N * tiles)), block(RO_THREADS);
    if (gk) SRLZ_LAUNCH((beam_level_kernel<true, true>), grid, block, lds, as_stream(stream), a, ga);
    else if (has_goal) SRLZ_LAUNCH((beam_level_kernel<false, true>), grid, block, lds, as_stream(stream), a, ga);
    else SRLZ_LAUNCH((beam_level_kernel<false, false>), grid, block, lds, as_stream(stream), a, ga);
    g = g * gamma;
  }
  return SRLZ_OK;
}
