// plan.hip — deployment planner: a categorical cross-entropy method over discrete action sequences on the learned dynamics, ONE launch
// per iteration, no plan ever on the host.  Replaces the loop every user of LatentDynamics.act writes around srlz_rollout: sample K
// action sequences, upload, roll, download the returns, sort, refit, I times — one host round trip an iteration.
//
// Everything but the returns is integer arithmetic (include/srlz.h states the algorithm): the sampling table cum[n][t][a] (uint32) is
// the inclusive prefix sum of integer weights; the action of (iteration i, environment n, plan k, step t) is word t & 3 of
// Philox4x32-10 at counter (t >> 2, k, n, i) under the 64-bit seed, scaled by the row's total and looked up in the row.
//
// A launch.  Grid N x ceil(K / 32) workgroups of 512 threads; an environment owns whole tiles, rows past K idle.  The workgroup copies
// cum[n] to LDS (iteration 0: builds it from the caller's weights or uniform), and runs the 32-row state tile of rollout_tile.h — the
// text rollout_kernel runs — with rows whose actions are sampled by their owner thread, one step ahead, and written to the population.
// The returns are therefore the bits srlz_rollout leaves for the same plans.
// Finisher.  A workgroup that ends takes a ticket of its environment (__threadfence, atomicAdd: priors.hip's episode_prior_fwd_kernel;
// here one thread fences behind the tile's last barrier — the fence of every wave cost 25 us a launch at 256 workgroups);
// the one that takes the last does select, best-so-far and refit for that environment and resets the ticket.  No spin, no grid
// barrier.  Ranks come from counting (K^2 <= 1 M comparisons over 512 threads): a rank is unique (ties go to the lower k), so the
// elites land in their slots without atomics; the action counts are integers, added with LDS integer atomics — one value whatever
// the order.  No float atomics.  The finisher reads other workgroups' returns and plans past its own L1 (agent-scope loads).
// LDS at the limits (S = 512, H = 32, T = 32, A = 256, K = 1024): tile 114.7 KB + table 32 KB + keys and elites 8 KB = 155.7 KB of 160.
// With a goal (plan_cem_kernel<PlanGoalArgs>, srlz_plan_cem_goal): the tile's goal term compiled in, + 2.1 KB for its partials =
// 157.8 KB; the key is then the score of include/srlz.h, the reward head optional.  Everything else is the same text.
#include <math.h>
#include <type_traits>
#include "common.h"
#include "rollout_tile.h"

using namespace rollout_tile;

namespace {

constexpr int PL_MAX_A = 256;
constexpr int PL_MAX_K = 1024;
constexpr int PL_MAX_T = 32;
constexpr int PL_MAX_Q = 4096;

struct PlanArgs {
  TileArgs tile;            // (tile.returns: this iteration's [N,K])
  int* pop;                 // this iteration's plans [N,K,T]
  const unsigned* init_w;   // iteration 0: weights [N,T,A] / [T,A] (init_stride 0), NULL = uniform
  long long init_stride;
  unsigned* cum;            // [N,T,A]: read by iterations > 0, written by every finisher
  unsigned* tickets;        // [N]
  float* bestkey;           // [N]
  int* best_plan;           // [N,T]
  float* best_return;       // [N]
  int K, tiles, iter, E, Q;
  unsigned key0, key1;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// Rows of one environment's tile: row i is plan k0 + i of environment n; its actions are sampled here and written to the population.
struct SampledRows {
  const PlanArgs& p;
  const unsigned* tab;  // LDS: cum[n], [T,A]
  const int n, k0;
  int* mypop = nullptr;
  unsigned w[4] = {0, 0, 0, 0};
  __device__ __forceinline__ bool exists(int i) const { return k0 + i < p.K; }
  __device__ __forceinline__ long long env(int) const { return n; }
  __device__ __forceinline__ long long out(int i) const { return (long long)n * p.K + k0 + i; }
  __device__ __forceinline__ void begin(int i) { mypop = p.pop + out(i) * p.tile.T; }
  __device__ __forceinline__ int action(int i, int t) {
    if ((t & 3) == 0) philox4x32_10((unsigned)(t >> 2), (unsigned)(k0 + i), (unsigned)n, (unsigned)p.iter, p.key0, p.key1, w);
    const int q = t & 3;
    const unsigned u = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
    const int A = p.tile.A;
    const unsigned* row = tab + t * A;
    const unsigned target = __umulhi(u, row[A - 1]);
    int lo = 0, hi = A - 1;  // the first a with row[a] > target (row[A-1] > target for any positive total)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (row[mid] > target) hi = mid; else lo = mid + 1;
    }
    mypop[t] = lo;
    return lo;
  }
};

template <class T>
__device__ __forceinline__ T load_agent(const T* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The planner's arguments with a goal: the key is then the score with the goal term, and the reward head optional.
struct PlanGoalArgs : PlanArgs {
  GoalArgs goal;
};

// One iteration for one tile of one environment: plan_cem_kernel<PlanArgs> (srlz_plan_cem) and plan_cem_kernel<PlanGoalArgs>
// (srlz_plan_cem_goal) — sampling, tickets, select, best and refit are this one text either way; only the key's source differs.
template <class Args>
__global__ __launch_bounds__(RO_THREADS) void plan_cem_kernel(const Args p) {
  constexpr bool Goal = std::is_same<Args, PlanGoalArgs>::value;
  extern __shared__ __attribute__((aligned(16))) float pl_lds[];
  __shared__ int last;
  const int T = p.tile.T, A = p.tile.A, K = p.K, TA = T * A;
  const int tid = threadIdx.x;
  const int n = blockIdx.x / p.tiles, tile = blockIdx.x - n * p.tiles;
  unsigned* tab = (unsigned*)((char*)pl_lds + ro_lds_bytes(p.tile.S, !Goal || p.tile.w1 != nullptr, Goal));  // [T,A]; the finisher's counts afterwards
  float* keys = (float*)(tab + TA);                                             // [K]
  int* elite = (int*)(keys + K);                                                // [E]

  // ---- this environment's sampling table ----
  if (p.iter > 0) {
    const unsigned* src = p.cum + (long long)n * TA;
    for (int e = tid; e < TA; e += RO_THREADS) tab[e] = src[e];
  } else if (p.init_w) {
    const unsigned* src = p.init_w + n * p.init_stride;
    for (int t = tid; t < T; t += RO_THREADS) {
      unsigned run = 0;
      for (int a = 0; a < A; ++a) tab[t * A + a] = run += src[t * A + a];
    }
  } else {
    for (int e = tid; e < TA; e += RO_THREADS) tab[e] = (unsigned)(e % A) + 1u;
  }
  // (ro_tile's first barrier stands between these writes and the first sample — the first action is asked for before it, so:)
  __syncthreads();

  SampledRows rows{p, tab, n, tile * RO_ROWS};
  if constexpr (Goal) ro_tile<SampledRows, true>(p.tile, pl_lds, rows, &p.goal);
  else ro_tile(p.tile, pl_lds, rows);

  // ---- the environment's last workgroup to finish goes on ----
  // (ro_tile ended behind a workgroup barrier: every wave's stores happen before thread 0's fence, which releases them all)
  if (tid == 0) {
    __threadfence();
    last = atomicAdd(p.tickets + n, 1u) == (unsigned)p.tiles - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();

  const long long r0 = (long long)n * K;
  const float* rets = p.tile.returns + r0;
  const int* pop = p.pop + r0 * T;
  // select: key = the return, NaN read as -inf; rank = the plans ahead of k in (key descending, k ascending)
  for (int k = tid; k < K; k += RO_THREADS) {
    const float v = load_agent(rets + k);
    keys[k] = v != v ? -INFINITY : v;
  }
  for (int e = tid; e < TA; e += RO_THREADS) tab[e] = 0u;
  __syncthreads();
  for (int k = tid; k < K; k += RO_THREADS) {
    const float v = keys[k];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const float o = keys[j];
      rank += (o > v || (o == v && j < k)) ? 1 : 0;
    }
    if (rank < p.E) elite[rank] = k;
  }
  __syncthreads();
  // best so far, on the last wave while the others count: iteration 0 stores its top plan, a later one only a strictly greater key
  if (tid >= RO_THREADS - 64) {
    const int lane = tid & 63, top = elite[0];
    const float key = keys[top];
    const float prev = p.iter > 0 ? p.bestkey[n] : 0.f;  // (every lane reads it, in the one instruction, before lane 0 replaces it)
    if (p.iter == 0 || key > prev) {
      if (lane < T) p.best_plan[(long long)n * T + lane] = load_agent(pop + (long long)top * T + lane);  // T <= 32
      if (lane == 63) p.best_return[n] = load_agent(rets + top);  // the true return, NaN included
      if (lane == 0) p.bestkey[n] = key;
    }
    if (lane == 0) atomicExch(p.tickets + n, 0u);
  }
  // refit: count[t][a] over the elites, w = 1 + Q * count, cum = its prefix sum
  for (int e = tid; e < p.E * T; e += RO_THREADS) {
    const int el = e / T, t = e - el * T;
    const int a = load_agent(pop + (long long)elite[el] * T + t);
    atomicAdd(tab + t * A + a, 1u);
  }
  __syncthreads();
  unsigned* dst = p.cum + (long long)n * TA;
  for (int t = tid; t < T; t += RO_THREADS) {
    unsigned run = 0;
    for (int a = 0; a < A; ++a) dst[t * A + a] = run += 1u + (unsigned)p.Q * tab[t * A + a];
  }
}

// LDS of a launch: the tile, the table [T,A], keys [K] and elites (at most K)
size_t pl_lds_bytes(int S, bool reward, bool goal, int K, int T, int A) {
  return ro_lds_bytes(S, reward, goal) + ((size_t)T * A + 2 * (size_t)K) * 4;
}

int pl_supported(int S, int A, int H, int n_rewards, int K, int T) {
  return ro_supported(S, A, H, n_rewards) && A <= PL_MAX_A && K >= 1 && K <= PL_MAX_K && T >= 1 && T <= PL_MAX_T;
}

// tickets [N] u32, best keys [N] f32, then (no population kept) one iteration's returns [N,K] f32 and plans [N,K,T] i32
size_t pl_workspace(long long N, int K, int T, bool keep) {
  size_t b = (size_t)N * 8;
  if (!keep) b += (size_t)N * K * 4 + (size_t)N * K * T * 4;
  return b;
}

// With the goal term: the tile's own answer, the planner's limits, and the whole launch (+ the ticket flag) inside the CU's LDS.
int pl_goal_supported(int S, int A, int H, int n_rewards, int has_reward, int K, int T) {
  return ro_goal_supported(S, A, H, n_rewards, has_reward) && A <= PL_MAX_A && K >= 1 && K <= PL_MAX_K && T >= 1 && T <= PL_MAX_T &&
         pl_lds_bytes(S, has_reward != 0, true, K, T, A) + 16 <= RO_LDS_CAP;
}

bool pl_rows_ok(int N, int K) { return N >= 1 && K >= 1 && K <= PL_MAX_K && (long long)N * K <= 0x7fffffffLL - RO_ROWS; }

}  // namespace

extern "C" int srlz_plan_supported(int S, int A, int H, int n_rewards, int K, int T) { return pl_supported(S, A, H, n_rewards, K, T); }

extern "C" size_t srlz_plan_workspace(int N, int K, int T, int keep_population) {
  if (!pl_rows_ok(N, K) || T < 1 || T > PL_MAX_T) return 0;
  return pl_workspace(N, K, T, keep_population != 0);
}

extern "C" int srlz_plan_cem(const float* states, const float* wf, const float* bf, const float* w1, const float* b1, const float* w2,
                             const float* b2, const float* w3, const float* b3, const unsigned* init_weights,
                             long long init_env_stride, int* best_plan, float* best_return, unsigned* cum, int* plans, float* returns,
                             void* ws, size_t ws_bytes, int N, int K, int T, int S, int A, int H, int n_rewards, int iterations,
                             int elites, int sharpness, float gamma, unsigned long long seed, srlz_stream_t stream) {
  SRLZ_REQUIRE(w1 && b1 && w2 && b2 && w3 && b3, SRLZ_ERR_BAD_DESC, "plan_cem: the planner scores by the reward head: all six pointers");
  SRLZ_REQUIRE(pl_supported(S, A, H, n_rewards, K, T), SRLZ_ERR_BAD_DESC,
               "plan_cem: S=%d A=%d H=%d n_rewards=%d K=%d T=%d outside the limits 1 <= S <= %d, 1 <= A <= %d, 1 <= H <= %d, "
               "n_rewards == 2, 1 <= K <= %d, 1 <= T <= %d", S, A, H, n_rewards, K, T, RO_MAX_S, PL_MAX_A, RO_MAX_H, PL_MAX_K, PL_MAX_T);
  SRLZ_REQUIRE(pl_rows_ok(N, K), SRLZ_ERR_BAD_DESC, "plan_cem: N=%d K=%d: at least one environment, N * K below 2^31 - %d", N, K, RO_ROWS);
  SRLZ_REQUIRE(iterations >= 1 && elites >= 1 && elites <= K && sharpness >= 0 && sharpness <= PL_MAX_Q, SRLZ_ERR_BAD_DESC,
               "plan_cem: iterations=%d (>= 1), elites=%d (1 .. K = %d), sharpness=%d (0 .. %d)", iterations, elites, K, sharpness,
               PL_MAX_Q);
  SRLZ_REQUIRE(init_env_stride == 0 || init_env_stride == (long long)T * A, SRLZ_ERR_BAD_DESC,
               "plan_cem: init_weights are [N,T,A] (environment stride T * A = %lld) or shared [T,A] (stride 0), got stride %lld",
               (long long)T * A, init_env_stride);
  SRLZ_REQUIRE((plans != nullptr) == (returns != nullptr), SRLZ_ERR_BAD_DESC,
               "plan_cem: the population is kept whole (plans and returns) or not at all");
  const int tiles = (K + RO_ROWS - 1) / RO_ROWS;
  SRLZ_REQUIRE((long long)N * tiles <= 0x7fffffffLL && (long long)N * K * T * (plans ? iterations : 1) <= (1LL << 40), SRLZ_ERR_BAD_DESC,
               "plan_cem: N=%d K=%d T=%d iterations=%d: too many workgroups or a population beyond 2^40 actions", N, K, T, iterations);
  SRLZ_REQUIRE(states && wf && bf && best_plan && best_return && cum && ws, SRLZ_ERR_NULL, "plan_cem: null pointer");
  const bool keep = plans != nullptr;
  const size_t need = pl_workspace(N, K, T, keep);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "plan_cem: workspace of %zu bytes, %zu needed", ws_bytes, need);

  unsigned* tickets = (unsigned*)ws;
  float* bestkey = (float*)(tickets + N);
  float* ws_ret = bestkey + N;
  int* ws_pop = (int*)(ws_ret + (size_t)N * K);
  SRLZ_HIP(hipMemsetAsync(tickets, 0, (size_t)N * 4, as_stream(stream)));  // (a call cut short must not leave the next one a ticket)
  const size_t lds = ro_lds_bytes(S, true) + ((size_t)T * A + 2 * (size_t)K) * 4;
  SRLZ_MAX_LDS(plan_cem_kernel<PlanArgs>, lds);
  for (int i = 0; i < iterations; ++i) {
    PlanArgs a{{states, wf, bf, w1, b1, w2, b2, w3, b3, nullptr, keep ? returns + (size_t)i * N * K : ws_ret, nullptr, nullptr, T, S, A, H,
                gamma},
               keep ? plans + (size_t)i * N * K * T : ws_pop, init_weights, init_env_stride, cum, tickets, bestkey, best_plan,
               best_return, K, tiles, i, elites, sharpness, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32)};
    SRLZ_LAUNCH(plan_cem_kernel<PlanArgs>, dim3((unsigned)(N * tiles)), dim3(RO_THREADS), lds, as_stream(stream), a);
  }
  return SRLZ_OK;
}

// ---- the same planner keyed by the score with the goal term (include/srlz.h states the rule); the reward head is optional ----
extern "C" int srlz_plan_goal_supported(int S, int A, int H, int n_rewards, int has_reward, int K, int T) {
  return pl_goal_supported(S, A, H, n_rewards, has_reward, K, T);
}

extern "C" size_t srlz_plan_goal_workspace(int N, int K, int T, int keep_population) {
  return srlz_plan_workspace(N, K, T, keep_population);
}

extern "C" int srlz_plan_cem_goal(const float* states, const float* wf, const float* bf, const float* w1, const float* b1,
                                  const float* w2, const float* b2, const float* w3, const float* b3, const unsigned* init_weights,
                                  long long init_env_stride, int* best_plan, float* best_return, unsigned* cum, int* plans,
                                  float* returns, void* ws, size_t ws_bytes, int N, int K, int T, int S, int A, int H, int n_rewards,
                                  int iterations, int elites, int sharpness, float gamma, unsigned long long seed, const float* goal,
                                  long long goal_env_stride, float goal_weight, int goal_mode, srlz_stream_t stream) {
  const int n_head = (w1 != nullptr) + (b1 != nullptr) + (w2 != nullptr) + (b2 != nullptr) + (w3 != nullptr) + (b3 != nullptr);
  SRLZ_REQUIRE(n_head == 0 || n_head == 6, SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: the reward head is given whole (six pointers) or not at all, got %d of them", n_head);
  const bool reward = n_head == 6;
  SRLZ_REQUIRE(pl_goal_supported(S, A, H, n_rewards, reward, K, T), SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: S=%d A=%d H=%d n_rewards=%d K=%d T=%d outside the limits 1 <= S <= %d, 1 <= A <= %d, 1 <= H <= %d, "
               "n_rewards == 2, 1 <= K <= %d, 1 <= T <= %d", S, A, H, n_rewards, K, T, RO_MAX_S, PL_MAX_A, RO_MAX_H, PL_MAX_K, PL_MAX_T);
  SRLZ_REQUIRE(pl_rows_ok(N, K), SRLZ_ERR_BAD_DESC, "plan_cem_goal: N=%d K=%d: at least one environment, N * K below 2^31 - %d", N, K,
               RO_ROWS);
  SRLZ_REQUIRE(iterations >= 1 && elites >= 1 && elites <= K && sharpness >= 0 && sharpness <= PL_MAX_Q, SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: iterations=%d (>= 1), elites=%d (1 .. K = %d), sharpness=%d (0 .. %d)", iterations, elites, K, sharpness,
               PL_MAX_Q);
  SRLZ_REQUIRE(init_env_stride == 0 || init_env_stride == (long long)T * A, SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: init_weights are [N,T,A] (environment stride T * A = %lld) or shared [T,A] (stride 0), got stride %lld",
               (long long)T * A, init_env_stride);
  SRLZ_REQUIRE((plans != nullptr) == (returns != nullptr), SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: the population is kept whole (plans and returns) or not at all");
  SRLZ_REQUIRE(isfinite(goal_weight) && goal_weight > 0.f, SRLZ_ERR_BAD_DESC, "plan_cem_goal: goal_weight=%g must be finite and > 0",
               (double)goal_weight);
  SRLZ_REQUIRE(goal_mode == 0 || goal_mode == 1, SRLZ_ERR_BAD_DESC, "plan_cem_goal: goal_mode=%d is neither 0 (running) nor 1 (final)",
               goal_mode);
  SRLZ_REQUIRE(goal_env_stride == 0 || goal_env_stride == (long long)S, SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: goals are [N,S] (environment stride S = %d) or one shared [S] (stride 0), got stride %lld", S,
               goal_env_stride);
  const int tiles = (K + RO_ROWS - 1) / RO_ROWS;
  SRLZ_REQUIRE((long long)N * tiles <= 0x7fffffffLL && (long long)N * K * T * (plans ? iterations : 1) <= (1LL << 40), SRLZ_ERR_BAD_DESC,
               "plan_cem_goal: N=%d K=%d T=%d iterations=%d: too many workgroups or a population beyond 2^40 actions", N, K, T,
               iterations);
  SRLZ_REQUIRE(states && wf && bf && best_plan && best_return && cum && ws && goal, SRLZ_ERR_NULL, "plan_cem_goal: null pointer");
  const bool keep = plans != nullptr;
  const size_t need = pl_workspace(N, K, T, keep);
  SRLZ_REQUIRE(ws_bytes >= need, SRLZ_ERR_WORKSPACE, "plan_cem_goal: workspace of %zu bytes, %zu needed", ws_bytes, need);

  unsigned* tickets = (unsigned*)ws;
  float* bestkey = (float*)(tickets + N);
  float* ws_ret = bestkey + N;
  int* ws_pop = (int*)(ws_ret + (size_t)N * K);
  SRLZ_HIP(hipMemsetAsync(tickets, 0, (size_t)N * 4, as_stream(stream)));
  const size_t lds = pl_lds_bytes(S, reward, true, K, T, A);
  SRLZ_MAX_LDS(plan_cem_kernel<PlanGoalArgs>, lds);
  for (int i = 0; i < iterations; ++i) {
    PlanGoalArgs a{{{states, wf, bf, w1, b1, w2, b2, w3, b3, nullptr, keep ? returns + (size_t)i * N * K : ws_ret, nullptr, nullptr, T, S, A,
                     reward ? H : 0, gamma},
                    keep ? plans + (size_t)i * N * K * T : ws_pop, init_weights, init_env_stride, cum, tickets, bestkey, best_plan,
                    best_return, K, tiles, i, elites, sharpness, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32)},
                   {goal, goal_env_stride, goal_weight, goal_mode, nullptr}};
    SRLZ_LAUNCH(plan_cem_kernel<PlanGoalArgs>, dim3((unsigned)(N * tiles)), dim3(RO_THREADS), lds, as_stream(stream), a);
  }
  return SRLZ_OK;
}
