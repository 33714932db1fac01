// rollout.hip — deployment dynamics: R = N*K rows (environment n, candidate plan k) rolled T steps through forwardModel and
// rewardModel in ONE launch.  Replaces, per step and row, the reference's models/forward_inverse.py:21-31 (forwardModel:
// state + Linear([state ; onehot(action)])) and :78-95 (rewardModel: Linear-ReLU-Linear-ReLU-Linear on [state ; next_state]), which the
// training kernels run as srlz_concat_onehot + srlz_linear_fwd_res and srlz_cat_cols + 3 x srlz_linear_fwd: six launches a step.
//
// Tiling.  A workgroup (512 threads, 8 waves) owns 32 rows for all T steps.  The state tile lives in LDS as st[k][row] (row stride
// 33 floats: the MFMA operand reads walk rows, the epilogue's writes walk k, both conflict-free) from step 0 to step T-1; nothing
// but the optional trajectory / logits is written per step.
//   forward model : D[32 x S] = st[32 x S] . Wf[:, :S]^T as v_mfma_f32_32x32x2_f32 blocks of 32 output columns, block b on wave b & 7
//                   (at most 2 blocks = 32 accumulator registers a wave at S = 512).  The B operand is read from Wf in place (L2: the
//                   matrix is at most ~1 MB and every workgroup walks it once a step): a lane's share of a chunk of 32 k is 64
//                   contiguous bytes of its row, four 16-byte loads, requested one chunk of 16 MFMAs ahead (ro_gemm).  The one-hot
//                   never exists: column Wf[:, S + a] is requested before the block's k-loop and added behind it.
//                   d = fl(fl(acc + Wf[j][S+a]) + bf[j]);  s' = fl(s + d).
//   reward layer 1: [s ; s'] . W1^T on the same MFMA, H <= 32 outputs in one block, the 2S-long sum cut into chunks of 32 k; wave w
//                   takes chunks w, w+8, .. of the s half (before the tile is overwritten) and of the s' half (after), and the eight
//                   partial blocks are added in wave order (((p0 + p1) + p2) + ..) + p7, then + b1.
//   layers 2, 3   : fmaf chains in index order on the vector pipe (H*H and 2*H products a row), softmax(l)[1] = 1 / (1 + exp(l0 - l1)).
// Every sum's order depends on (S, A, H) alone — not on the row's place in the launch, its neighbours, N, K or T.  No atomics.
//
// On-chip budget at the limits (S = 512, H = 32): state tile 512 * 33 * 4 = 67.6 KB, partial blocks 8 * 32 * 33 * 4 = 33.8 KB,
// hidden activations 2 * 32 * 33 * 4 = 8.4 KB, W2 / W3 / biases 4.6 KB, row records 0.3 KB: 115 KB of the CU's 160 KB.  A second
// state tile (S = 1024) does not fit next to that, and H = 64 would be a second MFMA block and twice the partial blocks.
// 166 VGPRs, no scratch (tools/kres.py): three waves a SIMD by registers, one workgroup a CU by LDS at S = 512, three at S = 200.
// The tile itself (ro_gemm, the step loop, the reward head) is rollout_tile.h, shared with plan.hip; this file is the rows whose
// actions come from the caller's plans, and the launchers.
// rollout_goal_kernel (srlz_rollout_goal) is the same tile with its goal term compiled in: per step one more reduction over the state
// tile — |s_{t+1} - goal|^2, 16 partials a row in 2.1 KB of LDS — joins the score; 186 VGPRs, no scratch.  rollout_kernel itself is,
// instruction for instruction, what it was without that switch.
#include <math.h>
#include "common.h"
#include "rollout_tile.h"

using namespace rollout_tile;

namespace {

struct RolloutArgs {
  TileArgs tile;
  const int* plans;      // [N,K,T] or [K,T] with env_stride 0
  long long env_stride;  // ints between two environments' plans
  int R, K;
};

// Rows of a caller's plans: tile row i is row r = row0 + i of the call's R = N * K, environment r / K, plan r % K.
struct PlanRows {
  const RolloutArgs& p;
  const long long row0;
  const int* myplan = nullptr;  // threads 0..31: row tid's plan
  __device__ __forceinline__ bool exists(int i) const { return (unsigned)row0 + i < (unsigned)p.R; }  // (R + 32 fits 31 bits: the launcher checks)
  __device__ __forceinline__ long long env(int i) const { return (long long)(((unsigned)row0 + i) / (unsigned)p.K); }
  __device__ __forceinline__ long long out(int i) const { return row0 + i; }
  __device__ __forceinline__ void begin(int i) {
    const long long r = row0 + i;
    myplan = p.plans + (r / p.K) * p.env_stride + (r % p.K) * (long long)p.tile.T;
  }
  __device__ __forceinline__ int action(int, int t) const { return myplan[t]; }
};

__global__ __launch_bounds__(RO_THREADS) void rollout_kernel(const RolloutArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ro_lds[];
  PlanRows rows{p, (long long)blockIdx.x * RO_ROWS};
  ro_tile(p.tile, ro_lds, rows);
}

// The same rows with the goal term of the score compiled in (rollout_tile.h, Goal = true).
__global__ __launch_bounds__(RO_THREADS) void rollout_goal_kernel(const RolloutArgs p, const GoalArgs g) {
  extern __shared__ __attribute__((aligned(16))) float ro_lds[];
  PlanRows rows{p, (long long)blockIdx.x * RO_ROWS};
  ro_tile<PlanRows, true>(p.tile, ro_lds, rows, &g);
}

}  // namespace

extern "C" int srlz_rollout_supported(int S, int A, int H, int n_rewards) { return ro_supported(S, A, H, n_rewards); }

extern "C" int srlz_rollout_tile(void) { return RO_ROWS; }

extern "C" int srlz_rollout(const float* states, const int* plans, long long plan_env_stride, const float* wf, const float* bf,
                            const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                            float* final_states, float* returns, float* trajectory, float* reward_logits, int N, int K, int T, int S,
                            int A, int H, int n_rewards, float gamma, srlz_stream_t stream) {
  const int n_head = (w1 != nullptr) + (b1 != nullptr) + (w2 != nullptr) + (b2 != nullptr) + (w3 != nullptr) + (b3 != nullptr);
  SRLZ_REQUIRE(n_head == 0 || n_head == 6, SRLZ_ERR_BAD_DESC,
               "rollout: the reward head is given whole (six pointers) or not at all, got %d of them", n_head);
  const bool reward = n_head == 6;
  SRLZ_REQUIRE(ro_supported(S, A, reward ? H : 1, reward ? n_rewards : 2), SRLZ_ERR_BAD_DESC,
               "rollout: S=%d A=%d H=%d n_rewards=%d outside the limits 1 <= S <= %d, 1 <= A <= %d, 1 <= H <= %d, n_rewards == 2", S, A,
               H, n_rewards, RO_MAX_S, RO_MAX_A, RO_MAX_H);
  SRLZ_REQUIRE(N >= 1 && K >= 1 && T >= 1 && (long long)N * K <= 0x7fffffffLL - RO_ROWS, SRLZ_ERR_BAD_DESC,
               "rollout: N=%d K=%d T=%d: at least one row and one step, N * K below 2^31 - %d", N, K, T, RO_ROWS);
  SRLZ_REQUIRE(plan_env_stride == 0 || plan_env_stride == (long long)K * T, SRLZ_ERR_BAD_DESC,
               "rollout: plans are [N,K,T] (environment stride K * T = %lld) or shared [K,T] (stride 0), got stride %lld",
               (long long)K * T, plan_env_stride);
  SRLZ_REQUIRE(reward || (!returns && !reward_logits), SRLZ_ERR_BAD_DESC,
               "rollout: returns / reward_logits asked for without a reward head");
  SRLZ_REQUIRE(states && plans && wf && bf && final_states, SRLZ_ERR_NULL, "rollout: null pointer");
  const int R = N * K;
  RolloutArgs a{{states, wf, bf, w1, b1, w2, b2, w3, b3, final_states, returns, trajectory, reward_logits, T, S, A, reward ? H : 0, gamma},
                plans, plan_env_stride, R, K};
  const size_t lds = ro_lds_bytes(S, reward);
  SRLZ_MAX_LDS(rollout_kernel, lds);
  SRLZ_LAUNCH(rollout_kernel, dim3((unsigned)((R + RO_ROWS - 1) / RO_ROWS)), dim3(RO_THREADS), lds, as_stream(stream), a);
  return SRLZ_OK;
}

// ---- the same launch with the goal-distance term in the score (include/srlz.h states the rule) ----
extern "C" int srlz_rollout_goal_supported(int S, int A, int H, int n_rewards, int has_reward) {
  return ro_goal_supported(S, A, H, n_rewards, has_reward);
}

extern "C" int srlz_rollout_goal(const float* states, const int* plans, long long plan_env_stride, const float* wf, const float* bf,
                                 const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                                 float* final_states, float* returns, float* trajectory, float* reward_logits, int N, int K, int T,
                                 int S, int A, int H, int n_rewards, float gamma, const float* goal, long long goal_env_stride,
                                 float goal_weight, int goal_mode, float* goal_dist, srlz_stream_t stream) {
  const int n_head = (w1 != nullptr) + (b1 != nullptr) + (w2 != nullptr) + (b2 != nullptr) + (w3 != nullptr) + (b3 != nullptr);
  SRLZ_REQUIRE(n_head == 0 || n_head == 6, SRLZ_ERR_BAD_DESC,
               "rollout_goal: the reward head is given whole (six pointers) or not at all, got %d of them", n_head);
  const bool reward = n_head == 6;
  SRLZ_REQUIRE(ro_goal_supported(S, A, H, n_rewards, reward), SRLZ_ERR_BAD_DESC,
               "rollout_goal: S=%d A=%d H=%d n_rewards=%d outside the limits 1 <= S <= %d, 1 <= A <= %d, 1 <= H <= %d, n_rewards == 2",
               S, A, H, n_rewards, RO_MAX_S, RO_MAX_A, RO_MAX_H);
  SRLZ_REQUIRE(N >= 1 && K >= 1 && T >= 1 && (long long)N * K <= 0x7fffffffLL - RO_ROWS, SRLZ_ERR_BAD_DESC,
               "rollout_goal: N=%d K=%d T=%d: at least one row and one step, N * K below 2^31 - %d", N, K, T, RO_ROWS);
  SRLZ_REQUIRE(plan_env_stride == 0 || plan_env_stride == (long long)K * T, SRLZ_ERR_BAD_DESC,
               "rollout_goal: plans are [N,K,T] (environment stride K * T = %lld) or shared [K,T] (stride 0), got stride %lld",
               (long long)K * T, plan_env_stride);
  SRLZ_REQUIRE(reward || !reward_logits, SRLZ_ERR_BAD_DESC, "rollout_goal: reward_logits asked for without a reward head");
  SRLZ_REQUIRE(isfinite(goal_weight) && goal_weight > 0.f, SRLZ_ERR_BAD_DESC, "rollout_goal: goal_weight=%g must be finite and > 0",
               (double)goal_weight);
  SRLZ_REQUIRE(goal_mode == 0 || goal_mode == 1, SRLZ_ERR_BAD_DESC, "rollout_goal: goal_mode=%d is neither 0 (running) nor 1 (final)",
               goal_mode);
  SRLZ_REQUIRE(goal_env_stride == 0 || goal_env_stride == (long long)S, SRLZ_ERR_BAD_DESC,
               "rollout_goal: goals are [N,S] (environment stride S = %d) or one shared [S] (stride 0), got stride %lld", S,
               goal_env_stride);
  SRLZ_REQUIRE(states && plans && wf && bf && final_states && goal, SRLZ_ERR_NULL, "rollout_goal: null pointer");
  const int R = N * K;
  RolloutArgs a{{states, wf, bf, w1, b1, w2, b2, w3, b3, final_states, returns, trajectory, reward_logits, T, S, A, reward ? H : 0, gamma},
                plans, plan_env_stride, R, K};
  GoalArgs ga{goal, goal_env_stride, goal_weight, goal_mode, goal_dist};
  const size_t lds = ro_lds_bytes(S, reward, true);
  SRLZ_MAX_LDS(rollout_goal_kernel, lds);
  SRLZ_LAUNCH(rollout_goal_kernel, dim3((unsigned)((R + RO_ROWS - 1) / RO_ROWS)), dim3(RO_THREADS), lds, as_stream(stream), a, ga);
  return SRLZ_OK;
}
