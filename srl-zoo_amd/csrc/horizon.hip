// horizon.hip — the k-step error of the latent dynamics on a recorded sequence (evaluation/predict_forward.py): from every start frame
// the recorded actions go through forwardModel (and the imagined pairs through rewardModel), and the imagined state after t + 1 steps
// is compared with the recorded one — models/forward_inverse.py:21-31, 78-95 composed open loop.
//
// horizon_rows_kernel: the state tile of rollout_tile.h (the text rollout.hip and plan.hip run) with a third row source and the
// tile's third mode.  A workgroup owns 32 starts for all T steps; row r starts from states[starts[r]], takes actions[starts[r] + t]
// while t < len[r] (action 0 afterwards: the tile rolls on, nothing of it is reported), and once s_{t+1} is in the tile
//   err[r,t]  = sum_j fl(s_{t+1}[j] - states[starts[r] + t + 1][j])^2,   base[r,t] = sum_j fl(states[starts[r]][j] - the same)^2
// in the goal term's order (16 column groups a row, an fma chain over ascending j, the partials added in group order), NaN for
// t >= len[r].  Nothing but err, base and the optional logits / trajectory leaves the chip: M * T * S floats of imagined states are
// never written.  The target rows of neighbouring starts overlap, so the states are read from HBM about once.  LDS: the tile of
// ro_lds_bytes plus 2 x 16 x 33 partials (4.2 KB): 119 KB of 160 at S = 512, H = 32.  No atomics.
//
// horizon_sums_kernel: [M,T] rows to per-horizon totals, one workgroup per horizon t, fp64.  Thread k of 512 adds its rows
// r = k, k + 512, .. in ascending order (rows with len[r] <= t are skipped), then the 512 partials fold in halves:
// p[k] += p[k + h] for h = 256, 128, .. 1.  A function of (M, T) alone; integer counts; no atomics.
#include <math.h>
#include "common.h"
#include "rollout_tile.h"

using namespace rollout_tile;

namespace {

constexpr int HZ_MAX_T = 32;
constexpr int HZ_SUM_THREADS = 512;

struct HorizonArgs {
  TileArgs tile;
  const int* actions;  // [N]
  const int* starts;   // [M]
  const int* len;      // [M]
  int M;
};

// Rows of a recorded sequence: tile row i is start r = row0 + i of the call's M.
struct RecordedRows {
  const HorizonArgs& p;
  const long long row0;
  const int* myact = nullptr;  // threads 0..31: the recorded actions from row tid's start on
  int mylen = 0;
  __device__ __forceinline__ bool exists(int i) const { return (unsigned)row0 + i < (unsigned)p.M; }  // (M + 32 fits 31 bits: the launcher checks)
  __device__ __forceinline__ long long env(int i) const { return p.starts[row0 + i]; }
  __device__ __forceinline__ long long out(int i) const { return row0 + i; }
  __device__ __forceinline__ long long target(int i, int t) const {
    return t < p.len[row0 + i] ? (long long)p.starts[row0 + i] + t + 1 : -1;
  }
  __device__ __forceinline__ void begin(int i) {
    myact = p.actions + p.starts[row0 + i];
    mylen = p.len[row0 + i];
  }
  __device__ __forceinline__ int action(int, int t) const { return t < mylen ? myact[t] : 0; }
};

__global__ __launch_bounds__(RO_THREADS) void horizon_rows_kernel(const HorizonArgs p, const TrackArgs k) {
  extern __shared__ __attribute__((aligned(16))) float hz_lds[];
  RecordedRows rows{p, (long long)blockIdx.x * RO_ROWS};
  ro_tile<RecordedRows, RO_TRACK>(p.tile, hz_lds, rows, nullptr, &k);
}

struct SumsArgs {
  const float *err, *base, *logits;  // [M,T], [M,T], [M,T,2] or NULL
  const int *labels, *starts, *len;  // [N] or NULL, [M], [M]
  long long* count;                  // [T]
  double *sum_err, *sum_base;        // [T]
  long long* hits;                   // [T] or NULL
  int M, T;
};

__global__ __launch_bounds__(HZ_SUM_THREADS) void horizon_sums_kernel(const SumsArgs p) {
  __shared__ double se[HZ_SUM_THREADS], sb[HZ_SUM_THREADS];
  __shared__ int sc[HZ_SUM_THREADS], sh[HZ_SUM_THREADS];
  const int t = blockIdx.x, k = threadIdx.x, T = p.T;
  double e = 0.0, b = 0.0;
  int c = 0, h = 0;
  for (int r = k; r < p.M; r += HZ_SUM_THREADS) {
    if (p.len[r] <= t) continue;
    const size_t o = (size_t)r * T + t;
    e += (double)p.err[o];
    b += (double)p.base[o];
    ++c;
    if (p.logits) {
      const int cls = p.logits[2 * o + 1] > p.logits[2 * o] ? 1 : 0;  // argmax as torch takes it: a tie or a NaN is class 0
      h += cls == p.labels[(long long)p.starts[r] + t];
    }
  }
  se[k] = e; sb[k] = b; sc[k] = c; sh[k] = h;
  __syncthreads();
  for (int half = HZ_SUM_THREADS / 2; half >= 1; half >>= 1) {
    if (k < half) {
      se[k] += se[k + half];
      sb[k] += sb[k + half];
      sc[k] += sc[k + half];
      sh[k] += sh[k + half];
    }
    __syncthreads();
  }
  if (k == 0) {
    p.count[t] = sc[0];
    p.sum_err[t] = se[0];
    p.sum_base[t] = sb[0];
    if (p.hits) p.hits[t] = sh[0];
  }
}

}  // namespace

extern "C" int srlz_horizon_supported(int S, int A, int H, int n_rewards, int has_reward) {
  return ro_track_supported(S, A, H, n_rewards, has_reward);
}

extern "C" int srlz_horizon_rows(const float* states, const int* actions, const int* starts, const int* len, const float* wf,
                                 const float* bf, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                 const float* b3, float* err, float* base, float* reward_logits, float* trajectory, int N, int M, int T,
                                 int S, int A, int H, int n_rewards, srlz_stream_t stream) {
  const int n_head = (w1 != nullptr) + (b1 != nullptr) + (w2 != nullptr) + (b2 != nullptr) + (w3 != nullptr) + (b3 != nullptr);
  SRLZ_REQUIRE(n_head == 0 || n_head == 6, SRLZ_ERR_BAD_DESC,
               "horizon_rows: the reward head is given whole (six pointers) or not at all, got %d of them", n_head);
  const bool reward = n_head == 6;
  SRLZ_REQUIRE(ro_track_supported(S, A, H, n_rewards, reward), SRLZ_ERR_BAD_DESC,
               "horizon_rows: S=%d A=%d H=%d n_rewards=%d outside the limits 1 <= S <= %d, 1 <= A <= %d, 1 <= H <= %d, n_rewards == 2", S,
               A, H, n_rewards, RO_MAX_S, RO_MAX_A, RO_MAX_H);
  SRLZ_REQUIRE(N >= 1 && M >= 1 && M <= 0x7fffffff - RO_ROWS && T >= 1 && T <= HZ_MAX_T, SRLZ_ERR_BAD_DESC,
               "horizon_rows: N=%d M=%d T=%d: at least one frame and one start, M below 2^31 - %d, 1 <= T <= %d", N, M, T, RO_ROWS,
               HZ_MAX_T);
  SRLZ_REQUIRE(reward || !reward_logits, SRLZ_ERR_BAD_DESC, "horizon_rows: reward_logits asked for without a reward head");
  SRLZ_REQUIRE(states && actions && starts && len && wf && bf && err && base, SRLZ_ERR_NULL, "horizon_rows: null pointer");
  HorizonArgs a{{states, wf, bf, w1, b1, w2, b2, w3, b3, nullptr, nullptr, trajectory, reward_logits, T, S, A, reward ? H : 0, 1.f},
                actions, starts, len, M};
  TrackArgs k{err, base};
  const size_t lds = ro_track_lds_bytes(S, reward);
  SRLZ_MAX_LDS(horizon_rows_kernel, lds);
  SRLZ_LAUNCH(horizon_rows_kernel, dim3((unsigned)((M + RO_ROWS - 1) / RO_ROWS)), dim3(RO_THREADS), lds, as_stream(stream), a, k);
  return SRLZ_OK;
}

extern "C" int srlz_horizon_sums(const float* err, const float* base, const float* reward_logits, const int* labels, const int* starts,
                                 const int* len, int M, int T, long long* count, double* sum_err, double* sum_base, long long* hits,
                                 srlz_stream_t stream) {
  const int n_hit = (reward_logits != nullptr) + (labels != nullptr) + (hits != nullptr);
  SRLZ_REQUIRE(n_hit == 0 || n_hit == 3, SRLZ_ERR_BAD_DESC,
               "horizon_sums: reward_logits, labels and hits are given together or not at all, got %d of them", n_hit);
  SRLZ_REQUIRE(M >= 1 && T >= 1 && T <= HZ_MAX_T, SRLZ_ERR_BAD_DESC, "horizon_sums: M=%d T=%d: at least one row, 1 <= T <= %d", M, T,
               HZ_MAX_T);
  SRLZ_REQUIRE(err && base && starts && len && count && sum_err && sum_base, SRLZ_ERR_NULL, "horizon_sums: null pointer");
  SumsArgs a{err, base, reward_logits, labels, starts, len, count, sum_err, sum_base, hits, M, T};
  SRLZ_LAUNCH(horizon_sums_kernel, dim3((unsigned)T), dim3(HZ_SUM_THREADS), 0, as_stream(stream), a);
  return SRLZ_OK;
}
