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
#include <math.h>
#include "common.h"

namespace {

constexpr int RO_ROWS = 32;     // rows a workgroup owns
constexpr int RO_LD = 33;       // floats between two k of the state tile / two rows of the small tiles
constexpr int RO_MAX_S = 512;
constexpr int RO_MAX_H = 32;
constexpr int RO_MAX_A = 65536;
constexpr int RO_WAVES = 8;
constexpr int RO_THREADS = 64 * RO_WAVES;
constexpr int RO_KC = 32;       // k of a chunk: the B-operand loads in flight ahead of its 16 MFMAs

struct RolloutArgs {
  const float* states;   // [N,S]
  const int* plans;      // [N,K,T] or [K,T] with env_stride 0
  long long env_stride;  // ints between two environments' plans
  const float *wf, *bf;  // [S,S+A], [S]
  const float *w1, *b1, *w2, *b2, *w3, *b3;  // [H,2S],[H],[H,H],[H],[2,H],[2]; w1 == NULL: no reward head
  float *final_states, *returns, *trajectory, *logits;
  int R, K, T, S, A, H;
  float gamma;
};

__host__ __device__ inline int ro_sp(int S) { return (S + RO_KC - 1) & ~(RO_KC - 1); }  // the tile's k, whole chunks

// floats of LDS: state tile, 8 partial blocks, h1, h2, W2, W3, b1, b2, b3 (+2 pad), then 2 * 32 ints
__host__ __device__ inline size_t ro_lds_bytes(int S, bool reward) {
  size_t fl = (size_t)ro_sp(S) * RO_LD;
  if (reward) fl += RO_WAVES * RO_ROWS * RO_LD + 2 * RO_ROWS * RO_LD + RO_MAX_H * RO_MAX_H + 2 * RO_MAX_H + 2 * RO_MAX_H + 4;
  return (fl + 2 * RO_ROWS) * 4;
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

__global__ __launch_bounds__(RO_THREADS) void rollout_kernel(const RolloutArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ro_lds[];
  const int S = p.S, A = p.A, H = p.H, T = p.T;
  const bool reward = p.w1 != nullptr;
  const int sp = ro_sp(S), nblk = (S + 31) >> 5;
  float* st = ro_lds;
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
  int* act = (int*)fp;        // this step's action of each row, -1 = outside [0, A)
  int* bad = act + RO_ROWS;   // sticky: the row met an action outside [0, A)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h_ = lane >> 5, l31_ = lane & 31;
  const long long row0 = (long long)blockIdx.x * RO_ROWS;
  const int ldw = S + A;
  const float nanf_ = __int_as_float(0x7fc00000);

  // ---- step 0: the rows' states (rows past R and k >= S: zeros), the small reward-head operands, the first actions ----
  for (int e = tid; e < RO_ROWS * sp; e += RO_THREADS) {
    const int i = e / sp, k = e - i * sp;
    const unsigned r = (unsigned)row0 + i;  // (R + 32 fits 31 bits: the launcher checks)
    float v = 0.f;
    if (r < (unsigned)p.R && k < S) v = p.states[(long long)(r / (unsigned)p.K) * S + k];
    st[k * RO_LD + i] = v;
  }
  if (reward) {
    for (int e = tid; e < H * H; e += RO_THREADS) w2s[e] = p.w2[e];
    for (int e = tid; e < 2 * H; e += RO_THREADS) w3s[e] = p.w3[e];
    for (int e = tid; e < H; e += RO_THREADS) { b1s[e] = p.b1[e]; b2s[e] = p.b2[e]; }
    if (tid < 2) b3s[tid] = p.b3[tid];
  }
  const int* myplan = nullptr;  // threads 0..31: row tid's plan
  float ret = 0.f, g = 1.f;
  if (tid < RO_ROWS) {
    const long long r = row0 + tid;
    bad[tid] = 0;
    if (r < p.R) {
      myplan = p.plans + (r / p.K) * p.env_stride + (r % p.K) * (long long)T;
      const int a = myplan[0];
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

    // ---- s_{t+1} out: wave w writes rows 4w .. 4w+3 of the tile, a row's S floats along the lanes ----
    if (p.trajectory || t == T - 1) {
      for (int i = wave * (RO_ROWS / RO_WAVES); i < (wave + 1) * (RO_ROWS / RO_WAVES); ++i) {
        const long long rg = row0 + i;
        if (rg >= p.R) break;
        float* tr = p.trajectory ? p.trajectory + (rg * T + t) * S : nullptr;
        float* fin = t == T - 1 ? p.final_states + rg * S : nullptr;
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
      const long long rg = row0 + tid;
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
        ret = __fadd_rn(ret, __fmul_rn(g, prob));
        g = __fmul_rn(g, p.gamma);
        if (rg < p.R) {
          if (p.logits) {
            float* o = p.logits + (rg * T + t) * 2;
            o[0] = l0;
            o[1] = l1;
          }
          if (t == T - 1 && p.returns) p.returns[rg] = ret;
        }
      }
      if (t + 1 < T && myplan) {  // the next step's action (read by the epilogue, two barriers from here)
        const int a = myplan[t + 1];
        const bool ok = (unsigned)a < (unsigned)A;
        act[tid] = ok ? a : -1;
        if (!ok) bad[tid] = 1;
      }
    }
    __syncthreads();
  }
}

int ro_supported(int S, int A, int H, int n_rewards) {
  return S >= 1 && S <= RO_MAX_S && A >= 1 && A <= RO_MAX_A && H >= 1 && H <= RO_MAX_H && n_rewards == 2;
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
  RolloutArgs a{states, plans, plan_env_stride, wf, bf, w1, b1, w2, b2, w3, b3, final_states, returns, trajectory, reward_logits,
                R, K, T, S, A, reward ? H : 0, gamma};
  const size_t lds = ro_lds_bytes(S, reward);
  SRLZ_MAX_LDS(rollout_kernel, lds);
  SRLZ_LAUNCH(rollout_kernel, dim3((unsigned)((R + RO_ROWS - 1) / RO_ROWS)), dim3(RO_THREADS), lds, as_stream(stream), a);
  return SRLZ_OK;
}
