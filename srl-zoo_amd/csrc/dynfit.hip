// dynfit.hip — the normal equations of the forward head in fp64 on gfx950, wave64: the least-squares fit of
//     next_state = state + Linear(cat(state, onehot(action)))          (reference models/forward_inverse.py:16,30-31)
// over a list of recorded transitions (srlz/dynfit.py solves the small system on the host).
//
// For transition m, i = starts[m]:  z = [ (double)s_i | onehot(a_i) | 1 ]  (P = S + A + 1 columns),  y = (double)s_{i+1} - (double)s_i.
// G = sum_m z zᵀ [P,P] and C = sum_m z yᵀ [P,S].  Neither Z nor Y is ever written: the contraction runs over the ROWS (pca.hip
// contracts over the contiguous axis), the rows are gathered by `starts`, and the one-hot block, the constant column and the
// difference are formed while a stage of rows goes into LDS.
//
// Output tiles are 16 x 16.  Row tile ti (16 columns of z) needs the column tiles  L(ti) = [ z tiles 0 .. ti ; y tiles 0 .. TS-1 ]:
// the lower triangle of G, and C.  The flat tile index is  ti (ti + 1) / 2 + ti TS + e,  e the place in L(ti).
// Kernels:
//   dynfit_tiles_kernel   workgroup = (chunk of transitions, row tile ti, group g of DF_NT entries of L(ti)).  Per stage of DF_ROWS
//                         transitions the 256 threads write xs[row][0..16) = the z columns of ti and xs[row][16 + 16 e' ..) = the
//                         columns of the group's entries, in fp64 (the element index runs fastest over the columns: the loads of s_i
//                         and s_{i+1} are coalesced).  Then v_mfma_f64_16x16x4_f64: the MFMA's k index runs over four rows of the
//                         stage; wave w takes the row quads w, w + 4, .. and keeps one accumulator per entry of the group.  After the
//                         last stage the four waves' tiles are added in wave order, ((w0 + w1) + w2) + w3, and go to
//                         ws[tile][chunk][16][16].
//   dynfit_reduce_kernel  thread = output element: its partials summed in chunk order; G is mirrored (the upper triangle is a copy
//                         of the lower one: exactly symmetric).  Every element of G and C is written exactly once.
// Operand / result layout of the fp64 MFMA as in pca.hip: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D: col = lane & 15, row = (lane >> 4) + 4 * reg.
// No float atomics, every sum has one order that depends on (M, S, A) alone: repeated calls are bit-identical.
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_WAVES = DF_THREADS / 64;
constexpr int DF_ROWS = 32;                     // transitions of a stage; chunks are multiples of it
constexpr int DF_NT = 8;                        // column tiles (accumulators) of a workgroup
constexpr int DF_COLS = 16 + DF_NT * 16;        // columns of a staged row: the row tile's, then the group's
constexpr int DF_STRIDE = DF_COLS + 2;          // (padding: the four rows of an MFMA step start in different banks)
constexpr int DF_MAX_S = 512;
constexpr int DF_MAX_A = 64;
constexpr int DF_MAX_CHUNKS = 256;
constexpr int DF_MAX_PARTIALS = 16384;          // tiles x chunks: 32 MiB of partials at most

struct DfPlan {
  int P, TP, TS, tiles, groups, chunks, chunk_rows;
  size_t total;  // bytes of partials: [tiles][chunks][16][16] fp64
};

__host__ __device__ __forceinline__ int df_entries(int ti, int TS) { return ti + 1 + TS; }
__host__ __device__ __forceinline__ int df_tile_base(int ti, int TS) { return ti * (ti + 1) / 2 + ti * TS; }

bool df_supported(int S, int A) { return S >= 1 && S <= DF_MAX_S && A >= 1 && A <= DF_MAX_A; }

// A function of the shapes alone, so that the queries and the launcher agree.
DfPlan df_plan(int M, int S, int A) {
  DfPlan p;
  p.P = S + A + 1;
  p.TP = (p.P + 15) / 16;
  p.TS = (S + 15) / 16;
  p.tiles = df_tile_base(p.TP, p.TS);
  p.groups = 0;
  for (int ti = 0; ti < p.TP; ++ti) p.groups += (df_entries(ti, p.TS) + DF_NT - 1) / DF_NT;
  long long c = ((long long)M + DF_ROWS - 1) / DF_ROWS;
  if (c > DF_MAX_CHUNKS) c = DF_MAX_CHUNKS;
  if (c > DF_MAX_PARTIALS / p.tiles) c = DF_MAX_PARTIALS / p.tiles;
  if (c < 1) c = 1;
  const long long rows = (((long long)M + c - 1) / c + DF_ROWS - 1) / DF_ROWS * DF_ROWS;
  p.chunk_rows = (int)rows;
  p.chunks = (int)(((long long)M + rows - 1) / rows);
  p.total = (size_t)p.tiles * p.chunks * 256 * sizeof(double);
  return p;
}

// Column `col` of [z | y] rows: kind 0 = z, 1 = y.  `fr` < 0: a row past the chunk's end, all zeros (the constant column too).
__device__ __forceinline__ double df_elem(const float* __restrict__ states, int fr, int act, int kind, int col, int S, int A) {
  if (fr < 0) return 0.0;
  if (kind == 0) {
    if (col < S) return (double)states[(size_t)fr * S + col];
    if (col < S + A) return act == col - S ? 1.0 : 0.0;  // (an action outside [0, A): a zero one-hot row)
    return col == S + A ? 1.0 : 0.0;
  }
  if (col >= S) return 0.0;
  return (double)states[(size_t)(fr + 1) * S + col] - (double)states[(size_t)fr * S + col];
}

__global__ __launch_bounds__(DF_THREADS) void dynfit_tiles_kernel(const float* __restrict__ states, const int* __restrict__ actions,
                                                                   const int* __restrict__ starts, int N, int M, int S, int A, int TS,
                                                                   int chunk_rows, double* __restrict__ ws) {
  __shared__ double xs[DF_ROWS * DF_STRIDE];
  __shared__ double part[DF_WAVES][256];
  __shared__ int fr_s[DF_ROWS], act_s[DF_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  // blockIdx.y -> (row tile ti, group g)
  int ti = 0, g = blockIdx.y;
  for (;; ++ti) {
    const int ng = (df_entries(ti, TS) + DF_NT - 1) / DF_NT;
    if (g < ng) break;
    g -= ng;
  }
  const int e0 = g * DF_NT;
  const int nt = min(DF_NT, df_entries(ti, TS) - e0);  // entries of this group: 1 .. DF_NT
  const int chunk = blockIdx.x;
  const int row_begin = chunk * chunk_rows, row_end = min(M, row_begin + chunk_rows);
  f64x4 acc[DF_NT];
#pragma unroll
  for (int t = 0; t < DF_NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int r0 = row_begin; r0 < row_end; r0 += DF_ROWS) {
    if (tid < DF_ROWS) {
      const int m = r0 + tid;
      int fr = -1, act = -1;
      if (m < row_end) {
        fr = min(max(starts[m], 0), N - 2);  // (the host table was checked before the launch; this one is never trusted with an address)
        act = actions[fr];
      }
      fr_s[tid] = fr;
      act_s[tid] = act;
    }
    __syncthreads();
    for (int idx = tid; idx < DF_ROWS * DF_COLS; idx += DF_THREADS) {
      const int r = idx / DF_COLS, c = idx - r * DF_COLS;
      double v = 0.0;
      if (c < 16) {
        v = df_elem(states, fr_s[r], act_s[r], 0, ti * 16 + c, S, A);
      } else {
        const int el = (c - 16) >> 4, e = e0 + el;
        if (el < nt) v = e <= ti ? df_elem(states, fr_s[r], act_s[r], 0, e * 16 + (c & 15), S, A)
                                 : df_elem(states, fr_s[r], act_s[r], 1, (e - ti - 1) * 16 + (c & 15), S, A);
      }
      xs[r * DF_STRIDE + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < DF_ROWS / 4 / DF_WAVES; ++ks) {
      const double* row = xs + ((ks * DF_WAVES + wave) * 4 + q) * DF_STRIDE;
      const double a = row[i];
#pragma unroll
      for (int t = 0; t < DF_NT; ++t)
        if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, row[16 + t * 16 + i], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  const size_t tile0 = (size_t)df_tile_base(ti, TS) + e0;
#pragma unroll
  for (int t = 0; t < DF_NT; ++t) {
    if (t < nt) {  // (uniform over the workgroup: the barriers are met by every thread)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) part[wave][(q + 4 * reg) * 16 + i] = acc[t][reg];
      __syncthreads();
      double* out = ws + ((tile0 + t) * gridDim.x + chunk) * 256;
      out[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(DF_THREADS) void dynfit_reduce_kernel(const double* __restrict__ ws, int chunks, int P, int S, int TS,
                                                                    double* __restrict__ G, double* __restrict__ C) {
  // blockIdx.x = flat tile -> (row tile ti, entry e)
  int ti = 0, e = blockIdx.x;
  for (;; ++ti) {
    const int n = df_entries(ti, TS);
    if (e < n) break;
    e -= n;
  }
  const int el = threadIdx.x, row = ti * 16 + (el >> 4);
  if (row >= P) return;
  const bool gram = e <= ti;
  const int col = (gram ? e : e - ti - 1) * 16 + (el & 15);
  if (gram ? col > row : col >= S) return;  // (a diagonal tile keeps its lower half: the mirror below writes the upper one)
  const double* p = ws + (size_t)blockIdx.x * chunks * 256 + el;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += p[(size_t)c * 256];
  if (gram) {
    G[(size_t)row * P + col] = s;
    if (col != row) G[(size_t)col * P + row] = s;
  } else {
    C[(size_t)row * S + col] = s;
  }
}

}  // namespace

extern "C" int srlz_dynfit_supported(int S, int A) { return df_supported(S, A) ? 1 : 0; }

extern "C" int srlz_dynfit_chunk_rows(int M, int S, int A) { return (M >= 1 && df_supported(S, A)) ? df_plan(M, S, A).chunk_rows : 0; }

extern "C" size_t srlz_dynfit_workspace(int M, int S, int A) { return (M >= 1 && df_supported(S, A)) ? df_plan(M, S, A).total : 0; }

extern "C" int srlz_dynfit_gram(const float* states, const int* actions, const int* starts, const int* starts_host, int N, int M, int S,
                                int A, double* G, double* C, void* ws, size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE(df_supported(S, A), SRLZ_ERR_BAD_DESC, "dynfit_gram: needs 1 <= S <= %d and 1 <= A <= %d (S=%d, A=%d)", DF_MAX_S, DF_MAX_A,
               S, A);
  SRLZ_REQUIRE(states && actions && starts && starts_host && G && C && ws, SRLZ_ERR_NULL, "dynfit_gram: null pointer");
  SRLZ_REQUIRE(N >= 2 && M >= 1, SRLZ_ERR_BAD_DESC, "dynfit_gram: needs N >= 2 frames and M >= 1 transitions (N=%d, M=%d)", N, M);
  SRLZ_REQUIRE((long long)N * S < (1LL << 31), SRLZ_ERR_BAD_DESC, "dynfit_gram: N * S = %lld must stay below 2^31", (long long)N * S);
  for (int m = 0; m < M; ++m)
    SRLZ_REQUIRE(starts_host[m] >= 0 && starts_host[m] <= N - 2, SRLZ_ERR_BAD_DESC,
                 "dynfit_gram: starts[%d] = %d outside [0, %d] (a transition needs frames i and i + 1)", m, starts_host[m], N - 2);
  const DfPlan p = df_plan(M, S, A);
  SRLZ_REQUIRE(ws_bytes >= p.total, SRLZ_ERR_WORKSPACE, "dynfit_gram: workspace %zu < %zu bytes", ws_bytes, p.total);
  SRLZ_LAUNCH(dynfit_tiles_kernel, dim3(p.chunks, p.groups), dim3(DF_THREADS), 0, as_stream(stream), states, actions, starts, N, M, S, A,
              p.TS, p.chunk_rows, (double*)ws);
  SRLZ_LAUNCH(dynfit_reduce_kernel, dim3(p.tiles), dim3(DF_THREADS), 0, as_stream(stream), (const double*)ws, p.chunks, p.P, S, p.TS, G,
              C);
  return 0;
}
