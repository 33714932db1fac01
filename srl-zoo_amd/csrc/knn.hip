// knn.hip — exact k nearest neighbours in fp64 on gfx950, wave64: the search behind KNN-MSE (reference evaluation/knn_images.py:83-84,
// NearestNeighbors(n_neighbors=k + 1, algorithm='ball_tree').fit(states).kneighbors(states)).
//
// Contract (include/srlz.h): dist2(q, x) = sum_d (q_d - x_d)^2 as ONE fp64 chain acc = fma(q_d - x_d, q_d - x_d, acc) over
// d = 0 .. D-1, so a pair's value does not depend on any tiling; row r of the output = the K database rows with the smallest key
// (dist2, index), ascending.  No float atomics, every merge has one order: repeated calls are bit-identical.
//
// Three launches:
//   (1) knn_transpose_kernel: queries [Q, D] -> qT [Dpad][Qpad] in the workspace, zero padded (Dpad multiple of 16, Qpad of 256), so
//       that the 256 threads of a tile read dimension d of their queries as one coalesced row.  A padded dimension adds
//       fma(0, 0, acc) = acc: the chain is unchanged.
//   (2) knn_partial_kernel<KC>: workgroup (query tile of 256, database split s); thread = one query.  The split's rows pass through
//       LDS 16 rows x 64 dimensions at a time (read as broadcasts), the thread keeps 16 running chains and 16 query values in
//       registers and, per 16 rows, offers the finished distances to its sorted candidate list of KC >= K entries — registers only,
//       every index static.  The list goes to part[q][s][K].  The database is split so that about 1024 workgroups exist whatever Q
//       is: Q = 200 against tens of thousands of rows fills the chip with 256 splits, Q = N with a dozen.
//   (3) knn_merge_kernel: one wave per query merges the S sorted lists: lane l owns lists l, l + 64, l + 128, l + 192, K rounds of a
//       wave-wide minimum over the list heads by (dist2, index) (wave_min_key_d, common.h).  Indices are unique, so every round has
//       one winner.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int KNN_THREADS = 256;  // queries per tile = threads per workgroup
constexpr int KNN_BN = 16;        // database rows per LDS tile = running chains per thread
constexpr int KNN_DK = 16;        // query values held in registers
constexpr int KNN_DKS = 64;       // dimensions per LDS tile
constexpr int KNN_LOADS = KNN_BN * KNN_DKS / KNN_THREADS;  // tile elements staged per thread
constexpr int KNN_MAX_SPLITS = 256;                        // 4 lists per lane of the merging wave
constexpr int KNN_TARGET_WGS = 1024;
constexpr int KNN_MAX_K = 32;

struct KnnPlan {
  int qtiles, splits, chunk;  // chunk: database rows per split (a multiple of KNN_BN)
  int qpad, dpad;
  size_t qt_off, pd_off, pi_off, total;
};

size_t knn_align(size_t x) { return (x + 255) & ~(size_t)255; }

// A function of the shapes alone (not of the device), so that srlz_knn_workspace and the launcher agree.
KnnPlan knn_plan(int N, int Q, int D, int K) {
  KnnPlan p;
  p.qtiles = (Q + KNN_THREADS - 1) / KNN_THREADS;
  int s = (KNN_TARGET_WGS + p.qtiles - 1) / p.qtiles;
  if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
  const int tiles = (N + KNN_BN - 1) / KNN_BN;
  if (s > tiles) s = tiles;
  if (s < 1) s = 1;
  p.chunk = ((N + s - 1) / s + KNN_BN - 1) / KNN_BN * KNN_BN;
  p.splits = (N + p.chunk - 1) / p.chunk;
  p.qpad = p.qtiles * KNN_THREADS;
  p.dpad = (D + KNN_DK - 1) / KNN_DK * KNN_DK;
  size_t o = 0;
  p.qt_off = o; o += knn_align((size_t)p.dpad * p.qpad * sizeof(double));
  p.pd_off = o; o += knn_align((size_t)Q * p.splits * K * sizeof(double));
  p.pi_off = o; o += knn_align((size_t)Q * p.splits * K * sizeof(int));
  p.total = o;
  return p;
}

__global__ __launch_bounds__(256) void knn_transpose_kernel(const double* __restrict__ q, int Q, int D, int qpad, int dpad,
                                                            double* __restrict__ qT) {
  const size_t n = (size_t)qpad * dpad;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int d = (int)(e / qpad), j = (int)(e - (size_t)d * qpad);
  qT[e] = (d < D && j < Q) ? q[(size_t)j * D + d] : 0.0;
}

// (d, i) into the ascending list by key (dist2, index): the entries behind the insertion point move down one slot, the last one drops
// out.  Fully unrolled: the list never leaves its registers.
template <int KC>
__device__ __forceinline__ void knn_offer(double (&ld)[KC], int (&li)[KC], double d, int i) {
  if (!key_less_d(d, i, ld[KC - 1], li[KC - 1])) return;
  int pos = 0;  // entries that stay in front of (d, i)
#pragma unroll
  for (int j = 0; j < KC - 1; ++j) pos += key_less_d(ld[j], li[j], d, i) ? 1 : 0;
#pragma unroll
  for (int j = KC - 1; j >= 0; --j) {
    if (j > 0 && j > pos) {
      ld[j] = ld[j > 0 ? j - 1 : 0];
      li[j] = li[j > 0 ? j - 1 : 0];
    } else if (j == pos) {
      ld[j] = d;
      li[j] = i;
    }
  }
}

template <int KC>
__global__ __launch_bounds__(KNN_THREADS, KC <= 16 ? 2 : 1) void knn_partial_kernel(const double* __restrict__ db, int N, int D,
                                                                  const double* __restrict__ qT, int Q, int qpad, int K, int chunk,
                                                                  int splits, double* __restrict__ pd, int* __restrict__ pi) {
  __shared__ double xs[KNN_BN][KNN_DKS];
  const int tid = threadIdx.x;
  const int split = blockIdx.y, q = blockIdx.x * KNN_THREADS + tid;  // q < qpad: the padded queries are zeros, computed and dropped
  const int row_begin = split * chunk, row_end = min(N, row_begin + chunk);
  const int ntile = (row_end - row_begin + KNN_BN - 1) / KNN_BN, nchunk = (D + KNN_DKS - 1) / KNN_DKS;
  const int nstage = ntile * nchunk;

  double ld[KC];
  int li[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    ld[j] = INFINITY;
    li[j] = INT_MAX;
  }
  double acc[KNN_BN];
#pragma unroll
  for (int r = 0; r < KNN_BN; ++r) acc[r] = 0.0;

  // element e of a tile: row e / 64, dimension e % 64; outside the split or beyond D: 0 (adds nothing to a chain)
  auto fetch = [&](int stage, double (&v)[KNN_LOADS]) {
    const int row0 = row_begin + (stage / nchunk) * KNN_BN, d0 = (stage % nchunk) * KNN_DKS;
#pragma unroll
    for (int u = 0; u < KNN_LOADS; ++u) {
      const int e = u * KNN_THREADS + tid, row = row0 + e / KNN_DKS, d = d0 + e % KNN_DKS;
      v[u] = (row < row_end && d < D) ? db[(size_t)row * D + d] : 0.0;
    }
  };
  auto stash = [&](const double (&v)[KNN_LOADS]) {
#pragma unroll
    for (int u = 0; u < KNN_LOADS; ++u) {
      const int e = u * KNN_THREADS + tid;
      xs[e / KNN_DKS][e % KNN_DKS] = v[u];
    }
  };

  double pre[KNN_LOADS];
  fetch(0, pre);
  stash(pre);
  __syncthreads();
  for (int stage = 0; stage < nstage; ++stage) {
    const int t = stage / nchunk, c = stage - t * nchunk;
    const int d0 = c * KNN_DKS;
    if (stage + 1 < nstage) fetch(stage + 1, pre);  // in flight while this stage computes
    const int nsub = (min(KNN_DKS, D - d0) + KNN_DK - 1) / KNN_DK;
    for (int sub = 0; sub < nsub; ++sub) {
      double qv[KNN_DK];
      const double* qp = qT + (size_t)(d0 + sub * KNN_DK) * qpad + q;  // rows below dpad: zero padded
#pragma unroll
      for (int dd = 0; dd < KNN_DK; ++dd) qv[dd] = qp[(size_t)dd * qpad];
#pragma unroll
      for (int dd = 0; dd < KNN_DK; ++dd) {
#pragma unroll
        for (int r = 0; r < KNN_BN; ++r) {
          const double diff = qv[dd] - xs[r][sub * KNN_DK + dd];
          acc[r] = fma(diff, diff, acc[r]);  // THE chain: d ascending, one fma per dimension
        }
      }
    }
    if (c == nchunk - 1) {
      const int row0 = row_begin + t * KNN_BN;
#pragma unroll
      for (int r = 0; r < KNN_BN; ++r) {
        if (row0 + r < row_end) knn_offer<KC>(ld, li, acc[r], row0 + r);
        acc[r] = 0.0;
      }
    }
    __syncthreads();
    if (stage + 1 < nstage) stash(pre);
    __syncthreads();
  }
  if (q < Q) {
    double* od = pd + ((size_t)q * splits + split) * K;
    int* oi = pi + ((size_t)q * splits + split) * K;
#pragma unroll
    for (int j = 0; j < KC; ++j)
      if (j < K) {
        od[j] = ld[j];
        oi[j] = li[j];
      }
  }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ pd, const int* __restrict__ pi, int Q, int K,
                                                        int splits, int* __restrict__ idx, double* __restrict__ dist2) {
  constexpr int OWN = KNN_MAX_SPLITS / 64;
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Q) return;  // (whole waves: no workgroup barrier below)
  const double* qd = pd + (size_t)q * splits * K;
  const int* qi = pi + (size_t)q * splits * K;
  double hd[OWN];
  int hi[OWN], pos[OWN];
#pragma unroll
  for (int o = 0; o < OWN; ++o) {
    const int s = lane + 64 * o;
    pos[o] = 0;
    hd[o] = s < splits ? qd[(size_t)s * K] : INFINITY;
    hi[o] = s < splits ? qi[(size_t)s * K] : INT_MAX;
  }
  for (int k = 0; k < K; ++k) {
    double bd = hd[0];
    int bi = hi[0];
#pragma unroll
    for (int o = 1; o < OWN; ++o)
      if (key_less_d(hd[o], hi[o], bd, bi)) {
        bd = hd[o];
        bi = hi[o];
      }
    wave_min_key_d(bd, bi);
    if (lane == 0) {
      idx[(size_t)q * K + k] = bi;
      dist2[(size_t)q * K + k] = bd;
    }
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
      const int s = lane + 64 * o;
      if (s < splits && hi[o] == bi && hi[o] != INT_MAX) {  // the one list whose head won moves on
        ++pos[o];
        hd[o] = pos[o] < K ? qd[(size_t)s * K + pos[o]] : INFINITY;
        hi[o] = pos[o] < K ? qi[(size_t)s * K + pos[o]] : INT_MAX;
      }
    }
  }
}

template <typename T>
T* knn_at(void* base, size_t off) { return (T*)((char*)base + off); }

bool knn_shape_ok(int N, int Q, int D, int K) {
  return K >= 1 && K <= KNN_MAX_K && K <= N && D >= 1 && Q >= 1 && (long long)N * D < (1LL << 31) &&
         (long long)Q * K < (1LL << 31);
}

}  // namespace

extern "C" size_t srlz_knn_workspace(int N, int Q, int D, int K) { return knn_shape_ok(N, Q, D, K) ? knn_plan(N, Q, D, K).total : 0; }

extern "C" int srlz_knn_f64(const double* db, int N, const double* queries, int Q, int D, int K, int* idx, double* dist2, void* ws,
                            size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE(db && queries && idx && dist2 && ws, SRLZ_ERR_NULL, "knn_f64: null pointer");
  SRLZ_REQUIRE(K >= 1 && K <= KNN_MAX_K && K <= N, SRLZ_ERR_BAD_DESC, "knn_f64: needs 1 <= K <= min(%d, N) (K=%d, N=%d)", KNN_MAX_K, K,
               N);
  SRLZ_REQUIRE(D >= 1 && Q >= 1, SRLZ_ERR_BAD_DESC, "knn_f64: needs D >= 1 and Q >= 1 (D=%d, Q=%d)", D, Q);
  SRLZ_REQUIRE((long long)N * D < (1LL << 31) && (long long)Q * K < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "knn_f64: N * D and Q * K must stay below 2^31 (N=%d, D=%d, Q=%d, K=%d)", N, D, Q, K);
  const KnnPlan p = knn_plan(N, Q, D, K);
  SRLZ_REQUIRE(ws_bytes >= p.total, SRLZ_ERR_WORKSPACE, "knn_f64: workspace %zu < %zu bytes", ws_bytes, p.total);
  double* qT = knn_at<double>(ws, p.qt_off);
  double* pd = knn_at<double>(ws, p.pd_off);
  int* pi = knn_at<int>(ws, p.pi_off);
  const size_t nq = (size_t)p.qpad * p.dpad;
  SRLZ_LAUNCH(knn_transpose_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, as_stream(stream), queries, Q, D, p.qpad, p.dpad,
              qT);
  const dim3 grid(p.qtiles, p.splits);  // (splits <= 256 fits grid.y for any Q)
  if (K <= 8)
    SRLZ_LAUNCH(knn_partial_kernel<8>, grid, dim3(KNN_THREADS), 0, as_stream(stream), db, N, D, qT, Q, p.qpad, K, p.chunk, p.splits, pd,
                pi);
  else if (K <= 16)
    SRLZ_LAUNCH(knn_partial_kernel<16>, grid, dim3(KNN_THREADS), 0, as_stream(stream), db, N, D, qT, Q, p.qpad, K, p.chunk, p.splits, pd,
                pi);
  else
    SRLZ_LAUNCH(knn_partial_kernel<32>, grid, dim3(KNN_THREADS), 0, as_stream(stream), db, N, D, qT, Q, p.qpad, K, p.chunk, p.splits, pd,
                pi);
  SRLZ_LAUNCH(knn_merge_kernel, dim3((Q + 3) / 4), dim3(256), 0, as_stream(stream), pd, pi, Q, K, p.splits, idx, dist2);
  return 0;
}
