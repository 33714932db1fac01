// gtc.hip — the ground-truth correlation (GTC) in fp64 on gfx950, wave64: the rows the reference reads of
// np.corrcoef(x + eps, states + eps, rowvar=0) (plotting/representation_plot.py:283, read at :296-300) — the G ground-truth dimensions
// against all G + S columns of the virtual matrix [gt | states], which is never written out as a concatenation.
//
// Contract (include/srlz.h): two passes — column means, then sums of centred products; var_k for every column, cov_{g,k} for g < G;
// corr = cov / sqrt(var_g) / sqrt(var_k) with two divisions, clipped to [-1, 1] by comparisons, so that 0 / 0 = NaN of a zero-variance
// column survives as it does in numpy.  No float atomics, every sum has one order: repeated calls are bit-identical.
//
// Rows are cut into chunks whose size is a function of (N, G, S) alone (gtc_plan).  Five launches:
//   (1) gtc_sum_kernel: workgroup (64-column tile, row chunk); lane = column, wave w adds rows begin + w, begin + w + 4, ... of its
//       column in row order, the four wave sums are added as ((s0 + s1) + s2) + s3 -> psum[chunk][column] in the workspace.
//   (2) gtc_mean_kernel: thread = column, adds the partials in chunk order -> colstats[0][column] = sum / N.
//   (3) gtc_centred_kernel<GT>: the same walk with x = value - mean: av = fma(x, x, av) and, for g < G, ac[g] = fma(gt_g - mean_g, x,
//       ac[g]) in registers (GT = 4, 8 or 16 >= G accumulators, every index static) -> pvar[chunk][column], pcov[chunk][g][column].
//   (4) gtc_reduce_kernel: thread = (column, 0 = variance | 1 + g = covariance), partials in chunk order, / (N - 1) ->
//       colstats[1][column] and the raw covariance in corr[g][column].
//   (5) gtc_finish_kernel: corr[g][k] = clip(corr[g][k] / sqrt(var_g) / sqrt(var_k)).
// A thread owns a column from the first row to the last, so no sum crosses lanes: the only combine is the four-wave one in LDS.
#include <math.h>

#include "common.h"

namespace {

constexpr int GTC_TILE = 64;          // columns per workgroup = lanes of a wave
constexpr int GTC_WAVES = 4;          // waves per workgroup: rows of a chunk are dealt round-robin
constexpr int GTC_THREADS = GTC_TILE * GTC_WAVES;
constexpr int GTC_ROWS = 256;         // a chunk is a multiple of this many rows (64 per wave)
constexpr int GTC_TARGET_WGS = 1024;  // about this many workgroups whatever the shape
constexpr int GTC_MAX_G = 16;

struct GtcPlan {
  int C, tiles, chunk, nchunks;  // chunk: rows per workgroup (a multiple of GTC_ROWS)
  size_t psum_off, pvar_off, pcov_off, total;
};

size_t gtc_align(size_t x) { return (x + 255) & ~(size_t)255; }

// A function of the shape alone (not of the device), so that srlz_gtc_workspace and the launcher agree and the order of every sum
// is fixed by (N, G, S).
GtcPlan gtc_plan(int N, int G, int S) {
  GtcPlan p;
  p.C = G + S;
  p.tiles = (p.C + GTC_TILE - 1) / GTC_TILE;
  const int want = (GTC_TARGET_WGS + p.tiles - 1) / p.tiles;
  p.chunk = ((N + want - 1) / want + GTC_ROWS - 1) / GTC_ROWS * GTC_ROWS;
  p.nchunks = (N + p.chunk - 1) / p.chunk;  // <= want <= GTC_TARGET_WGS: fits grid.y
  size_t o = 0;
  p.psum_off = o; o += gtc_align((size_t)p.nchunks * p.C * sizeof(double));
  p.pvar_off = o; o += gtc_align((size_t)p.nchunks * p.C * sizeof(double));
  p.pcov_off = o; o += gtc_align((size_t)p.nchunks * G * p.C * sizeof(double));
  p.total = o;
  return p;
}

bool gtc_shape_ok(int N, int G, int S) {
  return N >= 2 && G >= 1 && G <= GTC_MAX_G && S >= 1 && (long long)N * ((long long)G + S) < (1LL << 31);
}

// element (r, k) of the virtual matrix [gt | states]
__device__ __forceinline__ double gtc_at(const double* __restrict__ gt, const double* __restrict__ st, int G, int S, int r, int k) {
  return k < G ? gt[(size_t)r * G + k] : st[(size_t)r * S + (k - G)];
}

__global__ __launch_bounds__(GTC_THREADS) void gtc_sum_kernel(const double* __restrict__ gt, const double* __restrict__ st, int N,
                                                              int G, int S, int chunk, double* __restrict__ psum) {
  __shared__ double sm[GTC_WAVES][GTC_TILE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int C = G + S, k = blockIdx.x * GTC_TILE + lane;
  const int begin = blockIdx.y * chunk, end = min(N, begin + chunk);
  double s = 0.0;
  if (k < C) {
#pragma unroll 4
    for (int r = begin + w; r < end; r += GTC_WAVES) s += gtc_at(gt, st, G, S, r, k);
  }
  sm[w][lane] = s;
  __syncthreads();
  if (w == 0 && k < C) psum[(size_t)blockIdx.y * C + k] = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}

__global__ __launch_bounds__(256) void gtc_mean_kernel(const double* __restrict__ psum, int C, int nchunks, int N,
                                                       double* __restrict__ mean) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < nchunks; ++c) s += psum[(size_t)c * C + k];  // chunk order (unrolled: the loads go ahead, the adds keep it)
  mean[k] = s / (double)N;
}

template <int GT>
__global__ __launch_bounds__(GTC_THREADS) void gtc_centred_kernel(const double* __restrict__ gt, const double* __restrict__ st, int N,
                                                                  int G, int S, int chunk, const double* __restrict__ mean,
                                                                  double* __restrict__ pvar, double* __restrict__ pcov) {
  __shared__ double sm[GTC_WAVES][GT + 1][GTC_TILE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int C = G + S, k = blockIdx.x * GTC_TILE + lane;
  const int begin = blockIdx.y * chunk, end = min(N, begin + chunk);
  double mg[GT], ac[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    mg[g] = g < G ? mean[g] : 0.0;
    ac[g] = 0.0;
  }
  double av = 0.0;
  if (k < C) {
    const double mk = mean[k];
#pragma unroll 4
    for (int r = begin + w; r < end; r += GTC_WAVES) {
      const double x = gtc_at(gt, st, G, S, r, k) - mk;
      const double* __restrict__ grow = gt + (size_t)r * G;  // the same G values for every lane: one broadcast read each
      av = fma(x, x, av);
#pragma unroll
      for (int g = 0; g < GT; ++g)
        if (g < G) ac[g] = fma(grow[g] - mg[g], x, ac[g]);
    }
  }
  sm[w][0][lane] = av;
#pragma unroll
  for (int g = 0; g < GT; ++g) sm[w][g + 1][lane] = ac[g];
  __syncthreads();
  if (w == 0 && k < C) {
    pvar[(size_t)blockIdx.y * C + k] = ((sm[0][0][lane] + sm[1][0][lane]) + sm[2][0][lane]) + sm[3][0][lane];
#pragma unroll
    for (int g = 0; g < GT; ++g)
      if (g < G)
        pcov[((size_t)blockIdx.y * G + g) * C + k] =
            ((sm[0][g + 1][lane] + sm[1][g + 1][lane]) + sm[2][g + 1][lane]) + sm[3][g + 1][lane];
  }
}

// blockIdx.y = 0: the variance of column k -> var[k]; 1 + g: the covariance of (g, k) -> corr[g][k], not yet normalised
__global__ __launch_bounds__(256) void gtc_reduce_kernel(const double* __restrict__ pvar, const double* __restrict__ pcov, int G, int C,
                                                         int nchunks, int N, double* __restrict__ var, double* __restrict__ corr) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  const int which = blockIdx.y;
  double s = 0.0;
  if (which == 0) {
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) s += pvar[(size_t)c * C + k];
    var[k] = s / (double)(N - 1);
  } else {
    const int g = which - 1;
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) s += pcov[((size_t)c * G + g) * C + k];
    corr[(size_t)g * C + k] = s / (double)(N - 1);
  }
}

// numpy's corrcoef: c /= stddev[:, None]; c /= stddev[None, :]; clip.  The comparisons let NaN through (fmin / fmax would not).
__global__ __launch_bounds__(256) void gtc_finish_kernel(const double* __restrict__ var, int G, int C, double* __restrict__ corr) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= G * C) return;
  const int g = e / C, k = e - g * C;
  double c = corr[e] / sqrt(var[g]);
  c = c / sqrt(var[k]);
  corr[e] = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
}

}  // namespace

extern "C" size_t srlz_gtc_workspace(int N, int G, int S) { return gtc_shape_ok(N, G, S) ? gtc_plan(N, G, S).total : 0; }

extern "C" int srlz_gtc_rows_f64(const double* gt, const double* states, int N, int G, int S, double* corr, double* colstats, void* ws,
                                 size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE(gt && states && corr && colstats && ws, SRLZ_ERR_NULL, "gtc_rows_f64: null pointer");
  SRLZ_REQUIRE(N >= 2, SRLZ_ERR_BAD_DESC, "gtc_rows_f64: needs N >= 2 rows (N=%d)", N);
  SRLZ_REQUIRE(G >= 1 && G <= GTC_MAX_G && S >= 1, SRLZ_ERR_BAD_DESC, "gtc_rows_f64: needs 1 <= G <= %d and S >= 1 (G=%d, S=%d)",
               GTC_MAX_G, G, S);
  SRLZ_REQUIRE((long long)N * ((long long)G + S) < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "gtc_rows_f64: N * (G + S) must stay below 2^31 (N=%d, G=%d, S=%d)", N, G, S);
  const GtcPlan p = gtc_plan(N, G, S);
  SRLZ_REQUIRE(ws_bytes >= p.total, SRLZ_ERR_WORKSPACE, "gtc_rows_f64: workspace %zu < %zu bytes", ws_bytes, p.total);
  double* psum = (double*)((char*)ws + p.psum_off);
  double* pvar = (double*)((char*)ws + p.pvar_off);
  double* pcov = (double*)((char*)ws + p.pcov_off);
  double* mean = colstats;
  double* var = colstats + p.C;
  const dim3 grid(p.tiles, p.nchunks);
  const unsigned cblocks = (unsigned)((p.C + 255) / 256);
  SRLZ_LAUNCH(gtc_sum_kernel, grid, dim3(GTC_THREADS), 0, as_stream(stream), gt, states, N, G, S, p.chunk, psum);
  SRLZ_LAUNCH(gtc_mean_kernel, dim3(cblocks), dim3(256), 0, as_stream(stream), psum, p.C, p.nchunks, N, mean);
  if (G <= 4)
    SRLZ_LAUNCH(gtc_centred_kernel<4>, grid, dim3(GTC_THREADS), 0, as_stream(stream), gt, states, N, G, S, p.chunk, mean, pvar, pcov);
  else if (G <= 8)
    SRLZ_LAUNCH(gtc_centred_kernel<8>, grid, dim3(GTC_THREADS), 0, as_stream(stream), gt, states, N, G, S, p.chunk, mean, pvar, pcov);
  else
    SRLZ_LAUNCH(gtc_centred_kernel<16>, grid, dim3(GTC_THREADS), 0, as_stream(stream), gt, states, N, G, S, p.chunk, mean, pvar, pcov);
  SRLZ_LAUNCH(gtc_reduce_kernel, dim3(cblocks, G + 1), dim3(256), 0, as_stream(stream), pvar, pcov, G, p.C, p.nchunks, N, var, corr);
  SRLZ_LAUNCH(gtc_finish_kernel, dim3((unsigned)((G * p.C + 255) / 256)), dim3(256), 0, as_stream(stream), var, G, p.C, corr);
  return 0;
}
