// pca.hip — the PCA baseline's arithmetic in fp64 on gfx950, wave64: sklearn's IncrementalPCA.partial_fit / transform (reference
// srl_baselines/pca.py:98-121) with the LAPACK SVD of the (k + bs + 1) x D matrix per minibatch replaced by its small Gram matrix.
//
// The matrix sklearn decomposes is never written.  Its rows are VIRTUAL (struct VRows) and formed where they are read:
//     [ nb basis rows S·V, fp64 ;  nf frame rows minus a column vector (batch mean / running mean) ;  one correction row ]
// a frame row being the loader's planar uint8 bytes through the srlz_normalize_lut table, or fp32.
//
// Kernels:
//   pca_stats_kernel     thread = column, rows looped: sklearn.utils.extmath._incremental_mean_and_var, the batch mean and the
//                        mean-correction row.
//   pca_tiles_kernel     workgroup = (chunk of D, 16 x 16 output tile); the product of two virtual matrices over that chunk with
//                        v_mfma_f64_16x16x4_f64.  A wave takes 64 columns per step: lane (i = lane & 15, q = lane >> 4) holds the 16
//                        CONSECUTIVE columns 16 q .. 16 q + 15 of row i (one 16-byte load of a uint8 frame) and the 16 MFMAs of the
//                        step pair them off — the k index of an MFMA is only a summation index, any assignment of columns to it is
//                        right as long as both operands use the same one.  The four waves' tiles are added in wave order and the
//                        partial [16][16] goes to ws[tile][chunk].  Used for G = A·Aᵀ (lower triangle of tiles) and for the
//                        transform (frames − mean)·(S·V)ᵀ.
//   pca_gram_reduce / pca_transform_reduce    thread = output element: its partials summed in chunk order; G is mirrored (the upper
//                        triangle is a copy of the lower one: exactly symmetric), the states are divided by S and rounded to fp32.
//   pca_project_kernel   out[k, D] = W[k, r]·A: wave = 16 rows of W x 64 columns, the MFMA's k index runs over the rows of A.
// C/D layout of the fp64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg (NOT the fp32 forms' 4 * (lane >> 4) + reg); A/B: one
// fp64 per lane, A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15].
// No float atomics, every sum has one order: repeated calls are bit-identical.
#include <math.h>

#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int PCA_THREADS = 256;
constexpr int PCA_WAVES = PCA_THREADS / 64;
constexpr int PCA_SLAB = 64;                      // columns a wave takes per step
constexpr int PCA_BLOCK_COLS = PCA_SLAB * PCA_WAVES;  // columns a workgroup takes per step: chunks are multiples of it
constexpr int PCA_TARGET_WGS = 1024;
constexpr int PCA_MAX_CHUNKS = 256;
constexpr int PCA_MAX_ROWS = 1 << 15;
constexpr int PCA_MAX_TILES = 65535;  // output tiles of one launch (grid.y)

struct VRows {
  const double* basis;  // [nb, D] fp64
  int nb;
  const uint8_t* u8;    // [nf, D] planar bytes, or
  const float* f32;     // [nf, D]
  const float* lut;     // [3][256], channel c of a uint8 frame reads row c % 3
  int plane;            // columns per channel plane (uint8 form)
  int nf;
  const double* sub;    // [D] subtracted from every frame row
  const double* corr;   // [D] the last row, or NULL
  int rows;             // nb + nf + (corr ? 1 : 0)
};

__device__ __forceinline__ double vrow_elem(const VRows& v, int row, int col, int D) {
  if (row >= v.rows || col >= D) return 0.0;
  if (row < v.nb) return v.basis[(size_t)row * D + col];
  row -= v.nb;
  if (row < v.nf) {
    const size_t e = (size_t)row * D + col;
    const double x = v.u8 ? (double)v.lut[((col / v.plane) % 3) * 256 + v.u8[e]] : (double)v.f32[e];
    return x - v.sub[col];
  }
  return v.corr[col];
}

// Columns c0 .. c0 + 15 of a row.  VEC: D (and the plane) are multiples of 16 and every buffer is 16-byte aligned, so the 16 columns
// lie wholly inside or outside the matrix and inside one channel plane.
template <bool VEC>
__device__ __forceinline__ void vrow_load16(const VRows& v, int row, int c0, int D, double (&x)[16]) {
  if (!VEC) {
#pragma unroll
    for (int s = 0; s < 16; ++s) x[s] = vrow_elem(v, row, c0 + s, D);
    return;
  }
#pragma unroll
  for (int s = 0; s < 16; ++s) x[s] = 0.0;
  if (row >= v.rows || c0 >= D) return;
  if (row < v.nb) {
    const f64x2* p = (const f64x2*)(v.basis + (size_t)row * D + c0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const f64x2 t = p[s];
      x[2 * s] = t.x;
      x[2 * s + 1] = t.y;
    }
    return;
  }
  row -= v.nb;
  if (row < v.nf) {
    const size_t e = (size_t)row * D + c0;
    if (v.u8) {
      const uint4 b = *(const uint4*)(v.u8 + e);
      const float* l = v.lut + ((c0 / v.plane) % 3) * 256;
      const unsigned w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int s = 0; s < 16; ++s) x[s] = (double)l[(w[s >> 2] >> (8 * (s & 3))) & 255u];
    } else {
      const f32x4* p = (const f32x4*)(v.f32 + e);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const f32x4 t = p[s];
        x[4 * s] = (double)t.x;
        x[4 * s + 1] = (double)t.y;
        x[4 * s + 2] = (double)t.z;
        x[4 * s + 3] = (double)t.w;
      }
    }
    const f64x2* q = (const f64x2*)(v.sub + c0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const f64x2 t = q[s];
      x[2 * s] -= t.x;
      x[2 * s + 1] -= t.y;
    }
    return;
  }
  const f64x2* p = (const f64x2*)(v.corr + c0);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const f64x2 t = p[s];
    x[2 * s] = t.x;
    x[2 * s + 1] = t.y;
  }
}

// ---- column statistics -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PCA_THREADS) void pca_stats_kernel(VRows x, int D, double n_seen, double* __restrict__ mean,
                                                                 double* __restrict__ var, double* __restrict__ bmean,
                                                                 double* __restrict__ corr) {
  const int col = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (col >= D) return;
  const int m = x.nf;
  auto value = [&](int row) -> double {
    const size_t e = (size_t)row * D + col;
    return x.u8 ? (double)x.lut[((col / x.plane) % 3) * 256 + x.u8[e]] : (double)x.f32[e];
  };
  double new_sum = 0.0;
  for (int row = 0; row < m; ++row) new_sum += value(row);
  const double T = new_sum / m;
  double correction = 0.0, sq = 0.0;
  for (int row = 0; row < m; ++row) {
    const double t = value(row) - T;
    correction += t;
    sq = fma(t, t, sq);
  }
  const double new_unnorm = sq - correction * correction / m;
  const double total = n_seen + m;
  const double last_mean = n_seen > 0.0 ? mean[col] : 0.0;
  double upd_unnorm = new_unnorm;
  if (n_seen > 0.0) {
    const double last_sum = last_mean * n_seen, ratio = n_seen / m;
    const double d = last_sum / ratio - new_sum;
    upd_unnorm = var[col] * n_seen + new_unnorm + ratio / total * d * d;
  }
  mean[col] = (last_mean * n_seen + new_sum) / total;
  var[col] = upd_unnorm / total;
  bmean[col] = T;
  corr[col] = n_seen > 0.0 ? sqrt(n_seen / total * m) * (last_mean - T) : 0.0;
}

// ---- tiles of a product of two virtual matrices over chunks of D ---------------------------------------------------------------
struct TilePlan {
  int tiles, chunks, chunk_cols;
  size_t total;  // bytes of partials: [tiles][chunks][16][16] fp64
};

// A function of the shapes alone, so that the workspace queries and the launchers agree.
TilePlan tile_plan(long long tiles, int D) {
  TilePlan p;
  p.tiles = (int)tiles;
  long long c = PCA_TARGET_WGS / (tiles > 0 ? tiles : 1);
  const int most = (D + PCA_BLOCK_COLS - 1) / PCA_BLOCK_COLS;
  if (c > PCA_MAX_CHUNKS) c = PCA_MAX_CHUNKS;
  if (c > most) c = most;
  if (c < 1) c = 1;
  p.chunk_cols = (int)(((D + c - 1) / c + PCA_BLOCK_COLS - 1) / PCA_BLOCK_COLS * PCA_BLOCK_COLS);
  p.chunks = (D + p.chunk_cols - 1) / p.chunk_cols;
  p.total = (size_t)tiles * p.chunks * 256 * sizeof(double);
  return p;
}

// tile t of the lower triangle, rows first: t = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void tri_tile(int t, int& ti, int& tj) {
  int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  while (i * (i + 1) / 2 > t) --i;
  ti = i;
  tj = t - i * (i + 1) / 2;
}

// TRI: A = B and blockIdx.y walks the lower triangle of tiles; else blockIdx.y = ti * tiles_b + tj over the whole rectangle.
template <bool VEC, bool TRI>
__global__ __launch_bounds__(PCA_THREADS) void pca_tiles_kernel(VRows a, VRows b, int tiles_b, int D, int chunk_cols,
                                                                 double* __restrict__ ws) {
  __shared__ double part[PCA_WAVES][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  int ti, tj;
  if (TRI) {
    tri_tile(blockIdx.y, ti, tj);
  } else {
    ti = blockIdx.y / tiles_b;
    tj = blockIdx.y - ti * tiles_b;
  }
  const int chunk = blockIdx.x, col_begin = chunk * chunk_cols;
  const int col_end = min(D, col_begin + chunk_cols);
  const bool same = TRI && ti == tj;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int c = col_begin + wave * PCA_SLAB; c < col_end; c += PCA_BLOCK_COLS) {
    double xa[16], xb[16];
    vrow_load16<VEC>(a, ti * 16 + i, c + q * 16, D, xa);
    if (same) {
#pragma unroll
      for (int s = 0; s < 16; ++s) xb[s] = xa[s];
    } else {
      vrow_load16<VEC>(b, tj * 16 + i, c + q * 16, D, xb);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s], xb[s], acc, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) part[wave][(q + 4 * reg) * 16 + i] = acc[reg];
  __syncthreads();
  double* out = ws + ((size_t)blockIdx.y * gridDim.x + chunk) * 256;
  const int e = threadIdx.x;
  out[e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
}

__global__ __launch_bounds__(PCA_THREADS) void pca_gram_reduce_kernel(const double* __restrict__ ws, int chunks, int r,
                                                                       double* __restrict__ G) {
  int ti, tj;
  tri_tile(blockIdx.x, ti, tj);
  const int e = threadIdx.x, row = ti * 16 + (e >> 4), col = tj * 16 + (e & 15);
  if (row >= r || col > row) return;  // (a diagonal tile keeps its lower half: the mirror below writes the upper one)
  const double* p = ws + (size_t)blockIdx.x * chunks * 256 + e;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += p[(size_t)c * 256];
  G[(size_t)row * r + col] = s;
  G[(size_t)col * r + row] = s;
}

__global__ __launch_bounds__(PCA_THREADS) void pca_transform_reduce_kernel(const double* __restrict__ ws, int chunks, int tiles_k, int M,
                                                                            int k, const double* __restrict__ S,
                                                                            float* __restrict__ states) {
  const int ti = blockIdx.x / tiles_k, tj = blockIdx.x - ti * tiles_k;
  const int e = threadIdx.x, row = ti * 16 + (e >> 4), col = tj * 16 + (e & 15);
  if (row >= M || col >= k) return;
  const double* p = ws + (size_t)blockIdx.x * chunks * 256 + e;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += p[(size_t)c * 256];
  const double sv = S[col];
  states[(size_t)row * k + col] = sv > 0.0 ? (float)(s / sv) : 0.0f;  // (a component without a singular value is a zero row)
}

// ---- out[k, D] = W[k, r] · A ---------------------------------------------------------------------------------------------------
// wave = 16 rows of W (tile blockIdx.y) x 64 columns; per step of four rows of A: one element of W (A operand) and four of A (B
// operands of the four column tiles, 16 consecutive columns each) per lane.
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(const double* __restrict__ W, int k, VRows a, int D,
                                                                   double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int c0 = (blockIdx.x * PCA_WAVES + wave) * PCA_SLAB;
  if (c0 >= D) return;  // (whole waves: no workgroup barrier below)
  const int r = a.rows, wrow = blockIdx.y * 16 + i;
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int r0 = 0; r0 < r; r0 += 4) {
    const int arow = r0 + q;
    const double w = (wrow < k && arow < r) ? W[(size_t)wrow * r + arow] : 0.0;
    double x[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = vrow_elem(a, arow, c0 + t * 16 + i, D);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, x[t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = c0 + t * 16 + i;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = blockIdx.y * 16 + q + 4 * reg;
      if (row < k && col < D) out[(size_t)row * D + col] = acc[t][reg];
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool rows_vec_ok(const VRows& v, int D) {
  if (D % 16) return false;
  if (v.u8 && v.plane % 16) return false;
  return aligned16(v.basis) && aligned16(v.u8) && aligned16(v.f32) && aligned16(v.sub) && aligned16(v.corr);
}

int frames_ok(const char* who, const uint8_t* x_u8, const float* x_f32, const float* lut, int plane, int m, int D) {
  SRLZ_REQUIRE((x_u8 != nullptr) != (x_f32 != nullptr), SRLZ_ERR_NULL, "%s: exactly one of x_u8 / x_f32 must be given", who);
  SRLZ_REQUIRE(m >= 1, SRLZ_ERR_BAD_DESC, "%s: needs at least one frame (m=%d)", who, m);
  SRLZ_REQUIRE(m <= PCA_MAX_ROWS, SRLZ_ERR_BAD_DESC, "%s: at most %d frames per call (m=%d)", who, PCA_MAX_ROWS, m);
  SRLZ_REQUIRE(D >= 1 && (long long)m * D < (1LL << 40), SRLZ_ERR_BAD_DESC, "%s: needs D >= 1 (D=%d)", who, D);
  if (x_u8) {
    SRLZ_REQUIRE(lut, SRLZ_ERR_NULL, "%s: uint8 frames need the srlz_normalize_lut table", who);
    SRLZ_REQUIRE(plane >= 1 && D % plane == 0 && (D / plane == 3 || D / plane == 6 || D / plane == 9), SRLZ_ERR_BAD_DESC,
                 "%s: uint8 frames are [m, C, plane] with C in (3, 6, 9) (D=%d, plane=%d)", who, D, plane);
  }
  return 0;
}

// The matrix of one minibatch: m centred frames (first minibatch), else [ basis ; centred frames ; correction row ].
int batch_rows(const char* who, VRows& a, const double* basis, int k, int first, const uint8_t* x_u8, const float* x_f32,
               const float* lut, int plane, int m, const double* bmean, const double* corr, int D) {
  if (int rc = frames_ok(who, x_u8, x_f32, lut, plane, m, D)) return rc;
  SRLZ_REQUIRE(bmean, SRLZ_ERR_NULL, "%s: null batch mean", who);
  SRLZ_REQUIRE(k >= 1 && k <= PCA_MAX_ROWS, SRLZ_ERR_BAD_DESC, "%s: needs 1 <= k <= %d (k=%d)", who, PCA_MAX_ROWS, k);
  SRLZ_REQUIRE(k <= D, SRLZ_ERR_BAD_DESC, "%s: n_components=%d invalid for n_features=%d", who, k, D);
  SRLZ_REQUIRE(!first || k <= m, SRLZ_ERR_BAD_DESC,
               "%s: n_components=%d must be less or equal to the batch number of samples %d for the first minibatch", who, k, m);
  SRLZ_REQUIRE(first || (basis && corr), SRLZ_ERR_NULL, "%s: a later minibatch needs the basis and the correction row", who);
  a = VRows{first ? nullptr : basis, first ? 0 : k, x_u8, x_f32, lut, plane, m, bmean, first ? nullptr : corr, first ? m : k + m + 1};
  return 0;
}

}  // namespace

extern "C" size_t srlz_pca_workspace(int rows, int D) {
  if (rows < 1 || rows > 2 * PCA_MAX_ROWS + 1 || D < 1) return 0;
  const long long T = (rows + 15) / 16;
  return T * (T + 1) / 2 <= PCA_MAX_TILES ? tile_plan(T * (T + 1) / 2, D).total : 0;
}

extern "C" size_t srlz_pca_transform_workspace(int M, int k, int D) {
  if (M < 1 || M > PCA_MAX_ROWS || k < 1 || k > PCA_MAX_ROWS || D < 1) return 0;
  const long long tiles = (long long)((M + 15) / 16) * ((k + 15) / 16);
  return tiles <= PCA_MAX_TILES ? tile_plan(tiles, D).total : 0;
}

extern "C" int srlz_pca_stats(const uint8_t* x_u8, const float* x_f32, const float* norm_lut, int plane, int m, int D,
                              long long n_seen, double* mean, double* var, double* bmean, double* corr, srlz_stream_t stream) {
  if (int rc = frames_ok("pca_stats", x_u8, x_f32, norm_lut, plane, m, D)) return rc;
  SRLZ_REQUIRE(mean && var && bmean && corr, SRLZ_ERR_NULL, "pca_stats: null pointer");
  SRLZ_REQUIRE(n_seen >= 0, SRLZ_ERR_BAD_DESC, "pca_stats: n_seen=%lld", n_seen);
  const VRows x{nullptr, 0, x_u8, x_f32, norm_lut, plane, m, nullptr, nullptr, m};
  SRLZ_LAUNCH(pca_stats_kernel, dim3((D + PCA_THREADS - 1) / PCA_THREADS), dim3(PCA_THREADS), 0, as_stream(stream), x, D, (double)n_seen,
              mean, var, bmean, corr);
  return 0;
}

extern "C" int srlz_pca_gram(const double* basis, int k, int first, const uint8_t* x_u8, const float* x_f32, const float* norm_lut,
                             int plane, int m, const double* bmean, const double* corr, int D, double* G, void* ws, size_t ws_bytes,
                             srlz_stream_t stream) {
  VRows a;
  if (int rc = batch_rows("pca_gram", a, basis, k, first, x_u8, x_f32, norm_lut, plane, m, bmean, corr, D)) return rc;
  SRLZ_REQUIRE(G && ws, SRLZ_ERR_NULL, "pca_gram: null pointer");
  const int r = a.rows, T = (r + 15) / 16;
  SRLZ_REQUIRE((long long)T * (T + 1) / 2 <= PCA_MAX_TILES, SRLZ_ERR_BAD_DESC, "pca_gram: %d rows exceed one launch's output tiles", r);
  const TilePlan p = tile_plan((long long)T * (T + 1) / 2, D);
  SRLZ_REQUIRE(ws_bytes >= p.total, SRLZ_ERR_WORKSPACE, "pca_gram: workspace %zu < %zu bytes", ws_bytes, p.total);
  const dim3 grid(p.chunks, p.tiles);
  if (rows_vec_ok(a, D))
    SRLZ_LAUNCH((pca_tiles_kernel<true, true>), grid, dim3(PCA_THREADS), 0, as_stream(stream), a, a, T, D, p.chunk_cols, (double*)ws);
  else
    SRLZ_LAUNCH((pca_tiles_kernel<false, true>), grid, dim3(PCA_THREADS), 0, as_stream(stream), a, a, T, D, p.chunk_cols, (double*)ws);
  SRLZ_LAUNCH(pca_gram_reduce_kernel, dim3(p.tiles), dim3(PCA_THREADS), 0, as_stream(stream), (const double*)ws, p.chunks, r, G);
  return 0;
}

extern "C" int srlz_pca_project(const double* W, const double* basis, int k, int first, const uint8_t* x_u8, const float* x_f32,
                                const float* norm_lut, int plane, int m, const double* bmean, const double* corr, int D, double* out,
                                srlz_stream_t stream) {
  VRows a;
  if (int rc = batch_rows("pca_project", a, basis, k, first, x_u8, x_f32, norm_lut, plane, m, bmean, corr, D)) return rc;
  SRLZ_REQUIRE(W && out, SRLZ_ERR_NULL, "pca_project: null pointer");
  SRLZ_REQUIRE(first || out != basis, SRLZ_ERR_BAD_DESC, "pca_project: the new basis must not be written over the one being read");
  const dim3 grid((D + PCA_BLOCK_COLS - 1) / PCA_BLOCK_COLS, (k + 15) / 16);
  SRLZ_LAUNCH(pca_project_kernel, grid, dim3(PCA_THREADS), 0, as_stream(stream), W, k, a, D, out);
  return 0;
}

extern "C" int srlz_pca_transform(const uint8_t* x_u8, const float* x_f32, const float* norm_lut, int plane, int M, const double* mean,
                                  const double* basis, const double* S, int k, int D, float* states, void* ws, size_t ws_bytes,
                                  srlz_stream_t stream) {
  if (int rc = frames_ok("pca_transform", x_u8, x_f32, norm_lut, plane, M, D)) return rc;
  SRLZ_REQUIRE(mean && basis && S && states && ws, SRLZ_ERR_NULL, "pca_transform: null pointer");
  SRLZ_REQUIRE(k >= 1 && k <= PCA_MAX_ROWS && k <= D, SRLZ_ERR_BAD_DESC, "pca_transform: needs 1 <= k <= min(%d, D) (k=%d, D=%d)",
               PCA_MAX_ROWS, k, D);
  const VRows a{nullptr, 0, x_u8, x_f32, norm_lut, plane, M, mean, nullptr, M};
  const VRows b{basis, k, nullptr, nullptr, nullptr, 1, 0, nullptr, nullptr, k};
  const int tm = (M + 15) / 16, tk = (k + 15) / 16;
  SRLZ_REQUIRE((long long)tm * tk <= PCA_MAX_TILES, SRLZ_ERR_BAD_DESC, "pca_transform: %d x %d output tiles exceed one launch (M=%d, k=%d)",
               tm, tk, M, k);
  const TilePlan p = tile_plan((long long)tm * tk, D);
  SRLZ_REQUIRE(ws_bytes >= p.total, SRLZ_ERR_WORKSPACE, "pca_transform: workspace %zu < %zu bytes", ws_bytes, p.total);
  const dim3 grid(p.chunks, p.tiles);
  if (rows_vec_ok(a, D) && rows_vec_ok(b, D))
    SRLZ_LAUNCH((pca_tiles_kernel<true, false>), grid, dim3(PCA_THREADS), 0, as_stream(stream), a, b, tk, D, p.chunk_cols, (double*)ws);
  else
    SRLZ_LAUNCH((pca_tiles_kernel<false, false>), grid, dim3(PCA_THREADS), 0, as_stream(stream), a, b, tk, D, p.chunk_cols, (double*)ws);
  SRLZ_LAUNCH(pca_transform_reduce_kernel, dim3(p.tiles), dim3(PCA_THREADS), 0, as_stream(stream), (const double*)ws, p.chunks, tk, M, k,
              S, states);
  return 0;
}
