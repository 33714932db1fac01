// dense.hip — the two wide nn.Linear layers of the mlp / linear models on the fp32 matrix cores.
// Replaces nn.Linear(input_dim, h) / nn.Linear(h, input_dim) of the reference's models/autoencoders.py:15-20,50-64, models/vae.py:17,29,
// models/priors.py:88-91,116 with input_dim = C * 224 * 224 (150 528 / 301 056) and h = 50, 64 or state_dim: GEMMs with one enormous
// dimension K and two small ones (M = the 2 * batch images of a step, n <= 256).
//
//   in  layer:  y[M,n]   = x[M,K] . W[n,K]^T + b       (dense_in_fwd: split over K, partials summed in z order by a second launch)
//               dW[n,K]  = dy^T[n,M] . x[M,K]          (dense_in_wgrad: the reduction over M <= 1024 stays inside the tile)
//   out layer:  out[M,K] = z[M,n] . W[K,n]^T + b       (dense_out_fwd; with the reconstruction loss in the epilogue: fp64 partials per
//                                                       workgroup and frame, summed in a fixed order by srlz_pair_loss_finalize)
//               dOut     = ((g / div) * 2) * (out - target), g read from device memory
//               dW[K,n]  = dOut^T . z, db = column sums of dOut (a column of ones next to z), dz[M,n] = dOut . W (split over K)
//
// x (and the reconstruction target) come either as fp32 or as the loader's planar uint8 frames [M][C][W][H] (the flat index of
// x.view(M, -1) IS the byte offset), normalised while they are staged through the same table (srlz_normalize_lut) that
// srlz_normalize_u8_planar uses: the two routes feed identical values into identical arithmetic, so they agree bit for bit.
//
// One tile kernel serves every product: 64 x 64 output tile per workgroup, four waves = four 32 x 32 quadrants of
// v_mfma_f32_32x32x2_f32, r-steps of 32 double-buffered in LDS (the next step's global loads are in flight during this step's 16
// MFMAs per wave), loads branch-free (an element outside the matrix reads offset 0 and is zeroed when it is stashed).  No float atomics:
// every sum has one owner and a fixed order, two runs are bit-identical.  All offsets are 32-bit; srlz_dense_supported() keeps every
// operand, workspace and output below 2^31 elements, and every launcher checks it.
#include "common.h"

namespace {

constexpr int BR = 32;  // r per step
constexpr int LD = 68;  // 64 + 4 padding floats per LDS row

enum Epi { EPI_PART = 0, EPI_STORE = 1, EPI_BIAS = 2, EPI_LOSS = 3, EPI_DOUT = 4 };

struct TileArgs {
  const float* A;  // fp32 operand A (or NULL when A_U8)
  const uint8_t* A8;
  int lda;         // elements between consecutive values of A's non-contiguous index
  const float* B;
  const uint8_t* B8;
  int ldb;
  int I, J, R, rchunk;
  int plane;         // W * H of the uint8 frames (channel of flat index k = k / plane)
  int ones_col;      // >= 0: B(r, ones_col) = 1 (db as one more output column), else -1
  float* C;          // EPI_PART: [z][I][J]; EPI_STORE / EPI_BIAS / EPI_DOUT: [I][J]
  float* C2;         // EPI_STORE with ones_col: the ones column's output, [I]
  int ldc;           // columns of C (EPI_STORE with ones_col writes the first ldc columns to C)
  const float* bias;
  const float* T;    // target, fp32 [I][J]
  const uint8_t* T8;
  const float* gain;  // EPI_DOUT: device scalar g
  float div;
  int half;           // EPI_LOSS: rows < half are frame 0, the rest frame 1
  double* partial;    // EPI_LOSS: [2][gridDim.x * gridDim.y]
  const float* lut;   // [3][256]
};

// A_RC / B_RC: operand contiguous along r (else along its row / column index).  A_U8 / B_U8 / T_U8: the operand / target is uint8 frames.
template <bool A_RC, bool B_RC, bool A_U8, bool B_U8, int EPI, bool T_U8>
__global__ __launch_bounds__(256) void dense_tile_kernel(TileArgs p) {
  __shared__ float As[2][BR][LD];
  __shared__ float Bs[2][BR][LD];
  __shared__ float tab[(A_U8 || B_U8 || T_U8) ? 768 : 1];
  __shared__ double red[(EPI == EPI_LOSS) ? 8 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int wi = wave & 1, wj = wave >> 1;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int I = p.I, J = p.J;
  if (A_U8 || B_U8 || T_U8) {
    for (int e = tid; e < 768; e += 256) tab[e] = p.lut[e];
    __syncthreads();
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int rbeg = blockIdx.z * p.rchunk;
  const int rend = (rbeg + p.rchunk < p.R) ? rbeg + p.rchunk : p.R;

  constexpr int U = BR * 64 / 256;
  float va[U], vb[U];
  unsigned ina = 0, inb = 0;
  auto fetch = [&](int r0) {
    ina = inb = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = tid + 256 * u;
      int i, r;
      if (A_RC) { i = e >> 5; r = e & 31; } else { r = e >> 6; i = e & 63; }
      const bool oka = i0 + i < I && r0 + r < rend;
      const int offa = oka ? (A_RC ? (i0 + i) * p.lda + r0 + r : (r0 + r) * p.lda + i0 + i) : 0;
      if (A_U8) {
        // (channel of the flat index: the column index of x is r here)
        const unsigned k = (unsigned)(r0 + r);
        va[u] = tab[((k / (unsigned)p.plane) % 3u) * 256u + p.A8[offa]];
      } else {
        va[u] = p.A[offa];
      }
      ina |= (oka ? 1u : 0u) << u;
      int j, rb;
      if (B_RC) { j = e >> 5; rb = e & 31; } else { rb = e >> 6; j = e & 63; }
      const bool okb = j0 + j < J && r0 + rb < rend;
      const int offb = okb ? (B_RC ? (j0 + j) * p.ldb + r0 + rb : (r0 + rb) * p.ldb + j0 + j) : 0;
      if (B_U8) {
        const unsigned k = (unsigned)(j0 + j);  // (the column index of x is j here)
        vb[u] = tab[((k / (unsigned)p.plane) % 3u) * 256u + p.B8[offb]];
      } else {
        vb[u] = p.B[offb];
      }
      if (j0 + j == p.ones_col && r0 + rb < rend) vb[u] = 1.f;
      inb |= ((okb || (j0 + j == p.ones_col && r0 + rb < rend)) ? 1u : 0u) << u;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = tid + 256 * u;
      int i, r;
      if (A_RC) { i = e >> 5; r = e & 31; } else { r = e >> 6; i = e & 63; }
      As[buf][r][i] = ((ina >> u) & 1u) ? va[u] : 0.f;
      int j, rb;
      if (B_RC) { j = e >> 5; rb = e & 31; } else { rb = e >> 6; j = e & 63; }
      Bs[buf][rb][j] = ((inb >> u) & 1u) ? vb[u] : 0.f;
    }
  };
  fetch(rbeg);
  stash(0);
  __syncthreads();
  int buf = 0;
  for (int r0 = rbeg; r0 < rend; r0 += BR) {
    const bool more = r0 + BR < rend;
    if (more) fetch(r0 + BR);
#pragma unroll
    for (int s = 0; s < BR / 2; ++s) {
      const float a = As[buf][2 * s + h][wi * 32 + l31];
      const float b = Bs[buf][2 * s + h][wj * 32 + l31];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  const int j = j0 + wj * 32 + l31;
  if (EPI == EPI_PART) {
    float* __restrict__ C = p.C + (size_t)blockIdx.z * I * J;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (i < I && j < J) C[i * J + j] = acc[r];
    }
  } else if (EPI == EPI_STORE) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (i < I && j < p.ldc) p.C[i * p.ldc + j] = acc[r];
      else if (i < I && j == p.ones_col) p.C2[i] = acc[r];
    }
  } else {
    float bj = p.bias ? p.bias[j < J ? j : 0] : 0.f;
    asm volatile("" : "+v"(bj));  // waited for once, here, not behind every store of the loop below (tools/isa_audit.py)
    // (the column's channel in the target frames; one per lane)
    const unsigned tc = T_U8 ? (((unsigned)(j < J ? j : 0) / (unsigned)p.plane) % 3u) * 256u : 0u;
    float gd = 0.f;
    if (EPI == EPI_DOUT) gd = (p.gain[0] / p.div) * 2.0f;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (i < I && j < J) {
        const float v = acc[r] + bj;
        if (EPI == EPI_BIAS) {
          p.C[i * J + j] = v;
        } else {
          const float t = T_U8 ? tab[tc + p.T8[i * J + j]] : p.T[i * J + j];
          const float d = v - t;
          if (EPI == EPI_DOUT) {
            p.C[i * J + j] = gd * d;
          } else {
            const double dd = (double)d * (double)d;
            if (i < p.half) s0 += dd; else s1 += dd;
          }
        }
      }
    }
    if (EPI == EPI_LOSS) {
      s0 = wave_sum_d(s0);
      s1 = wave_sum_d(s1);
      if (lane == 0) { red[2 * wave] = s0; red[2 * wave + 1] = s1; }
      __syncthreads();
      if (tid == 0) {
        const int nb = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
        p.partial[wg] = ((red[0] + red[2]) + red[4]) + red[6];
        p.partial[nb + wg] = ((red[1] + red[3]) + red[5]) + red[7];
      }
    }
  }
}

// out[i][j] = act(bias[j] + sum_z part[z][i][j]), z in order (act: 0 none, 1 ReLU, 2 tanh)
__global__ __launch_bounds__(256) void splitk_sum_kernel(const float* __restrict__ part, int Z, int I, int J,
                                                         const float* __restrict__ bias, int act, float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= I * J) return;
  float s = part[e];
  for (int z = 1; z < Z; ++z) s += part[z * I * J + e];
  if (bias) s += bias[e % J];
  if (act == 1) s = s > 0.f ? s : 0.f;
  else if (act == 2) s = tanhf(s);
  out[e] = s;
}

// out[c] = sum_r a[r][c], r in order (the bias gradient of the in layer: a = dy [M][n])
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, int rows, int cols, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += a[r * cols + c];
  out[c] = s;
}

__global__ __launch_bounds__(256) void tanh_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) y[e] = tanhf(x[e]);
}

// dx = (1 - y^2) * dy (torch's tanh_backward)
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                                       int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) {
    const float v = y[e];
    dx[e] = dy[e] * (1.f - v * v);
  }
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = a[e] + b[e];
}

constexpr long long LIM = 1LL << 31;

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// split of a reduction of length R over the output tiles: enough workgroups for every CU (about 1024 = four per CU), r-chunks of whole steps
inline int rchunk_for(int tiles, int R) {
  const int want = tiles >= 1024 ? 1 : cdiv(1024, tiles);
  const int steps = cdiv(R, BR);
  const int per = cdiv(steps, want < steps ? want : steps);
  return per * BR;
}

template <bool A_RC, bool B_RC, bool A_U8, bool B_U8, int EPI, bool T_U8>
int launch_tile(const TileArgs& a, int z, hipStream_t st) {
  SRLZ_LAUNCH((dense_tile_kernel<A_RC, B_RC, A_U8, B_U8, EPI, T_U8>), dim3(cdiv(a.J + (a.ones_col >= 0 ? 1 : 0), 64), cdiv(a.I, 64), z),
              dim3(256), 0, st, a);
  return 0;
}

TileArgs blank() {
  TileArgs a;
  a.A = nullptr; a.A8 = nullptr; a.lda = 0; a.B = nullptr; a.B8 = nullptr; a.ldb = 0;
  a.I = a.J = a.R = a.rchunk = 0; a.plane = 1; a.ones_col = -1;
  a.C = nullptr; a.C2 = nullptr; a.ldc = 0; a.bias = nullptr; a.T = nullptr; a.T8 = nullptr; a.gain = nullptr; a.div = 1.f;
  a.half = 0; a.partial = nullptr; a.lut = nullptr;
  return a;
}

// split of the in layer's forward / the out layer's data gradient: Z partial [M][n] matrices
inline int in_split(int M, int n, int K, int* rchunk) {
  const int rc = rchunk_for(cdiv(M, 64) * cdiv(n, 64), K);
  if (rchunk) *rchunk = rc;
  return cdiv(K, rc);
}

}  // namespace

extern "C" int srlz_dense_supported(int M, int n, int K, int plane) {
  SRLZ_REQUIRE(M >= 1 && n >= 1 && n <= 256, 0, "dense: M = %d must be >= 1 and n = %d in [1, 256]", M, n);
  SRLZ_REQUIRE(plane >= 1 && K >= plane && K % plane == 0 && (K / plane == 3 || K / plane == 6), 0,
               "dense: K = %d must be 3 or 6 planes of %d", K, plane);
  // every 32-bit offset of the kernels: x / out / dOut [M][K], W [n][K] (+ the ones column), split partials [Z][M][n]
  SRLZ_REQUIRE((long long)M * K < LIM && (long long)(n + 1) * K < LIM, 0, "dense: M * K = %lld exceeds the 32-bit offsets",
               (long long)M * K);
  const long long z = in_split(M, n, K, nullptr);
  SRLZ_REQUIRE(z * M * n < LIM, 0, "dense: split-K partials exceed the 32-bit offsets");
  return 1;
}

extern "C" size_t srlz_dense_in_workspace(int M, int n, int K) {
  if (M < 1 || n < 1 || K < 1) return 0;
  return (size_t)in_split(M, n, K, nullptr) * M * n * sizeof(float);
}

extern "C" int srlz_dense_in_fwd(const float* x, const uint8_t* x_u8, const float* lut, const float* w, const float* b, float* y, int M,
                                 int n, int K, int plane, int act, void* ws, size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE((x || (x_u8 && lut)) && w && y && ws, SRLZ_ERR_NULL, "dense_in_fwd: null pointer");
  if (!srlz_dense_supported(M, n, K, plane)) return SRLZ_ERR_BAD_DESC;
  SRLZ_REQUIRE(act >= 0 && act <= 2, SRLZ_ERR_BAD_DESC, "dense_in_fwd: act = %d", act);
  SRLZ_REQUIRE(ws_bytes >= srlz_dense_in_workspace(M, n, K), SRLZ_ERR_BAD_DESC, "dense_in_fwd: workspace too small");
  int rc = 0;
  const int Z = in_split(M, n, K, &rc);
  TileArgs a = blank();
  a.A = x; a.A8 = x_u8; a.lda = K; a.B = w; a.ldb = K;
  a.I = M; a.J = n; a.R = K; a.rchunk = rc; a.plane = plane; a.C = (float*)ws; a.lut = lut;
  hipStream_t st = as_stream(stream);
  const int e = x ? launch_tile<true, true, false, false, EPI_PART, false>(a, Z, st)
                  : launch_tile<true, true, true, false, EPI_PART, false>(a, Z, st);
  if (e) return e;
  SRLZ_LAUNCH(splitk_sum_kernel, dim3(cdiv((long long)M * n, 256)), dim3(256), 0, st, (const float*)ws, Z, M, n, b, act, y);
  return 0;
}

extern "C" int srlz_dense_in_wgrad(const float* dy, const float* x, const uint8_t* x_u8, const float* lut, float* dw, float* db, int M,
                                   int n, int K, int plane, srlz_stream_t stream) {
  SRLZ_REQUIRE(dy && (x || (x_u8 && lut)) && dw, SRLZ_ERR_NULL, "dense_in_wgrad: null pointer");
  if (!srlz_dense_supported(M, n, K, plane)) return SRLZ_ERR_BAD_DESC;
  TileArgs a = blank();
  // dW[j][k] = sum_m dy[m][j] x[m][k]: i = j (A = dy, contiguous along i), j = k (B = x, contiguous along k), r = m
  a.A = dy; a.lda = n; a.B = x; a.B8 = x_u8; a.ldb = K;
  a.I = n; a.J = K; a.R = M; a.rchunk = cdiv(M, BR) * BR; a.plane = plane; a.C = dw; a.ldc = K; a.lut = lut;
  hipStream_t st = as_stream(stream);
  const int e = x ? launch_tile<false, false, false, false, EPI_STORE, false>(a, 1, st)
                  : launch_tile<false, false, false, true, EPI_STORE, false>(a, 1, st);
  if (e) return e;
  if (db) {
    SRLZ_LAUNCH(colsum_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dy, M, n, db);
  }
  return 0;
}

namespace {
TileArgs out_args(const float* z, const float* w, const float* b, int M, int n, int K, int plane) {
  TileArgs a = blank();
  // out[m][k] = sum_j z[m][j] W[k][j] + b[k]: i = m, j = k, r = j (both operands contiguous along r)
  a.A = z; a.lda = n; a.B = w; a.ldb = n;
  a.I = M; a.J = K; a.R = n; a.rchunk = cdiv(n, BR) * BR; a.plane = plane; a.bias = b;
  return a;
}
}  // namespace

extern "C" int srlz_dense_out_fwd(const float* z, const float* w, const float* b, float* out, int M, int n, int K, int plane,
                                  srlz_stream_t stream) {
  SRLZ_REQUIRE(z && w && out, SRLZ_ERR_NULL, "dense_out_fwd: null pointer");
  if (!srlz_dense_supported(M, n, K, plane)) return SRLZ_ERR_BAD_DESC;
  TileArgs a = out_args(z, w, b, M, n, K, plane);
  a.C = out;
  return launch_tile<true, true, false, false, EPI_BIAS, false>(a, 1, as_stream(stream));
}

extern "C" int srlz_dense_out_fwd_loss_workgroups(int M, int K) {
  if (M < 1 || K < 1) return -1;
  return cdiv(M, 64) * cdiv(K, 64);
}

extern "C" int srlz_dense_out_fwd_loss(const float* z, const float* w, const float* b, const float* target, const uint8_t* target_u8,
                                       const float* lut, double* partial, int M, int n, int K, int plane, int half,
                                       srlz_stream_t stream) {
  SRLZ_REQUIRE(z && w && (target || (target_u8 && lut)) && partial, SRLZ_ERR_NULL, "dense_out_fwd_loss: null pointer");
  if (!srlz_dense_supported(M, n, K, plane)) return SRLZ_ERR_BAD_DESC;
  SRLZ_REQUIRE(half >= 0 && half <= M, SRLZ_ERR_BAD_DESC, "dense_out_fwd_loss: half = %d of M = %d", half, M);
  TileArgs a = out_args(z, w, b, M, n, K, plane);
  a.T = target; a.T8 = target_u8; a.lut = lut; a.partial = partial; a.half = half;
  hipStream_t st = as_stream(stream);
  return target ? launch_tile<true, true, false, false, EPI_LOSS, false>(a, 1, st)
                : launch_tile<true, true, false, false, EPI_LOSS, true>(a, 1, st);
}

namespace {
// dW[k][j] = sum_m dOut[m][k] z[m][j], db[k] = sum_m dOut[m][k] (output column n: a column of ones next to z) and, when dz is
// non-NULL, dz[m][j] = sum_k dOut[m][k] W[k][j] split over K with the partials (part) summed in z order
int out_grads(const float* dout, const float* z, const float* w, float* dz, float* dw, float* db, int M, int n, int K, float* part,
              hipStream_t st) {
  TileArgs g = blank();
  g.A = dout; g.lda = K; g.B = z; g.ldb = n;
  g.I = K; g.J = n; g.R = M; g.rchunk = cdiv(M, BR) * BR; g.ones_col = n; g.C = dw; g.C2 = db; g.ldc = n;
  int e = launch_tile<false, false, false, false, EPI_STORE, false>(g, 1, st);
  if (e) return e;
  if (dz) {
    int rc = 0;
    const int Z = in_split(M, n, K, &rc);
    TileArgs d = blank();
    d.A = dout; d.lda = K; d.B = w; d.ldb = n;
    d.I = M; d.J = n; d.R = K; d.rchunk = rc; d.C = part;
    e = launch_tile<true, false, false, false, EPI_PART, false>(d, Z, st);
    if (e) return e;
    SRLZ_LAUNCH(splitk_sum_kernel, dim3(cdiv((long long)M * n, 256)), dim3(256), 0, st, (const float*)part, Z, M, n, (const float*)nullptr,
                0, dz);
  }
  return 0;
}
}  // namespace

extern "C" size_t srlz_dense_out_bwd_workspace(int M, int n, int K) {
  if (M < 1 || n < 1 || K < 1) return 0;
  // dOut [M][K], then the data gradient's split partials [Z][M][n]
  return (size_t)M * K * sizeof(float) + srlz_dense_in_workspace(M, n, K);
}

extern "C" int srlz_dense_out_bwd(const float* z, const float* w, const float* b, const float* target, const uint8_t* target_u8,
                                  const float* lut, const float* gain, float div, float* dz, float* dw, float* db, int M, int n, int K,
                                  int plane, void* ws, size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE(z && w && (target || (target_u8 && lut)) && gain && dw && db && ws, SRLZ_ERR_NULL, "dense_out_bwd: null pointer");
  if (!srlz_dense_supported(M, n, K, plane)) return SRLZ_ERR_BAD_DESC;
  SRLZ_REQUIRE(div > 0.f && ws_bytes >= srlz_dense_out_bwd_workspace(M, n, K), SRLZ_ERR_BAD_DESC,
               "dense_out_bwd: div = %g, workspace %zu bytes", div, ws_bytes);
  hipStream_t st = as_stream(stream);
  float* dout = (float*)ws;
  float* part = dout + (size_t)M * K;
  // 1. dOut = ((g / div) * 2) * (z W^T + b - target), the output recomputed tile by tile
  TileArgs a = out_args(z, w, b, M, n, K, plane);
  a.T = target; a.T8 = target_u8; a.lut = lut; a.gain = gain; a.div = div; a.C = dout;
  const int e = target ? launch_tile<true, true, false, false, EPI_DOUT, false>(a, 1, st)
                       : launch_tile<true, true, false, false, EPI_DOUT, true>(a, 1, st);
  if (e) return e;
  // 2. / 3. the weight, bias and data gradients from dOut
  return out_grads(dout, z, w, dz, dw, db, M, n, K, part, st);
}

extern "C" int srlz_dense_out_bwd_from(const float* dout, const float* z, const float* w, float* dz, float* dw, float* db, int M, int n,
                                       int K, int plane, void* ws, size_t ws_bytes, srlz_stream_t stream) {
  SRLZ_REQUIRE(dout && z && w && dw && db && ws, SRLZ_ERR_NULL, "dense_out_bwd_from: null pointer");
  if (!srlz_dense_supported(M, n, K, plane)) return SRLZ_ERR_BAD_DESC;
  SRLZ_REQUIRE(ws_bytes >= srlz_dense_in_workspace(M, n, K), SRLZ_ERR_BAD_DESC, "dense_out_bwd_from: workspace %zu bytes", ws_bytes);
  return out_grads(dout, z, w, dz, dw, db, M, n, K, (float*)ws, as_stream(stream));
}

extern "C" int srlz_tanh_fwd(const float* x, float* y, int n, srlz_stream_t stream) {
  SRLZ_REQUIRE(x && y, SRLZ_ERR_NULL, "tanh_fwd: null pointer");
  SRLZ_REQUIRE(n >= 1, SRLZ_ERR_BAD_DESC, "tanh_fwd: n = %d", n);
  SRLZ_LAUNCH(tanh_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, y, n);
  return 0;
}

extern "C" int srlz_tanh_bwd(const float* y, const float* dy, float* dx, int n, srlz_stream_t stream) {
  SRLZ_REQUIRE(y && dy && dx, SRLZ_ERR_NULL, "tanh_bwd: null pointer");
  SRLZ_REQUIRE(n >= 1, SRLZ_ERR_BAD_DESC, "tanh_bwd: n = %d", n);
  SRLZ_LAUNCH(tanh_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), y, dy, dx, n);
  return 0;
}

extern "C" int srlz_add_f32(const float* a, const float* b, float* out, int n, srlz_stream_t stream) {
  SRLZ_REQUIRE(a && b && out, SRLZ_ERR_NULL, "add_f32: null pointer");
  SRLZ_REQUIRE(n >= 1, SRLZ_ERR_BAD_DESC, "add_f32: n = %d", n);
  SRLZ_LAUNCH(add_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), a, b, out, n);
  return 0;
}
