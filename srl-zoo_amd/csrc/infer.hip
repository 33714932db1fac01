// infer.hip — the deployment encoder: one encoder block of models/models.py:47-63 in EVAL mode as ONE launch,
//   pooled = maxpool3x3s2( relu( conv(x) * scale + shift ) )
// The running statistics are known before the launch, so BatchNorm, ReLU and MaxPool sit in the convolution's own epilogue and the raw
// convolution output never leaves the workgroup (the training kernels must write it: they wait for batch statistics before they pool).
//
// Tiling.  A workgroup (256 threads, 4 waves) owns a TP x TP tile of POOLED outputs of one image.  Its 3x3 stride-2 windows cover
// TC x TC = (2 TP + 1)^2 convolution positions, including the one row and one column it shares with its neighbours: the overlap is
// recomputed, not exchanged (81 positions for 64 owned ones at TP = 4; a larger tile wastes less but leaves a 224 x 224 frame of batch 1
// with too few workgroups for 256 CUs: block "in" has 14 x 14 = 196 tiles per image at TP = 4, block "mid" 49, block "last" 4).
// The input patch under those positions lands in LDS once; the convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 with
// M = 96 (81 positions, padded), N = 64 output channels (16 per wave), K = taps x input channels in ONE fixed order; the epilogue
// applies the affine and the ReLU, parks the 81 x 64 activated values in LDS (over the patch) and the pooling pass reads them back.
//
// Determinism.  No atomics.  An output's sum runs over k = 0 .. K-1 in the packed order (k-group, then step, then the MFMA's own four
// k) whatever the tile, the image index or the batch size: two runs are bit-identical, row i of a batch equals that frame run alone,
// and a convolution position computed by two neighbouring tiles has the same bits in both.
#include "common.h"

namespace {

constexpr int TP = 4;             // pooled outputs per tile edge
constexpr int TC = 2 * TP + 1;    // convolution positions per tile edge
constexpr int NPOS = TC * TC;     // 81
constexpr int MB = (NPOS + 15) / 16;  // 16-row MFMA blocks over the positions (6)
constexpr int PIXP = 68;          // LDS pitch (floats) of a 64-channel pixel: 16 rows of a ds_read_b128 fall on different banks

struct InferArgs {
  const void* x;       // kind in: uint8 frames by strides; mid / last: fp32 NHWC
  const float* lut;    // kind in: srlz_normalize_lut's table
  const float* wpack;  // srlz_infer_pack_weights
  const float* bnp;    // srlz_bn_eval_params' record
  float* out;
  int N, C, HI, WI, HC, WC, HP, WP, pool_pad, out_nchw;
  long long sn, sc, sy, sx;
  int tiles_x, tiles_y, G;  // G: k-groups of 16
  int c_fastest;            // kind in: walk the patch with the channel (1) or the column (0) as the fastest index
};

__host__ __device__ constexpr int ksize_of(int kind) { return kind == SRLZ_INFER_IN ? 7 : 3; }
__host__ __device__ constexpr int stride_of(int kind) { return kind == SRLZ_INFER_MID ? 1 : 2; }
__host__ __device__ constexpr int pad_of(int kind) { return kind == SRLZ_INFER_IN ? 3 : 1; }
__host__ __device__ constexpr int patch_edge(int kind) { return (TC - 1) * stride_of(kind) + ksize_of(kind); }  // 23, 11, 19
constexpr int IN_PATCH_FLOATS = 23 * 23 * 6 + 2;  // kind in: the patch of C = 6 (rounded to 16 bytes); the k table lies behind it
constexpr int IN_KMAX = 19 * 16;                  // kind in: K = 49 C padded to whole k-groups (C = 6: 294 -> 304)

__host__ __device__ constexpr int lds_floats(int kind) {
  const int act = NPOS * 64;
  const int patch = kind == SRLZ_INFER_IN ? IN_PATCH_FLOATS + IN_KMAX : patch_edge(kind) * patch_edge(kind) * PIXP;
  return patch > act ? patch : act;
}

// wpack[((g * 64 + co) * 4 + kk) * 4 + s]: the weight of output channel co at k = (g, s, kk), the k that lane (kk = lane >> 4) feeds to
// the MFMA of step s of k-group g.  kind in: k = g*16 + s*4 + kk = tap * C + c (zero behind 49 C).  mid / last: tap = g >> 2 and
// input channel (g & 3) * 16 + kk * 4 + s: the four steps of a lane are four CONSECUTIVE channels of one pixel, one ds_read_b128.
__global__ __launch_bounds__(256) void infer_pack_kernel(const float* __restrict__ w_ref, float* __restrict__ wpack, int kind, int C,
                                                         int G) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= G * 1024) return;
  const int s = i & 3, kk = (i >> 2) & 3, co = (i >> 4) & 63, g = i >> 10;
  float v = 0.f;
  if (kind == SRLZ_INFER_IN) {
    const int k = g * 16 + s * 4 + kk;
    if (k < 49 * C) v = w_ref[(co * C + k % C) * 49 + k / C];
  } else {
    v = w_ref[(co * 64 + (g & 3) * 16 + kk * 4 + s) * 9 + (g >> 2)];
  }
  wpack[i] = v;
}

template <int KIND>
__global__ __launch_bounds__(256) void infer_block_kernel(const InferArgs a) {
  extern __shared__ __align__(16) float smem[];
  constexpr int KS = ksize_of(KIND), ST = stride_of(KIND), PD = pad_of(KIND), PE = patch_edge(KIND);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y, n = b / a.tiles_y;
  const int cy0 = 2 * ty * TP - a.pool_pad, cx0 = 2 * tx * TP - a.pool_pad;  // the tile's first convolution position
  const int iy0 = cy0 * ST - PD, ix0 = cx0 * ST - PD;                        // and the first input pixel under it
  const int C = a.C;

  // ---- the input patch -> LDS (zero outside the image: the convolution's padding) ----
  if constexpr (KIND == SRLZ_INFER_IN) {
    const uint8_t* __restrict__ x = (const uint8_t*)a.x + (size_t)n * a.sn;
    const int total = PE * PE * C;
    for (int e = tid; e < total; e += 256) {
      int c, py, px;
      if (a.c_fastest) {
        c = e % C;
        const int pix = e / C;
        py = pix / PE;
        px = pix - py * PE;
      } else {
        px = e % PE;
        const int r = e / PE;
        py = r % PE;
        c = r / PE;
      }
      const int iy = iy0 + py, ix = ix0 + px;
      float v = 0.f;
      if ((unsigned)iy < (unsigned)a.HI && (unsigned)ix < (unsigned)a.WI)
        v = a.lut[(c % 3) * 256 + x[c * a.sc + iy * a.sy + ix * a.sx]];
      smem[(py * PE + px) * C + c] = v;
    }
    // patch offset of k = (g, s, kk) at [(g * 4 + kk) * 4 + s]; a k behind 49 C (zero weight) reads the patch's first float
    int* __restrict__ koff = (int*)(smem + IN_PATCH_FLOATS);
    for (int i = tid; i < a.G * 16; i += 256) {
      const int s = i & 3, kk = (i >> 2) & 3, g = i >> 4;
      const int k = g * 16 + s * 4 + kk;
      const int tap = k < KS * KS * C ? k / C : 0, c = k < KS * KS * C ? k % C : 0;
      koff[i] = ((tap / KS) * PE + tap % KS) * C + c;
    }
  } else {
    const float* __restrict__ x = (const float*)a.x + (size_t)n * a.HI * a.WI * 64;
    for (int e = tid; e < PE * PE * 16; e += 256) {
      const int pix = e >> 4, slot = e & 15;
      const int py = pix / PE, px = pix - py * PE;
      const int iy = iy0 + py, ix = ix0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)iy < (unsigned)a.HI && (unsigned)ix < (unsigned)a.WI) v = *(const f32x4*)(x + ((size_t)iy * a.WI + ix) * 64 + slot * 4);
      *(f32x4*)(smem + pix * PIXP + slot * 4) = v;
    }
  }
  __syncthreads();

  // ---- implicit GEMM: rows = positions (lane & 15 within a block), columns = this wave's 16 output channels ----
  const int kk = lane >> 4;
  int posoff[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    int m = mb * 16 + (lane & 15);
    if (m >= NPOS) m = 0;  // (rows 81 .. 95 compute position 0 again and are dropped)
    const int r = m / TC, c = m - r * TC;
    posoff[mb] = ((r * ST) * PE + c * ST) * (KIND == SRLZ_INFER_IN ? C : PIXP);
  }
  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* __restrict__ wp = a.wpack + ((wave * 16 + (lane & 15)) * 4 + kk) * 4;
  f32x4 bw = *(const f32x4*)wp;
  for (int g = 0; g < a.G; ++g) {
    const int gn = g + 1 < a.G ? g + 1 : g;
    const f32x4 bnext = *(const f32x4*)(wp + (size_t)gn * 1024);  // the next group's weights travel behind this group's MFMAs
    f32x4 av[MB];
    if constexpr (KIND == SRLZ_INFER_IN) {
      const int4 ko = *(const int4*)((const int*)(smem + IN_PATCH_FLOATS) + (g * 4 + kk) * 4);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        av[mb][0] = smem[posoff[mb] + ko.x];
        av[mb][1] = smem[posoff[mb] + ko.y];
        av[mb][2] = smem[posoff[mb] + ko.z];
        av[mb][3] = smem[posoff[mb] + ko.w];
      }
    } else {
      const int tap = g >> 2;
      const int toff = ((tap / 3) * PE + tap % 3) * PIXP + (g & 3) * 16 + kk * 4;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) av[mb] = *(const f32x4*)(smem + posoff[mb] + toff);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb][s], bw[s], acc[mb], 0, 0, 0);
    bw = bnext;
  }
  __syncthreads();  // every wave has read its last patch value: the activated positions go over the patch

  // ---- epilogue: affine (before the max: gamma may be negative), ReLU; a position outside the map is 0, which no window's maximum
  // notices (relu >= 0 and every window holds at least one position of the map) ----
  float* __restrict__ act = smem;  // [NPOS][64]
  const int ch = wave * 16 + (lane & 15);
  const float sc = a.bnp[128 + ch], sh = a.bnp[192 + ch];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = mb * 16 + kk * 4 + j;  // C/D map of the 16x16 MFMA: row = (lane >> 4) * 4 + register, column = lane & 15
      if (m < NPOS) {
        const int r = m / TC, c = m - r * TC;
        const bool ok = (unsigned)(cy0 + r) < (unsigned)a.HC && (unsigned)(cx0 + c) < (unsigned)a.WC;
        float z = acc[mb][j] * sc + sh;  // (the arithmetic of bn_relu_pool_fwd_kernel)
        z = z > 0.f ? z : 0.f;
        act[m * 64 + ch] = ok ? z : 0.f;
      }
    }
  __syncthreads();

  // ---- the pool: a thread = one pooled output x four channels ----
  const int p = tid >> 4, c4 = tid & 15;
  const int pr = p / TP, pc = p - pr * TP;
  const int py = ty * TP + pr, px = tx * TP + pc;
  if (py < a.HP && px < a.WP) {
    f32x4 best = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const f32x4 v = *(const f32x4*)(act + ((2 * pr + ky) * TC + 2 * pc + kx) * 64 + c4 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) best[j] = v[j] > best[j] ? v[j] : best[j];
      }
    if (a.out_nchw) {
#pragma unroll
      for (int j = 0; j < 4; ++j) a.out[(((size_t)n * 64 + c4 * 4 + j) * a.HP + py) * a.WP + px] = best[j];
    } else {
      *(f32x4*)(a.out + (((size_t)n * a.HP + py) * a.WP + px) * 64 + c4 * 4) = best;
    }
  }
}

struct Dims { int hc, wc, hp, wp; };

// The one place a descriptor is judged: NULL text = supported, `dm` filled.
const char* judge(const srlz_infer_block_desc* d, Dims* dm) {
  if (!d) return "null descriptor";
  if (d->kind != SRLZ_INFER_IN && d->kind != SRLZ_INFER_MID && d->kind != SRLZ_INFER_LAST) return "kind must be 0 (in), 1 (mid) or 2 (last)";
  if (d->n < 1 || d->hi < 1 || d->wi < 1) return "n, hi and wi must be positive";
  if (d->pool_pad != 0 && d->pool_pad != 1) return "pool_pad must be 0 or 1";
  if (d->out_nchw != 0 && d->out_nchw != 1) return "out_nchw must be 0 or 1";
  if (d->kind == SRLZ_INFER_IN ? (d->c_in != 3 && d->c_in != 6) : d->c_in != 64) return "c_in must be 3 or 6 (in) or 64 (mid, last)";
  const int k = ksize_of(d->kind), s = stride_of(d->kind), p = pad_of(d->kind);
  if (d->hi + 2 * p < k || d->wi + 2 * p < k) return "the map is smaller than the convolution's window";
  dm->hc = (d->hi + 2 * p - k) / s + 1;
  dm->wc = (d->wi + 2 * p - k) / s + 1;
  if (dm->hc + 2 * d->pool_pad < 3 || dm->wc + 2 * d->pool_pad < 3) return "the pooled map would be empty";
  dm->hp = (dm->hc + 2 * d->pool_pad - 3) / 2 + 1;
  dm->wp = (dm->wc + 2 * d->pool_pad - 3) / 2 + 1;
  if (d->kind == SRLZ_INFER_IN) {
    // the four strides describe a tensor without overlap: sorted by stride, each is at least the span of the one before
    // (an axis of extent 1 is never stepped along: its stride only has to be positive)
    const long long st4[4] = {d->stride_n, d->stride_c, d->stride_y, d->stride_x};
    const long long ex4[4] = {d->n, d->c_in, d->hi, d->wi};
    long long st[4], ex[4];
    int na = 0;
    for (int i = 0; i < 4; ++i) {
      if (st4[i] < 1) return "inconsistent strides: every stride must be at least 1";
      if (ex4[i] > 1) { st[na] = st4[i]; ex[na] = ex4[i]; ++na; }
    }
    for (int i = 0; i < na; ++i)
      for (int j = i + 1; j < na; ++j)
        if (st[j] < st[i]) {
          const long long t = st[i]; st[i] = st[j]; st[j] = t;
          const long long u = ex[i]; ex[i] = ex[j]; ex[j] = u;
        }
    for (int i = 1; i < na; ++i)
      if (st[i] < st[i - 1] * ex[i - 1]) return "inconsistent strides: two elements of the frames would share a byte";
    if ((long long)d->c_in * d->stride_c + (long long)d->hi * d->stride_y + (long long)d->wi * d->stride_x >= (1LL << 31))
      return "a frame is too large for 32-bit offsets";
  } else {
    if (d->stride_c != 1 || d->stride_x != 64 || d->stride_y != 64LL * d->wi || d->stride_n != 64LL * d->wi * d->hi)
      return "inconsistent strides: a 64-channel input is contiguous NHWC (n: hi*wi*64, c: 1, y: wi*64, x: 64)";
  }
  const long long tiles = (long long)((dm->hp + TP - 1) / TP) * ((dm->wp + TP - 1) / TP) * d->n;
  if (tiles > 0x7fffffffLL) return "too many tiles for one launch";
  return nullptr;
}

template <int KIND>
int launch(const InferArgs& a, int nblocks, hipStream_t st) {
  constexpr int bytes = lds_floats(KIND) * 4;
  SRLZ_MAX_LDS(infer_block_kernel<KIND>, bytes);
  SRLZ_LAUNCH(infer_block_kernel<KIND>, dim3(nblocks), dim3(256), bytes, st, a);
  return 0;
}

int groups_of(int kind, int c_in) { return kind == SRLZ_INFER_IN ? (49 * c_in + 15) / 16 : 36; }

}  // namespace

extern "C" int srlz_infer_tile(void) { return TP; }

extern "C" int srlz_infer_block_supported(const srlz_infer_block_desc* d) {
  Dims dm;
  return judge(d, &dm) == nullptr ? 1 : 0;
}

extern "C" int srlz_infer_block_out_dims(const srlz_infer_block_desc* d, int* hc, int* wc, int* hp, int* wp) {
  Dims dm;
  const char* why = judge(d, &dm);
  SRLZ_REQUIRE(!why, SRLZ_ERR_BAD_DESC, "infer_block: %s", why);
  if (hc) *hc = dm.hc;
  if (wc) *wc = dm.wc;
  if (hp) *hp = dm.hp;
  if (wp) *wp = dm.wp;
  return 0;
}

extern "C" long long srlz_infer_packed_floats(int kind, int c_in) {
  if (kind == SRLZ_INFER_IN ? (c_in != 3 && c_in != 6) : ((kind != SRLZ_INFER_MID && kind != SRLZ_INFER_LAST) || c_in != 64)) return 0;
  return (long long)groups_of(kind, c_in) * 1024;
}

extern "C" int srlz_infer_pack_weights(const float* w_ref, float* wpack, int kind, int c_in, srlz_stream_t stream) {
  SRLZ_REQUIRE(srlz_infer_packed_floats(kind, c_in) > 0, SRLZ_ERR_BAD_DESC, "infer_pack_weights: kind %d with %d input channels", kind, c_in);
  SRLZ_REQUIRE(w_ref && wpack, SRLZ_ERR_NULL, "infer_pack_weights: null pointer");
  const int G = groups_of(kind, c_in);
  SRLZ_LAUNCH(infer_pack_kernel, dim3(G * 4), dim3(256), 0, as_stream(stream), w_ref, wpack, kind, c_in, G);
  return 0;
}

extern "C" int srlz_infer_block(const void* x, const float* norm_lut, const float* wpack, const float* bnp, float* out,
                                const srlz_infer_block_desc* d, srlz_stream_t stream) {
  Dims dm;
  const char* why = judge(d, &dm);
  SRLZ_REQUIRE(!why, SRLZ_ERR_BAD_DESC, "infer_block: %s", why);
  SRLZ_REQUIRE(x && wpack && bnp && out && (d->kind != SRLZ_INFER_IN || norm_lut), SRLZ_ERR_NULL, "infer_block: null pointer");
  InferArgs a;
  a.x = x; a.lut = norm_lut; a.wpack = wpack; a.bnp = bnp; a.out = out;
  a.N = d->n; a.C = d->c_in; a.HI = d->hi; a.WI = d->wi; a.HC = dm.hc; a.WC = dm.wc; a.HP = dm.hp; a.WP = dm.wp;
  a.pool_pad = d->pool_pad; a.out_nchw = d->out_nchw;
  a.sn = d->stride_n; a.sc = d->stride_c; a.sy = d->stride_y; a.sx = d->stride_x;
  a.tiles_x = (dm.wp + TP - 1) / TP; a.tiles_y = (dm.hp + TP - 1) / TP; a.G = groups_of(d->kind, d->c_in);
  a.c_fastest = d->stride_c < d->stride_x ? 1 : 0;
  const int nblocks = a.tiles_x * a.tiles_y * d->n;
  if (d->kind == SRLZ_INFER_IN) return launch<SRLZ_INFER_IN>(a, nblocks, as_stream(stream));
  if (d->kind == SRLZ_INFER_MID) return launch<SRLZ_INFER_MID>(a, nblocks, as_stream(stream));
  return launch<SRLZ_INFER_LAST>(a, nblocks, as_stream(stream));
}
