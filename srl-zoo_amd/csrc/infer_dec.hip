// infer_dec.hip — the deployment decoder: decoder_conv of models/models.py:65-83 in EVAL mode, one launch per layer.
//   block (kinds FIRST, MID):  h = relu( (convT3x3s2(x) + b) * scale + shift )     64 -> 64, out = 2 in + 1
//   out   (kind OUT):          y = convT4x4s2(x) + b                               64 -> C in {3, 6}, out = 2 in + 2
// nn.ConvTranspose2d scatters: out[n,co,2iy+ky,2ix+kx] += x[n,ci,iy,ix] * w[ci,co,ky,kx].  Both kernels GATHER instead: a cell (cy, cx)
// owns the outputs (2cy .. 2cy+1, 2cx .. 2cx+1), one per parity class (oy & 1, ox & 1), and every tap of the filter feeds exactly one
// class from the cell's own pixel or its upper / left neighbour (ky = 2 or 3 reaches back one row: dy = ky >> 1).  No atomics, and the
// raw ConvTranspose output of a block never exists: bias, BatchNorm affine and ReLU are applied to the accumulators.
//
// Block kernel.  The 3x3 filter gives the classes (even, even) 2x2 taps, (even, odd) 2x1, (odd, even) 1x2 and (odd, odd) 1x1: nine taps,
// K = 64 each.  A workgroup (256 threads, 4 waves) owns TD x TD = 16 cells of one image = ONE 16-row MFMA block per class; the (TD + 1)^2
// input pixels under it land in LDS once, zero outside the map.  Implicit GEMM on v_mfma_f32_16x16x4_f32: rows = cells, columns = the
// wave's 16 output channels, k-groups of 16 in the order (tap, channel group), each feeding its tap's class; weights from a private
// packing (the layout of infer.hip: a lane's four k-steps are one 16-byte load and four consecutive channels of one LDS pixel), the next
// group's weights loaded behind the current group's MFMAs.  The cell grid of an hi x wi map is (hi + 1) x (wi + 1): the last cell row owns
// output row 2 hi only.  TD = 4 is the batch-1 choice.
//
// Out kernel.  Every output of the 4x4 stride-2 layer has exactly 2x2 taps (ky = py + 2 dy), K = 256, and only C <= 6 columns: an MFMA
// would idle 10 of its 16 columns, and the layer is 77 MFLOP per 224 x 224 x 3 picture against 3.1 MB of input, so it is plain fp32 FMA,
// output-stationary.  A workgroup owns TO x TO = 64 cells; wave w computes parity class w of all of them (lane = cell), so the weights of
// a wave are uniform and every lane reads only its own four pixels from LDS.  The epilogue writes the decode tensor fp32 [N,C,ho,wo] or
// the picture as bytes by four element strides (planar [N,C,W,H] and camera [N,H,W,C] frames are one kernel), with the byte arithmetic
// of latent.hip: x * std, + mean rounded separately, clip, rint(x * 255), NaN -> 0.
//
// Determinism.  An output's sum has one order — its class's taps in table order, channels ascending — whatever n, N or the tile.
#include <math.h>

#include "common.h"

namespace {

constexpr int TD = 4;        // block kernel: cells per tile edge
constexpr int PD = TD + 1;   // staged pixels per tile edge (the cells and their upper / left neighbours)
constexpr int TO = 8;        // out kernel: cells per tile edge (64 cells = the lanes of a wave)
constexpr int PO = TO + 1;
constexpr int PIXP = 68;     // LDS pitch (floats) of a 64-channel pixel, as in infer.hip
constexpr int GROUPS = 36;   // block kernel: 9 taps x 4 channel groups of 16

// the nine taps of the 3x3 filter in class order: (ee) 00 02 20 22, (eo) 01 21, (oe) 10 12, (oo) 11
__host__ __device__ constexpr int tap_ky(int t) { return t < 2 ? 0 : t < 4 ? 2 : t < 5 ? 0 : t < 6 ? 2 : 1; }
__host__ __device__ constexpr int tap_kx(int t) { return t < 4 ? (t & 1) * 2 : t < 6 ? 1 : t < 8 ? (t - 6) * 2 : 1; }
__host__ __device__ constexpr int tap_cls(int t) { return ((tap_ky(t) & 1) << 1) | (tap_kx(t) & 1); }

struct DecArgs {
  const float* x;
  const float* wpack;
  const float* bias;
  const float* bnp;  // block kinds: srlz_bn_eval_params' record
  void* out;
  int N, HI, WI, HO, WO, tiles_x, tiles_y, out_u8, bgr;
  long long sn, sc, sy, sx;  // byte output: element strides
};

// block: wpack[((g * 64 + co) * 4 + kk) * 4 + s] = w[ci = (g & 3) * 16 + kk * 4 + s][co][tap g >> 2]
// out:   wpack[((cls * 4 + tap) * 64 + ci) * CP + co] = w[ci][co][ky = (cls >> 1) + 2 (tap >> 1)][kx = (cls & 1) + 2 (tap & 1)], CP = 4 or 8
__global__ __launch_bounds__(256) void infer_dec_pack_kernel(const float* __restrict__ w_ref, float* __restrict__ wpack, int kind,
                                                             int c_out, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = 0.f;
  if (kind != SRLZ_INFER_DEC_OUT) {
    const int s = i & 3, kk = (i >> 2) & 3, co = (i >> 4) & 63, g = i >> 10, t = g >> 2;
    v = w_ref[(((g & 3) * 16 + kk * 4 + s) * 64 + co) * 9 + tap_ky(t) * 3 + tap_kx(t)];
  } else {
    const int cp = c_out == 3 ? 4 : 8;
    const int co = i % cp, ci = (i / cp) & 63, tap = (i / (cp * 64)) & 3, cls = i / (cp * 256);
    if (co < c_out) v = w_ref[(ci * c_out + co) * 16 + ((cls >> 1) + 2 * (tap >> 1)) * 4 + (cls & 1) + 2 * (tap & 1)];
  }
  wpack[i] = v;
}

template <int KIND>
__global__ __launch_bounds__(256) void infer_dec_block_kernel(const DecArgs a) {
  __shared__ __align__(16) float smem[PD * PD * PIXP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y, n = b / a.tiles_y;
  const int cy0 = ty * TD, cx0 = tx * TD;  // the tile's first cell; patch pixel (py, px) is input (cy0 - 1 + py, cx0 - 1 + px)

  // ---- the input pixels under the tile -> LDS (zero outside the map) ----
  if constexpr (KIND == SRLZ_INFER_DEC_FIRST) {
    const float* __restrict__ x = a.x + (size_t)n * 64 * a.HI * a.WI;  // [64, hi, wi], as the Linear layer writes it
    for (int e = tid; e < PD * PD * 64; e += 256) {
      const int px = e % PD, r = e / PD;
      const int py = r % PD, c = r / PD;
      const int iy = cy0 - 1 + py, ix = cx0 - 1 + px;
      float v = 0.f;
      if ((unsigned)iy < (unsigned)a.HI && (unsigned)ix < (unsigned)a.WI) v = x[((size_t)c * a.HI + iy) * a.WI + ix];
      smem[(py * PD + px) * PIXP + c] = v;
    }
  } else {
    const float* __restrict__ x = a.x + (size_t)n * a.HI * a.WI * 64;
    for (int e = tid; e < PD * PD * 16; e += 256) {
      const int pix = e >> 4, slot = e & 15;
      const int py = pix / PD, px = pix - py * PD;
      const int iy = cy0 - 1 + py, ix = cx0 - 1 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)iy < (unsigned)a.HI && (unsigned)ix < (unsigned)a.WI) v = *(const f32x4*)(x + ((size_t)iy * a.WI + ix) * 64 + slot * 4);
      *(f32x4*)(smem + pix * PIXP + slot * 4) = v;
    }
  }
  __syncthreads();

  // ---- implicit GEMM: rows = the 16 cells (lane & 15), columns = this wave's 16 output channels, one accumulator per class ----
  const int kk = lane >> 4, m = lane & 15;
  const int base = ((m / TD + 1) * PD + m % TD + 1) * PIXP + kk * 4;  // the cell's own pixel, this lane's four channels of a group
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* __restrict__ wp = a.wpack + ((wave * 16 + m) * 4 + kk) * 4;
  f32x4 bw = *(const f32x4*)wp;
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {
    const int gn = g + 1 < GROUPS ? g + 1 : g;
    const f32x4 bnext = *(const f32x4*)(wp + (size_t)gn * 1024);  // the next group's weights travel behind this group's MFMAs
    const int t = g >> 2, cls = tap_cls(t);
    const f32x4 av = *(const f32x4*)(smem + base - ((tap_ky(t) >> 1) * PD + (tap_kx(t) >> 1)) * PIXP + (g & 3) * 16);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bw[s], acc[cls], 0, 0, 0);
    bw = bnext;
  }

  // ---- epilogue: bias, affine, ReLU in registers; C/D map of the MFMA: row = (lane >> 4) * 4 + register, column = lane & 15 ----
  const int ch = wave * 16 + m;
  const float bi = a.bias[ch], sc = a.bnp[128 + ch], sh = a.bnp[192 + ch];
  float* __restrict__ out = (float*)a.out + (size_t)n * a.HO * a.WO * 64;
#pragma unroll
  for (int cls = 0; cls < 4; ++cls)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cell = kk * 4 + j;
      const int oy = 2 * (cy0 + cell / TD) + (cls >> 1), ox = 2 * (cx0 + cell % TD) + (cls & 1);
      if (oy < a.HO && ox < a.WO) {
        float z = (acc[cls][j] + bi) * sc + sh;  // (the expression of infer_block_kernel behind the bias)
        z = z > 0.f ? z : 0.f;
        out[((size_t)oy * a.WO + ox) * 64 + ch] = z;
      }
    }
}

// deNormalize(x, "image_net") of one value of channel k (0 = R), then the byte: the arithmetic of latent.hip.  Product and sum are two
// separately rounded fp32 operations (numpy's x *= std; x += mean), so contraction is switched off for these two functions.
__device__ __forceinline__ float dec_denormalize(float v, int k) {
#pragma clang fp contract(off)
  const float sd = k == 0 ? 0.229f : (k == 1 ? 0.224f : 0.225f);
  const float mn = k == 0 ? 0.485f : (k == 1 ? 0.456f : 0.406f);
  const float p = v * sd;  // (spelled as operators: the pragma reaches only what stands in this function)
  float r = p + mn;
  if (r != r) return r;
  r = r > 0.f ? r : 0.f;
  return r < 1.f ? r : 1.f;
}

__device__ __forceinline__ unsigned char dec_byte(float v) {
#pragma clang fp contract(off)
  const float s = rintf(v * 255.f);
  return s == s ? (unsigned char)(int)s : (unsigned char)0;
}

template <int C>
__global__ __launch_bounds__(256) void infer_dec_out_kernel(const DecArgs a) {
  __shared__ __align__(16) float smem[PO * PO * PIXP];
  constexpr int CP = C == 3 ? 4 : 8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int cls = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's parity class: its weights are uniform
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y, n = b / a.tiles_y;
  const int cy0 = ty * TO, cx0 = tx * TO;
  const float* __restrict__ x = a.x + (size_t)n * a.HI * a.WI * 64;
  for (int e = tid; e < PO * PO * 16; e += 256) {
    const int pix = e >> 4, slot = e & 15;
    const int py = pix / PO, px = pix - py * PO;
    const int iy = cy0 - 1 + py, ix = cx0 - 1 + px;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)iy < (unsigned)a.HI && (unsigned)ix < (unsigned)a.WI) v = *(const f32x4*)(x + ((size_t)iy * a.WI + ix) * 64 + slot * 4);
    *(f32x4*)(smem + pix * PIXP + slot * 4) = v;
  }
  __syncthreads();

  const int r = lane >> 3, c = lane & 7;
  float acc[C];
#pragma unroll
  for (int co = 0; co < C; ++co) acc[co] = 0.f;
  const float* __restrict__ w = a.wpack + (size_t)cls * 4 * 64 * CP;
#pragma unroll
  for (int tap = 0; tap < 4; ++tap) {
    const float* xp = smem + ((r + 1 - (tap >> 1)) * PO + c + 1 - (tap & 1)) * PIXP;
    const float* __restrict__ wt = w + tap * 64 * CP;
#pragma unroll 2
    for (int q = 0; q < 16; ++q) {
      const f32x4 xv = *(const f32x4*)(xp + q * 4);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int co = 0; co < C; ++co) acc[co] = fmaf(xv[s], wt[(q * 4 + s) * CP + co], acc[co]);
    }
  }

  const int oy = 2 * (cy0 + r) + (cls >> 1), ox = 2 * (cx0 + c) + (cls & 1);
  if (oy >= a.HO || ox >= a.WO) return;
#pragma unroll
  for (int co = 0; co < C; ++co) {
    const float d = acc[co] + a.bias[co];
    if (!a.out_u8) {
      ((float*)a.out)[(((size_t)n * C + co) * a.HO + oy) * a.WO + ox] = d;
    } else {
      const int cam = co / 3, k = co - cam * 3;
      const int cd = a.bgr ? cam * 3 + 2 - k : co;
      ((unsigned char*)a.out)[(long long)n * a.sn + cd * a.sc + oy * a.sy + ox * a.sx] = dec_byte(dec_denormalize(d, k));
    }
  }
}

struct Dims { int ho, wo, tiles_x, tiles_y; };

// The one place a descriptor is judged: NULL text = supported, `dm` filled.
const char* judge(const srlz_infer_dec_desc* d, Dims* dm) {
  if (!d) return "null descriptor";
  if (d->kind != SRLZ_INFER_DEC_FIRST && d->kind != SRLZ_INFER_DEC_MID && d->kind != SRLZ_INFER_DEC_OUT)
    return "kind must be 0 (first), 1 (mid) or 2 (out)";
  const bool is_out = d->kind == SRLZ_INFER_DEC_OUT;
  if (d->n < 1 || d->hi < 1 || d->wi < 1) return "n, hi and wi must be positive (an empty map)";
  if (d->hi > (1 << 29) || d->wi > (1 << 29)) return "a map edge beyond 2^29";
  if (d->c_in != 64) return "c_in must be 64";
  if (is_out ? (d->c_out != 3 && d->c_out != 6) : d->c_out != 64) return "c_out must be 64 (first, mid) or 3 or 6 (out)";
  if ((d->out_u8 != 0 && d->out_u8 != 1) || (d->bgr != 0 && d->bgr != 1)) return "out_u8 and bgr must be 0 or 1";
  if (d->out_u8 && !is_out) return "only kind out writes bytes";
  const long long hi = d->hi, wi = d->wi;
  if (d->kind == SRLZ_INFER_DEC_FIRST) {
    if (d->in_stride_n != 64 * hi * wi || d->in_stride_c != hi * wi || d->in_stride_y != wi || d->in_stride_x != 1)
      return "inconsistent input strides: kind first reads contiguous [N,64,hi,wi] (n: 64*hi*wi, c: hi*wi, y: wi, x: 1)";
  } else if (d->in_stride_n != 64 * hi * wi || d->in_stride_c != 1 || d->in_stride_y != 64 * wi || d->in_stride_x != 64) {
    return "inconsistent input strides: kinds mid and out read contiguous NHWC (n: hi*wi*64, c: 1, y: wi*64, x: 64)";
  }
  const int add = is_out ? 2 : 1, tile = is_out ? TO : TD;
  dm->ho = 2 * d->hi + add;
  dm->wo = 2 * d->wi + add;
  dm->tiles_y = (d->hi + 1 + tile - 1) / tile;  // the cell grid is (hi + 1) x (wi + 1)
  dm->tiles_x = (d->wi + 1 + tile - 1) / tile;
  if ((long long)dm->tiles_x * dm->tiles_y * d->n > 0x7fffffffLL) return "too many tiles for one launch (beyond 2^31 - 1)";
  if (d->out_u8) {
    // the four strides describe a tensor without overlap: sorted by stride, each is at least the span of the one before
    // (an axis of extent 1 is never stepped along: its stride only has to be positive)
    const long long st4[4] = {d->out_stride_n, d->out_stride_c, d->out_stride_y, d->out_stride_x};
    const long long ex4[4] = {d->n, d->c_out, dm->ho, dm->wo};
    long long st[4], ex[4];
    int na = 0;
    for (int i = 0; i < 4; ++i) {
      if (st4[i] < 1) return "inconsistent output strides: every stride must be at least 1";
      if (ex4[i] > 1) { st[na] = st4[i]; ex[na] = ex4[i]; ++na; }
    }
    for (int i = 0; i < na; ++i)
      for (int j = i + 1; j < na; ++j)
        if (st[j] < st[i]) {
          const long long t = st[i]; st[i] = st[j]; st[j] = t;
          const long long u = ex[i]; ex[i] = ex[j]; ex[j] = u;
        }
    for (int i = 1; i < na; ++i)
      if (st[i] < st[i - 1] * ex[i - 1]) return "inconsistent output strides: two elements of the frames would share a byte";
    if ((long long)d->c_out * d->out_stride_c + (long long)dm->ho * d->out_stride_y + (long long)dm->wo * d->out_stride_x >= (1LL << 31))
      return "a frame is too large for 32-bit offsets (beyond 2^31 - 1)";
  }
  return nullptr;
}

DecArgs make_args(const float* x, const float* wpack, const float* bias, const float* bnp, void* out, const srlz_infer_dec_desc* d,
                  const Dims& dm) {
  DecArgs a;
  a.x = x; a.wpack = wpack; a.bias = bias; a.bnp = bnp; a.out = out;
  a.N = d->n; a.HI = d->hi; a.WI = d->wi; a.HO = dm.ho; a.WO = dm.wo; a.tiles_x = dm.tiles_x; a.tiles_y = dm.tiles_y;
  a.out_u8 = d->out_u8; a.bgr = d->bgr;
  a.sn = d->out_stride_n; a.sc = d->out_stride_c; a.sy = d->out_stride_y; a.sx = d->out_stride_x;
  return a;
}

long long packed_floats(int kind, int c_out) {
  if (kind == SRLZ_INFER_DEC_FIRST || kind == SRLZ_INFER_DEC_MID) return c_out == 64 ? (long long)GROUPS * 1024 : 0;
  if (kind == SRLZ_INFER_DEC_OUT) return c_out == 3 ? 16 * 64 * 4 : (c_out == 6 ? 16 * 64 * 8 : 0);
  return 0;
}

}  // namespace

extern "C" int srlz_infer_dec_tile(int kind) {
  return kind == SRLZ_INFER_DEC_FIRST || kind == SRLZ_INFER_DEC_MID ? TD : (kind == SRLZ_INFER_DEC_OUT ? TO : 0);
}

extern "C" int srlz_infer_dec_supported(const srlz_infer_dec_desc* d) {
  Dims dm;
  return judge(d, &dm) == nullptr ? 1 : 0;
}

extern "C" int srlz_infer_dec_out_dims(const srlz_infer_dec_desc* d, int* ho, int* wo) {
  Dims dm;
  const char* why = judge(d, &dm);
  SRLZ_REQUIRE(!why, SRLZ_ERR_BAD_DESC, "infer_dec: %s", why);
  if (ho) *ho = dm.ho;
  if (wo) *wo = dm.wo;
  return 0;
}

extern "C" long long srlz_infer_dec_packed_floats(int kind, int c_out) { return packed_floats(kind, c_out); }

extern "C" int srlz_infer_dec_pack_weights(const float* w_ref, float* wpack, int kind, int c_out, srlz_stream_t stream) {
  const long long total = packed_floats(kind, c_out);
  SRLZ_REQUIRE(total > 0, SRLZ_ERR_BAD_DESC, "infer_dec_pack_weights: kind %d with %d output channels", kind, c_out);
  SRLZ_REQUIRE(w_ref && wpack, SRLZ_ERR_NULL, "infer_dec_pack_weights: null pointer");
  SRLZ_LAUNCH(infer_dec_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), w_ref, wpack, kind, c_out,
              (int)total);
  return 0;
}

extern "C" int srlz_infer_dec_block(const float* x, const float* wpack, const float* bias, const float* bnp, float* out,
                                    const srlz_infer_dec_desc* d, srlz_stream_t stream) {
  Dims dm;
  const char* why = judge(d, &dm);
  SRLZ_REQUIRE(!why, SRLZ_ERR_BAD_DESC, "infer_dec_block: %s", why);
  SRLZ_REQUIRE(d->kind != SRLZ_INFER_DEC_OUT, SRLZ_ERR_BAD_DESC, "infer_dec_block: kind out goes through srlz_infer_dec_out");
  SRLZ_REQUIRE(x && wpack && bias && bnp && out, SRLZ_ERR_NULL, "infer_dec_block: null pointer");
  const DecArgs a = make_args(x, wpack, bias, bnp, out, d, dm);
  const int nblocks = dm.tiles_x * dm.tiles_y * d->n;
  if (d->kind == SRLZ_INFER_DEC_FIRST)
    SRLZ_LAUNCH(infer_dec_block_kernel<SRLZ_INFER_DEC_FIRST>, dim3(nblocks), dim3(256), 0, as_stream(stream), a);
  else
    SRLZ_LAUNCH(infer_dec_block_kernel<SRLZ_INFER_DEC_MID>, dim3(nblocks), dim3(256), 0, as_stream(stream), a);
  return 0;
}

extern "C" int srlz_infer_dec_out(const float* x, const float* wpack, const float* bias, void* out, const srlz_infer_dec_desc* d,
                                  srlz_stream_t stream) {
  Dims dm;
  const char* why = judge(d, &dm);
  SRLZ_REQUIRE(!why, SRLZ_ERR_BAD_DESC, "infer_dec_out: %s", why);
  SRLZ_REQUIRE(d->kind == SRLZ_INFER_DEC_OUT, SRLZ_ERR_BAD_DESC, "infer_dec_out: kinds first and mid go through srlz_infer_dec_block");
  SRLZ_REQUIRE(x && wpack && bias && out, SRLZ_ERR_NULL, "infer_dec_out: null pointer");
  const DecArgs a = make_args(x, wpack, bias, nullptr, out, d, dm);
  const int nblocks = dm.tiles_x * dm.tiles_y * d->n;
  if (d->c_out == 3)
    SRLZ_LAUNCH(infer_dec_out_kernel<3>, dim3(nblocks), dim3(256), 0, as_stream(stream), a);
  else
    SRLZ_LAUNCH(infer_dec_out_kernel<6>, dim3(nblocks), dim3(256), 0, as_stream(stream), a);
  return 0;
}
