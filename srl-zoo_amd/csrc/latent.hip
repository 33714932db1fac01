// latent.hip — the image side of evaluation/enjoy_latent.py on gfx950, wave64: a decoded tensor [N,3,W,H] (the reference's tensor
// layout, W-major) becomes pictures [N,H,W,3] (H-major, channels interleaved), either as the float BGR images the reference hands
// to cv2.imshow or as ONE uint8 sheet of tiled pictures that crosses to the host in a single copy.
//
// Both entry points are per-plane transposes with a de-normalisation in between.  A workgroup owns a tile of LT_X columns (w) by
// LT_Y rows (h) of one image, all three channels:
//   read   wave v takes the plane rows x = v, v + 4, ...; its 64 lanes read 64 consecutive h (256 contiguous bytes)
//   LDS    tile[y][x * 3 + oc], rows of 3 * LT_X + 1 floats.  The write has lane = y, a stride of 97 dwords: 97 = 1 (mod 32), the
//          bank modulus of ds_write_b32, so the 32 lanes of a half-wave fall on 32 different banks.  The read has lane = the
//          position in a row: consecutive dwords.
//   write  row y of the tile is 3 * LT_X consecutive floats (bytes) of the output: 384 (96) contiguous bytes per row
// A tile that hangs over the map's edge (w or h no multiple of the tile, w != h) masks the read and the write alike; LDS words that
// were not written are not read.
//
// Rounding.  numpy's deNormalize is two in-place fp32 operations per channel, x *= std then x += mean: the product and the sum are
// rounded separately.  hipcc contracts them into one fma (other bits for a share of the values), and HIP's __fmul_rn / __fadd_rn
// are a plain * and + that it contracts just the same, so this file is built with -ffp-contract=off (csrc/Makefile, as preproc.hip
// is); the two operations are still spelled with the intrinsics to say what is meant.  In the ISA: v_mul_f32 then v_add_f32.
#include <math.h>

#include "common.h"

namespace {

constexpr int LT_X = 32;                // tile columns (w): plane rows a workgroup reads
constexpr int LT_Y = 64;                // tile rows (h): one lane each
constexpr int LT_THREADS = 256;
constexpr int LT_WAVES = LT_THREADS / 64;
constexpr int LT_RUN = 3 * LT_X;        // floats (bytes) of an output row of the tile
constexpr int LT_ROW = LT_RUN + 1;      // LDS row stride in dwords: odd, = 1 (mod 32)
constexpr int LT_FILL_PIXELS = 1024;    // sheet pixels a background workgroup walks

// deNormalize(x, "image_net") of one value of channel c (0 = R): x * std, + mean, clip(0, 1)          preprocessing/utils.py:54-66
// np.clip is min(max(x, 0), 1) with a NaN passed through.
__device__ __forceinline__ float lt_denormalize(float v, int c) {
  const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
  const float mn = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
  float r = __fadd_rn(__fmul_rn(v, sd), mn);
  if (r != r) return r;
  r = r > 0.f ? r : 0.f;
  return r < 1.f ? r : 1.f;
}

// np.rint(v * np.float32(255)).astype(np.uint8) of a value in [0, 1]: round half to even (v_rndne_f32).  A NaN gives 0.
__device__ __forceinline__ unsigned char lt_byte(float v) {
  const float s = rintf(__fmul_rn(v, 255.f));
  return s == s ? (unsigned char)(int)s : (unsigned char)0;
}

struct LtTile { int i, x0, y0; };

// workgroup b of the image part of a grid -> (image, tile origin); tiles of an image are neighbours in b
__device__ __forceinline__ LtTile lt_tile_of(int b, int w, int h) {
  const int tx = (w + LT_X - 1) / LT_X, ty = (h + LT_Y - 1) / LT_Y;
  const int per = tx * ty, i = b / per, t = b - i * per;
  return {i, (t % tx) * LT_X, (t / tx) * LT_Y};
}

// net_out[i] -> .T -> deNormalize -> (channel flip): the tile of image t.i into LDS as tile[y][x * 3 + oc], oc = 2 - c for BGR
// (the [:, :, ::-1] of getImage, evaluation/enjoy_latent.py:36-39) or c for RGB.  Ends with the barrier.
__device__ __forceinline__ void lt_stage(const float* __restrict__ dec, const LtTile t, int w, int h, bool bgr, float* tile) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = t.y0 + lane;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* __restrict__ plane = dec + ((size_t)t.i * 3 + c) * (size_t)w * h;
    const int oc = bgr ? 2 - c : c;
    for (int xr = wave; xr < LT_X; xr += LT_WAVES) {
      const int x = t.x0 + xr;
      if (x < w && y < h) tile[lane * LT_ROW + xr * 3 + oc] = lt_denormalize(plane[(size_t)x * h + y], c);
    }
  }
  __syncthreads();
}

// getImage (evaluation/enjoy_latent.py:21-39) for a batch: img [N,H,W,3] BGR float32
__global__ __launch_bounds__(LT_THREADS) void latent_bgr_kernel(const float* __restrict__ dec, int w, int h, float* __restrict__ img) {
  __shared__ float tile[LT_Y * LT_ROW];
  const LtTile t = lt_tile_of(blockIdx.x, w, h);
  lt_stage(dec, t, w, h, true, tile);
  for (int e = threadIdx.x; e < LT_Y * LT_RUN; e += LT_THREADS) {
    const int yr = e / LT_RUN, j = e - yr * LT_RUN;
    const int y = t.y0 + yr;
    if (y < h && t.x0 + j / 3 < w) img[(((size_t)t.i * h + y) * w + t.x0) * 3 + j] = tile[yr * LT_ROW + j];
  }
}

// The same pictures as bytes, tiled into one sheet (what replaces one cv2.imshow per tick, evaluation/enjoy_latent.py:147, in the
// headless mode).  Workgroups [0, image_blocks) write the pixels of the pictures, the workgroups behind them the background: the
// gaps, the border and the empty tiles of the last grid row.  The two sets of pixels are disjoint and together are the sheet.
__global__ __launch_bounds__(LT_THREADS) void latent_sheet_kernel(const float* __restrict__ dec, int n, int w, int h, int cols, int gap,
                                                                 int fill, int rgb, unsigned char* __restrict__ sheet, int sheet_h,
                                                                 int sheet_w, int image_blocks) {
  __shared__ float tile[LT_Y * LT_ROW];
  const int cell_h = h + gap, cell_w = w + gap;
  if ((int)blockIdx.x >= image_blocks) {
    const long long pixels = (long long)sheet_h * sheet_w;
    const long long p0 = (long long)(blockIdx.x - image_blocks) * LT_FILL_PIXELS;
    const int rows = (n + cols - 1) / cols;
    for (long long p = p0 + threadIdx.x; p < p0 + LT_FILL_PIXELS && p < pixels; p += LT_THREADS) {
      const int y = (int)(p / sheet_w), x = (int)(p - (long long)y * sheet_w);
      const int r = y / cell_h, c = x / cell_w;
      const bool picture = r < rows && c < cols && r * cols + c < n && y - r * cell_h >= gap && x - c * cell_w >= gap;
      if (!picture) {
        sheet[p * 3] = (unsigned char)fill;
        sheet[p * 3 + 1] = (unsigned char)fill;
        sheet[p * 3 + 2] = (unsigned char)fill;
      }
    }
    return;
  }
  const LtTile t = lt_tile_of(blockIdx.x, w, h);
  lt_stage(dec, t, w, h, rgb == 0, tile);
  const int top = gap + (t.i / cols) * cell_h, left = gap + (t.i % cols) * cell_w;
  for (int e = threadIdx.x; e < LT_Y * LT_RUN; e += LT_THREADS) {
    const int yr = e / LT_RUN, j = e - yr * LT_RUN;
    const int y = t.y0 + yr;
    if (y < h && t.x0 + j / 3 < w) sheet[((size_t)(top + y) * sheet_w + left + t.x0) * 3 + j] = lt_byte(tile[yr * LT_ROW + j]);
  }
}

// the checks both entry points share; `who` names the entry point in the error text
int lt_check(const char* who, const void* dec, int n, int w, int h, const void* out) {
  SRLZ_REQUIRE(dec && out, SRLZ_ERR_NULL, "%s: null pointer", who);
  SRLZ_REQUIRE(n >= 1 && w >= 1 && h >= 1, SRLZ_ERR_BAD_DESC, "%s: needs n, w, h >= 1 (n=%d, w=%d, h=%d)", who, n, w, h);
  // (factor by factor: the product of three ints can leave 64 bits)
  const long long lim = 1LL << 31, n3 = (long long)n * 3;
  SRLZ_REQUIRE(n3 < lim && n3 * w < lim && n3 * w * h < lim, SRLZ_ERR_BAD_DESC,
               "%s: n * 3 * w * h must stay below 2^31 (n=%d, w=%d, h=%d)", who, n, w, h);
  return 0;
}

int lt_image_blocks(int n, int w, int h) { return n * ((w + LT_X - 1) / LT_X) * ((h + LT_Y - 1) / LT_Y); }

}  // namespace

extern "C" int srlz_decoded_to_bgr(const float* dec, int n, int w, int h, float* img, srlz_stream_t stream) {
  const int rc = lt_check("decoded_to_bgr", dec, n, w, h, img);
  if (rc) return rc;
  SRLZ_LAUNCH(latent_bgr_kernel, dim3((unsigned)lt_image_blocks(n, w, h)), dim3(LT_THREADS), 0, as_stream(stream), dec, w, h, img);
  return 0;
}

extern "C" int srlz_decoded_to_sheet_u8(const float* dec, int n, int w, int h, int cols, int gap, int fill, int rgb,
                                        unsigned char* sheet, int sheet_h, int sheet_w, srlz_stream_t stream) {
  const int rc = lt_check("decoded_to_sheet_u8", dec, n, w, h, sheet);
  if (rc) return rc;
  SRLZ_REQUIRE(cols >= 1 && gap >= 0, SRLZ_ERR_BAD_DESC, "decoded_to_sheet_u8: needs cols >= 1 and gap >= 0 (cols=%d, gap=%d)", cols,
               gap);
  SRLZ_REQUIRE(fill >= 0 && fill <= 255, SRLZ_ERR_BAD_DESC, "decoded_to_sheet_u8: fill must lie in [0, 255] (fill=%d)", fill);
  const long long rows = ((long long)n + cols - 1) / cols;
  const long long want_h = rows * h + (rows + 1) * gap, want_w = (long long)cols * w + ((long long)cols + 1) * gap;
  SRLZ_REQUIRE(want_h < (1LL << 31) && want_w < (1LL << 31) && want_h * want_w * 3 < (1LL << 31), SRLZ_ERR_BAD_DESC,
               "decoded_to_sheet_u8: the sheet of %lld x %lld pixels must stay below 2^31 bytes", want_h, want_w);
  SRLZ_REQUIRE(sheet_h == want_h && sheet_w == want_w, SRLZ_ERR_BAD_DESC,
               "decoded_to_sheet_u8: inconsistent sheet size %d x %d, the grid of %lld x %d tiles of %d x %d with gap %d is %lld x %lld",
               sheet_h, sheet_w, rows, cols, h, w, gap, want_h, want_w);
  const int image_blocks = lt_image_blocks(n, w, h);
  const int fill_blocks = (int)((want_h * want_w + LT_FILL_PIXELS - 1) / LT_FILL_PIXELS);
  SRLZ_LAUNCH(latent_sheet_kernel, dim3((unsigned)(image_blocks + fill_blocks)), dim3(LT_THREADS), 0, as_stream(stream), dec, n, w, h,
              cols, gap, fill, rgb, sheet, sheet_h, sheet_w, image_blocks);
  return 0;
}
