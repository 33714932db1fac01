// convn.hip — the trunk convolutions with 64 to 512 channels (formulation: conv64.hip).
//
// ---------------------------------------------------------------------------------------------------------------
// convN: the same virtual-grid implicit GEMM for Cin, Cout in {64, 128, 256, 512} — FORWARD ONLY.  It exists for the frozen
// ResNet-18 trunk of EmbeddingNet (/root/reference/models/triplet.py:6-39 -> torchvision resnet18: 3x3 convolutions of
// stride 1 / 2 and 1x1 stride-2 downsample convolutions, all without bias); nothing is ever back-propagated through it.
// blockIdx.y = block of 64 output channels; the input channels are walked in blocks of 64 around the nine taps with the
// accumulators kept; weights are packed [cout block][cin block][tap][64][64].  A 1x1 stride-2 convolution runs as the 3x3
// stride-2 pad-1 program with only the centre tap non-zero (same output size, same sampled pixels; its 8 zero taps cost
// ~4 % of the trunk's FLOP).  x_bnp: one 256-float BatchNorm record per block of 64 input channels.
// ---------------------------------------------------------------------------------------------------------------
#include "conv64_tile.h"

namespace {

__global__ __launch_bounds__(256, 2) void convN_fwd_kernel(const float* __restrict__ src, const float* __restrict__ wpack,
                                                          float* __restrict__ dst, float* __restrict__ stats_partial,
                                                          const ConvProg P, int ntiles, int nci, int nco,
                                                          const float* __restrict__ src_bnp, int only_tap, int cshift) {
  // Round 5: rebuilt on the 64-channel family's machinery (conv64_fwd_body) — the tile's row table in LDS (one decomposition per row
  // and tile instead of one per row, thread, class AND input-channel block), the BatchNorm coefficients of every input-channel block
  // in LDS once per workgroup, operand fragments double-buffered in registers, the epilogue through a wave-private LDS transpose with
  // 16-byte stores.  Same tiles and the same accumulation order as the round-2 kernel: outputs bit-identical to it.
  // only_tap >= 0: the program's tap index of the ONE tap whose weights are not zero — a 1x1 stride-2 convolution (ResNet's downsample
  // branch) is the 3x3 stride-2 pad-1 program's centre tap; the other eight used to be multiplied through as zeros (4 % of the trunk).
  // cshift = log2(input channels).
  constexpr int NT = 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* As = (float*)smem;
  float* Bs = As + (TM + P.span) * 64;
  const int tpa = rowtab_passes(TM + P.span);
  unsigned* rowtab = (unsigned*)(Bs + 4096);
  int* rowinfo = (int*)(rowtab + 16 * tpa);      // [TM]: output pixel index, or -1
  float* frec = (float*)(rowinfo + TM);          // [nci][128]: scale, shift of every input-channel block (fused relu(bn(.)) operand)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int tile = xcd_remap(blockIdx.x, ntiles);
  const int co = blockIdx.y;
  const int cout = nco * 64;
  // BatchNorm groups (round 6: the six views of a time-contrastive step batched along n — models/learner.py:383-391 calls the trunk
  // once per view): tiles [g * tpg, (g + 1) * tpg) cover group g's own virtual grid, exactly as in conv64_fwd_body — a tile's
  // statistics partial belongs to one group, its fused operand uses that group's records ([group][input-channel block][256])
  const int grp = (P.G > 1) ? tile / P.tpg : 0;
  const int q0 = (tile - grp * P.tpg) * TM;
  src += (size_t)grp * P.src_gstride * nci;
  dst += (size_t)grp * P.dst_gstride * nco;
  if (src_bnp) src_bnp += (size_t)grp * nci * 256;

  if (tid < TM) {
    const int q = q0 + tid;
    int ri = -1;
    if (q < P.total_q) {
      const GridPix g = grid_pix<false>(P, q, P.ds);
      if (g.y < P.Hd && g.x < P.Wd) ri = (g.n * P.Hd + g.y) * P.Wd + g.x;
    }
    rowinfo[tid] = ri;
  }
  rowtab_build(rowtab, tpa, P, q0 + P.min_off, TM + P.span);
  if (src_bnp)
    for (int i = tid; i < nci * 128; i += NT) frec[i] = src_bnp[(i >> 7) * 256 + 128 + (i & 127)];

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  constexpr int BV = 1024 / NT;
  const int bslot = wave * (BV * 64) + lane;  // wave w moves (and may later scribble on) its own 4 KB of the slab
  f32x4 breg[BV];
  const float* wbase = wpack + (size_t)co * nci * NTAPS * 4096;
  const int t_first = only_tap >= 0 ? only_tap : 0, t_count = only_tap >= 0 ? 1 : NTAPS;
  {
    const f32x4* wsrc = (const f32x4*)(wbase + (size_t)P.tw[t_first] * 4096);
#pragma unroll
    for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot + i * 64];
  }
  const int nsteps = nci * t_count;
  int ci = 0, tk = 0;       // the step's input-channel block and its tap (tk-th of the block's t_count)
  int cur_src = -1;
  for (int step = 0; step < nsteps; ++step) {
    const int ti = t_first + tk;
    const int tsrc = P.tsrc[ti], toff = P.toff[ti];
    // the next step's (block, tap): its weight slab is requested behind this step's second barrier
    int tk2 = tk + 1, ci2 = ci;
    if (tk2 == t_count) { tk2 = 0; ci2 = ci + 1; }
    __syncthreads();  // all waves are done with the previous step's Bs (and with As if it is about to be replaced)
    if (tk == 0 || tsrc != cur_src) {
      stage_rows_tab<BATCH_FWD>(As, src, rowtab, tpa, tsrc, P.Ws, TM + P.span, src_bnp ? frec + ci * 128 : nullptr, cshift, ci * 64);
      cur_src = tsrc;
    }
    {
      f32x4* wdst = (f32x4*)Bs;
#pragma unroll
      for (int i = 0; i < BV; ++i) wdst[bslot + i * 64] = breg[i];
    }
    __syncthreads();
    {  // (past the last step: block 0, first tap again — never a run-time condition around loads, see conv64_fwd_body)
      const int cn = ci2 < nci ? ci2 : 0;
      const f32x4* wsrc = (const f32x4*)(wbase + ((size_t)cn * NTAPS + P.tw[t_first + tk2]) * 4096);
#pragma unroll
      for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot + i * 64];
    }
    __builtin_amdgcn_sched_barrier(0);  // the slab requests go out HERE, ahead of the step's MFMAs
    const int R = wave * 32 + l31 + toff - P.min_off;
    int abase = (R * 64 + ((h ^ (R & 15)) << 2)) * 4;  // bytes; slot (2kc + h) ^ (R & 15) is this XOR (kc << 5)
    asm volatile("" : "+v"(abase));
    const float* brow = Bs + l31 * 64;
    const int bkey = lane & 15;
    f32x4 a = *(const f32x4*)((const char*)As + abase);
    f32x4 b[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j] = *(const f32x4*)(brow + j * 2048 + ((h ^ bkey) << 2));
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) {
      f32x4 an = a, bn[2] = {b[0], b[1]};
      if (kc < 7) {
        const int slot = (kc + 1) * 2 + h;
        an = *(const f32x4*)((const char*)As + (abase ^ ((kc + 1) << 5)));
#pragma unroll
        for (int j = 0; j < 2; ++j) bn[j] = *(const f32x4*)(brow + j * 2048 + ((slot ^ bkey) << 2));
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ahead of this chunk's MFMAs
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[j][r], acc[j], 0, 0, 0);
      a = an; b[0] = bn[0]; b[1] = bn[1];
    }
    tk = tk2; ci = ci2;
  }
  __syncthreads();  // every wave is done with the last slab: Bs becomes scratch
  // epilogue: 16 tile rows at a time through this wave's 4 KB of the idle slab, so that every global store is 16 bytes per lane
  // (lane = (row group eg = lane >> 4, channels 4 eslot ..)); the BatchNorm partials in the same layout (see conv64_fwd_body::flush16)
  f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
  {
    float* S = Bs + wave * 1024;
    const int eg = lane >> 4, eslot = lane & 15;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int rowl = (rr & 3) + 8 * (rr >> 2) + 4 * h;
        const int swz = (rowl & 4) << 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) S[rowl * 64 + ((32 * j + l31) ^ swz)] = acc[j][8 * half + rr];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rowl = eg + 4 * k;
        const int row = wave * 32 + 16 * half + rowl;
        const f32x4 v = *(const f32x4*)(S + rowl * 64 + ((eslot ^ ((rowl & 4) << 1)) << 2));
        const int ri = rowinfo[row];
        if (ri >= 0) {
          *(f32x4*)(dst + (size_t)ri * cout + co * 64 + eslot * 4) = v;
#pragma unroll
          for (int e = 0; e < 4; ++e) { s4[e] += v[e]; q4[e] += v[e] * v[e]; }
        }
      }
    }
  }
  if (stats_partial) {
    __syncthreads();
    float* red = Bs;  // [4 waves][128]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s4[e] += __shfl_xor(s4[e], 16, 64); s4[e] += __shfl_xor(s4[e], 32, 64);
      q4[e] += __shfl_xor(q4[e], 16, 64); q4[e] += __shfl_xor(q4[e], 32, 64);
    }
    if (lane < 16) {
      *(f32x4*)(red + wave * 128 + lane * 4) = s4;
      *(f32x4*)(red + wave * 128 + 64 + lane * 4) = q4;
    }
    __syncthreads();
    // chunk-major: the partial records of one 64-channel block are contiguous (what srlz_bn_finalize_chunks reduces)
    if (tid < 128) stats_partial[((size_t)co * ntiles + tile) * 128 + tid] = red[tid] + red[128 + tid] + red[256 + tid] + red[384 + tid];
  }
}

// w_ref [Cout][Cin][k][k] (k = 3 or 1) -> packed [cout block][cin block][tap][n][swizzled k]; a 1x1 kernel becomes the centre tap
__global__ void convN_pack_kernel(const float* __restrict__ w_ref, float* __restrict__ pf, int nci, int nco, int ksize) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)nco * nci * NTAPS * 4096;
  if (id >= total) return;
  const int k = (int)(id & 63), n = (int)((id >> 6) & 63);
  const long long blk = id >> 12;
  const int tap = (int)(blk % NTAPS);
  const int ci = (int)((blk / NTAPS) % nci), co = (int)(blk / NTAPS / nci);
  const int cin = nci * 64;
  float v;
  if (ksize == 3) v = w_ref[((size_t)(co * 64 + n) * cin + ci * 64 + k) * 9 + tap];
  else v = (tap == 4) ? w_ref[(size_t)(co * 64 + n) * cin + ci * 64 + k] : 0.f;
  pf[blk * 4096 + n * 64 + ((((k >> 2) ^ (n & 15)) << 2) | (k & 3))] = v;
}

// source rows, slab, row table, rowinfo, (scale, shift) of up to 8 input-channel blocks
static size_t convn_lds_bytes(const ConvProg& P) {
  return (size_t)(TM + P.span) * 256 + 16384 + (size_t)64 * rowtab_passes(TM + P.span) + TM * 4 + 8 * 128 * 4;
}

static int check_convn(const srlz_convn_desc* d) {
  SRLZ_REQUIRE(d != nullptr, SRLZ_ERR_NULL, "convn: null descriptor");
  SRLZ_REQUIRE(d->n > 0 && d->cin > 0 && d->cout > 0 && d->cin % 64 == 0 && d->cout % 64 == 0, SRLZ_ERR_BAD_DESC,
               "convn: channels must be multiples of 64 (cin=%d cout=%d)", d->cin, d->cout);
  // (the staging addresses a pixel's channels by a shift, the fused operand's coefficients of all input-channel blocks sit in 4 KB of LDS)
  SRLZ_REQUIRE((d->cin & (d->cin - 1)) == 0 && d->cin <= 512, SRLZ_ERR_BAD_DESC,
               "convn: %d input channels (a power of two from 64 to 512)", d->cin);
  SRLZ_REQUIRE(d->groups >= 0 && (d->groups <= 1 || d->n % d->groups == 0), SRLZ_ERR_BAD_DESC,
               "convn: n = %d is not a multiple of groups = %d", d->n, d->groups);
  const bool k3 = d->ksize == 3 && d->pad == 1 && (d->stride == 1 || d->stride == 2);
  const bool k1 = d->ksize == 1 && d->pad == 0 && d->stride == 2;
  SRLZ_REQUIRE(k3 || k1, SRLZ_ERR_BAD_DESC, "convn: 3x3 pad 1 stride 1/2 or 1x1 stride 2 only (k=%d s=%d p=%d)", d->ksize, d->stride,
               d->pad);
  const int eho = (d->hi + 2 * d->pad - d->ksize) / d->stride + 1, ewo = (d->wi + 2 * d->pad - d->ksize) / d->stride + 1;
  SRLZ_REQUIRE(eho == d->ho && ewo == d->wo, SRLZ_ERR_BAD_DESC, "convn: output size %dx%d inconsistent (expected %dx%d)", d->ho,
               d->wo, eho, ewo);
  return 0;
}

static int convn_program(ConvProg* P, const srlz_convn_desc* d) {
  // (a 1x1 stride-2 pad-0 convolution samples exactly the centre-tap pixels of the 3x3 stride-2 pad-1 program)
  const int rc = conv64::build_program(P, 1, d->stride, 1, d->n, d->hi, d->wi, d->ho, d->wo, d->groups > 1 ? d->groups : 1);
  SRLZ_REQUIRE(rc == 0, SRLZ_ERR_BAD_DESC, "convn: cannot build a grid program for this descriptor");
  return 0;
}

}  // namespace

extern "C" size_t srlz_convn_packed_floats(const srlz_convn_desc* d) {
  if (check_convn(d)) return 0;
  return (size_t)(d->cin / 64) * (d->cout / 64) * NTAPS * 4096;
}

extern "C" int srlz_convn_pack_weights(const float* w_ref, float* wpack, const srlz_convn_desc* d, srlz_stream_t stream) {
  if (int rc = check_convn(d)) return rc;
  SRLZ_REQUIRE(w_ref && wpack, SRLZ_ERR_NULL, "convn_pack: null pointer");
  const long long total = (long long)(d->cin / 64) * (d->cout / 64) * NTAPS * 4096;
  SRLZ_LAUNCH(convN_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), w_ref, wpack, d->cin / 64,
              d->cout / 64, d->ksize);
  return 0;
}

extern "C" int srlz_convn_fwd_tiles(const srlz_convn_desc* d) {
  if (check_convn(d)) return -1;
  ConvProg P;
  if (convn_program(&P, d)) return -1;
  return P.G * P.tpg;
}

extern "C" int srlz_convn_fwd(const float* x, const float* wpack, float* y, float* stats_partial, const float* x_bnp,
                              const srlz_convn_desc* d, srlz_stream_t stream) {
  if (int rc = check_convn(d)) return rc;
  SRLZ_REQUIRE(x && wpack && y, SRLZ_ERR_NULL, "convn_fwd: null pointer");
  ConvProg P;
  if (int rc = convn_program(&P, d)) return rc;
  const int ntiles = P.G * P.tpg;
  const size_t lds = convn_lds_bytes(P);
  SRLZ_REQUIRE(lds <= 160 * 1024, SRLZ_ERR_BAD_DESC, "convn: tile needs %zu bytes of LDS", lds);
  SRLZ_MAX_LDS(convN_fwd_kernel, lds);
  int cshift = 6;
  while ((1 << cshift) < d->cin) ++cshift;
  // (the row table keeps pixel indices in 28 bits, the staging 32-bit float offsets)
  // (per BatchNorm group: P.N images)
  SRLZ_REQUIRE((long long)P.N * d->hi * d->wi * d->cin < (1LL << 32) && (long long)P.N * d->hi * d->wi < (1LL << 28), SRLZ_ERR_BAD_DESC,
               "convn: a group of %d images of %d x %d x %d is beyond the tile tables' 32-bit offsets", P.N, d->hi, d->wi, d->cin);
  int only_tap = -1;
  if (d->ksize == 1) {  // the tap of the 3x3 program that carries the 1x1 kernel: weight slab 4 = (ky, kx) = (1, 1)
    for (int t = 0; t < NTAPS; ++t)
      if (P.tw[t] == 4) only_tap = t;
    SRLZ_REQUIRE(only_tap >= 0, SRLZ_ERR_BAD_DESC, "convn: no centre tap in the program of a 1x1 convolution");
  }
  SRLZ_LAUNCH(convN_fwd_kernel, dim3(ntiles, d->cout / 64), dim3(256), lds, as_stream(stream), x, wpack, y, stats_partial, P, ntiles,
              d->cin / 64, d->cout / 64, x_bnp, only_tap, cshift);
  return 0;
}
