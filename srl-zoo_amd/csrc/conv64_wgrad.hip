// conv64_wgrad.hip — the weight gradients of the 3x3, 64 -> 64 convolutions and transposed convolutions (formulation: conv64.hip).
//
// ---------------------------------------------------------------------------------------------------------------
// Weight-gradient kernel: dW[w][ci][co] = sum_q S_c(q+off)[ci] * G_d(q)[co]   (G = dy at dest class d).
// GEMM view: M = ci (64), N = co (64), K = grid positions.  4 waves = 4 quadrants of 32x32, each holding all 9 taps
// (144 accumulator registers); persistent over K-chunks of 64 positions; per-workgroup partials are reduced by
// conv64_wgrad_reduce in a fixed order (deterministic).
// ---------------------------------------------------------------------------------------------------------------
#include "conv64_tile.h"

namespace {

template <bool S2, int TK>
__global__ __launch_bounds__(256, 2) void conv64_wgrad_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ g,
                                                             float* __restrict__ partial, const ConvProg P,
                                                             int nchunks, const OpFuse x_fuse, const OpFuse g_fuse) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ss = (float*)smem;              // (TK + span) x 64
  float* Gs = Ss + (TK + P.span) * 64;   // TK x 64

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int mi = wave & 1, nj = wave >> 1;

  f32x16 acc[NTAPS];
#pragma unroll
  for (int t = 0; t < NTAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;  // column sum of dy (bias gradient): thread (col = tid&63, part = tid>>6)

  constexpr int NG = S2 ? 4 : 1;
  constexpr int GSTART[5] = {0, S2 ? 4 : 9, 6, 8, 9};

  // nchunks = P.G * cpg: chunk -> (BatchNorm group, chunk of that group's grid); a chunk never straddles two groups
  const int cpg = nchunks / P.G;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int grp = (P.G > 1) ? chunk / cpg : 0;
    const int q0 = (chunk - grp * cpg) * TK;
    const float* __restrict__ xg = x + grp * P.src_gstride;
    const float* __restrict__ gg = g + grp * P.dst_gstride;
    const OpFuse xf = fuse_for_group(x_fuse, grp, grp * P.src_gstride);
    const OpFuse gf = fuse_for_group(g_fuse, grp, grp * P.dst_gstride);
    int cur_s = -1, cur_g = -1;
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      const int t0 = GSTART[gi], t1 = GSTART[gi + 1];
      const int cs = P.tsrc[t0], cd = P.tdst[t0];
      __syncthreads();
      if (cs != cur_s) {
        stage_rows<false, 4>(Ss, xg, P.Hs, P.Ws, P.ss, cs, P.PW, P.PH, P.total_q, q0 + P.min_off, TK + P.span, xf);
        cur_s = cs;
      }
      const bool newg = (cd != cur_g);
      if (newg) {
        if (g_fuse.y) stage_rows<false, 2, 256, true>(Gs, gg, P.Hd, P.Wd, P.ds, cd, P.PW, P.PH, P.total_q, q0, TK, gf);
        else stage_rows<false, 4>(Gs, gg, P.Hd, P.Wd, P.ds, cd, P.PW, P.PH, P.total_q, q0, TK);
        cur_g = cd;
      }
      __syncthreads();
      if (newg) {
        const int col = tid & 63, part = tid >> 6;
#pragma unroll
        for (int r = 0; r < TK / 4; ++r) bsum += Gs[(part * (TK / 4) + r) * 64 + col];
      }
      // blocks of 4 k-steps (rows 8b + 2i + h): one address per operand column and block, the 4 rows as immediate offsets
      const float* gcol = Gs + h * 64 + nj * 32 + l31;
      const float* scol = Ss + h * 64 + mi * 32 + l31;
#pragma unroll 2
      for (int b = 0; b < TK / 8; ++b) {
        float bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = gcol[(8 * b + 2 * i) * 64];
#pragma unroll
        for (int t = t0; t < t1; ++t) {
          const float* ap = scol + (8 * b + P.toff[t] - P.min_off) * 64;
          float af[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = ap[2 * i * 64];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[i], acc[t], 0, 0, 0);
        }
      }
    }
  }
  // partial[wg][9 (reference tap index)][64 ci][64 co] + [wg][64] bias sums after all workgroups' tap blocks
  float* out = partial + (size_t)blockIdx.x * (NTAPS * 4096);
#pragma unroll
  for (int t = 0; t < NTAPS; ++t) {
    float* o = out + (size_t)P.tw[t] * 4096;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      o[row * 64 + nj * 32 + l31] = acc[t][r];
    }
  }
  __syncthreads();
  float* red = Ss;
  red[tid] = bsum;
  __syncthreads();
  if (tid < 64) {
    float* bout = partial + (size_t)gridDim.x * (NTAPS * 4096) + (size_t)blockIdx.x * 64;
    bout[tid] = red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight-gradient kernel of the stride-2 GATHER programs (conv3: four source classes in tap groups {4, 2, 2, 1}, one destination
// class), software-pipelined.  conv64_wgrad_kernel<true> stages each class synchronously between two barriers — four HBM round
// trips per 64-position chunk in front of 128 / 64 / 64 / 32 MFMAs per wave — and walks (image, row, column) for every staged row
// (~30 vector-ALU instructions per row, 24 rows per thread and chunk against 288 MFMAs).  Here
//  * the rows of the NEXT group's class (the next chunk's class 0 and gradient rows behind the last group) are requested into
//    registers right after the barrier that opens a group's MFMA loop and land in LDS behind the barrier that closes it;
//  * a chunk's rows are decomposed once, into two small tables (source side: rowtab_build; gradient side below), rebuilt for the next
//    chunk in the inter-barrier section of the last group, when nobody reads them.
// Same chunks per workgroup, same MFMA order, same partial layout as conv64_wgrad_kernel<true, 64>: results are bit-identical.
// ---------------------------------------------------------------------------------------------------------------
constexpr int WG_TK = 64;           // positions per chunk (128 was tried: the extra staging registers spill)
constexpr int WG_SROWS = 8;         // source rows per thread: WG_TK + span <= 128
constexpr int WG_SWORDS = 16 * WG_SROWS, WG_GWORDS = 16 * 4;

// gradient side: entry of row R of the chunk at (R & 15) * 4 + (R >> 4) = pixel index << 1 | 1 (0: outside the tensor)
__device__ __forceinline__ void wg_gtab_build(unsigned* __restrict__ tab, const ConvProg& P, int q0) {
  int R = (int)threadIdx.x - 128;  // (threads 128 .. 191; the source table is built by threads 0 .. 127)
  asm volatile("" : "+v"(R));
  if ((unsigned)R < (unsigned)WG_GWORDS) {
    const int q = q0 + R;
    unsigned e = 0;
    if (q < P.total_q) {
      const GridPix g = grid_pix<false>(P, q, P.ds);
      if (g.y < P.Hd && g.x < P.Wd) e = pix_entry(g.n, g.y, g.x, P.Hd, P.Wd);
    }
    tab[(R & 15) * 4 + (R >> 4)] = e;
  }
}

__global__ __launch_bounds__(256, 2) void conv64_wgrad_gather_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                    float* __restrict__ partial, const ConvProg P, int nchunks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int srows = WG_TK + P.span;
  float* Ss = (float*)smem;                    // (WG_TK + span) x 64: the rows of the current source class
  float* Gs = Ss + srows * 64;                 // WG_TK x 64: the chunk's gradient rows
  unsigned* stab = (unsigned*)(Gs + WG_TK * 64);  // [16][WG_SROWS]
  unsigned* gtab = stab + WG_SWORDS;              // [16][4]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int mi = wave & 1, nj = wave >> 1;

  f32x16 acc[NTAPS];
#pragma unroll
  for (int t = 0; t < NTAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  constexpr int GSTART[5] = {0, 4, 6, 8, 9};
  const int cpg = nchunks / P.G;
  f32x4 sv[WG_SROWS], gv[4];
  unsigned sok = 0, gok = 0;

  // rows of source class `cls` of the chunk whose table is in stab -> registers (branch-free; masks applied at the landing)
  auto s_request = [&](const float* __restrict__ xg, int cls) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int slot = t & 15;
    const unsigned delta = (unsigned)((cls >> 1) * P.Ws + (cls & 1));
    const unsigned* __restrict__ tp = stab + (t >> 4) * WG_SROWS;
    const uint4 e0 = *(const uint4*)tp, e1 = *(const uint4*)(tp + 4);
    const unsigned e[WG_SROWS] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
    sok = 0;
#pragma unroll
    for (int j = 0; j < WG_SROWS; ++j) {
      const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)e[j], (unsigned)cls, 1u);
      sv[j] = *(const f32x4*)(xg + (((((e[j] >> 4) + delta) << 6) & m) + slot * 4));
      sok |= m & (1u << j);
    }
  };
  auto g_request = [&](const float* __restrict__ gg, bool live) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int slot = t & 15;
    const uint4 q = *(const uint4*)(gtab + (t >> 4) * 4);
    const unsigned e[4] = {q.x, q.y, q.z, q.w};
    gok = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gv[j] = *(const f32x4*)(gg + (((e[j] >> 1) << 6) + slot * 4));
      gok |= (live ? (e[j] & 1u) : 0u) << j;
    }
  };
  auto s_land = [&]() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int slot = t & 15, r = t >> 4;
#pragma unroll
    for (int j = 0; j < WG_SROWS; ++j) {
      const int R = r + 16 * j;
      const f32x4 v = ((sok >> j) & 1u) ? sv[j] : f32x4{0.f, 0.f, 0.f, 0.f};
      if (R < srows) *(f32x4*)(Ss + R * 64 + slot * 4) = v;  // (an LDS write only: no vector-memory operation in a branch)
    }
  };
  auto g_land = [&]() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int slot = t & 15, r = t >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) *(f32x4*)(Gs + (r + 16 * j) * 64 + slot * 4) = ((gok >> j) & 1u) ? gv[j] : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto tables = [&](int q0, bool live) {
    // (no rows for a chunk past the end: every entry 0 -> every row reads pixel 0 and lands as zeros)
    if (tid < 128) rowtab_build(stab, WG_SROWS, P, q0 + P.min_off, live ? srows : 0);
    wg_gtab_build(gtab, P, live ? q0 : P.total_q);
  };

  int chunk = blockIdx.x;
  if (chunk < nchunks) {  // the first chunk's class 0 and gradient rows are staged the plain way
    const int grp = (P.G > 1) ? chunk / cpg : 0;
    tables((chunk - grp * cpg) * WG_TK, true);
    __syncthreads();
    s_request(x + grp * P.src_gstride, P.tsrc[0]);
    g_request(g + grp * P.dst_gstride, true);
  }
  for (; chunk < nchunks; chunk += gridDim.x) {
    const int grp = (P.G > 1) ? chunk / cpg : 0;
    const float* __restrict__ xg = x + grp * P.src_gstride;
    const int chunk2 = chunk + (int)gridDim.x;
    const bool more = chunk2 < nchunks;
    const int grp2 = (P.G > 1 && more) ? chunk2 / cpg : grp;
    const int q02 = ((more ? chunk2 : chunk) - grp2 * cpg) * WG_TK;
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const int t0 = GSTART[gi], t1 = GSTART[gi + 1];
      __syncthreads();  // every wave is done with the previous group's Ss (and, at gi == 0, with the previous chunk's Gs)
      s_land();
      if (gi == 0) g_land();
      if (gi == 3) tables(q02, more);  // (the last request through this chunk's tables went out behind the previous barrier)
      __syncthreads();
      if (gi < 3) s_request(xg, P.tsrc[GSTART[gi + 1]]);
      else {
        s_request(x + grp2 * P.src_gstride, P.tsrc[0]);
        g_request(g + grp2 * P.dst_gstride, more);
      }
      __builtin_amdgcn_sched_barrier(0);  // the requests go out HERE, ahead of the group's MFMAs
      if (gi == 0) {
        const int col = tid & 63, part = tid >> 6;
#pragma unroll
        for (int r = 0; r < WG_TK / 4; ++r) bsum += Gs[(part * (WG_TK / 4) + r) * 64 + col];
      }
      const float* gcol = Gs + h * 64 + nj * 32 + l31;
      const float* scol = Ss + h * 64 + mi * 32 + l31;
#pragma unroll 2
      for (int b = 0; b < WG_TK / 8; ++b) {
        float bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = gcol[(8 * b + 2 * i) * 64];
#pragma unroll
        for (int t = t0; t < t1; ++t) {
          const float* ap = scol + (8 * b + P.toff[t] - P.min_off) * 64;
          float af[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = ap[2 * i * 64];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[i], acc[t], 0, 0, 0);
        }
      }
    }
  }
  float* out = partial + (size_t)blockIdx.x * (NTAPS * 4096);
#pragma unroll
  for (int t = 0; t < NTAPS; ++t) {
    float* o = out + (size_t)P.tw[t] * 4096;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      o[row * 64 + nj * 32 + l31] = acc[t][r];
    }
  }
  __syncthreads();
  float* red = Ss;
  red[tid] = bsum;
  __syncthreads();
  if (tid < 64) {
    float* bout = partial + (size_t)gridDim.x * (NTAPS * 4096) + (size_t)blockIdx.x * 64;
    bout[tid] = red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight-gradient kernel, ring version (programs with ONE source class: stride-1 conv, transposed conv).
// Same GEMM as above, but
//  * a workgroup walks a CONTIGUOUS range of chunks and keeps the source rows in a 256-row LDS ring: consecutive
//    chunks share TK+span-64 of their TK+span rows (span = 116 for conv2), so each chunk only fetches 64 new source rows
//    instead of 180 (121 -> 64 for the transposed convolutions);
//  * the new source rows and the next gradient rows are requested into registers BEFORE the chunk's MFMA loop and
//    written to LDS after it: their latency sits behind the matrix work (two barriers per group remain).
// ---------------------------------------------------------------------------------------------------------------
// The source ring of conv64_wgrad_ring_kernel: row q of the virtual grid lives at slot q mod RING_ROWS; the first RING_MIRROR
// slots are kept a second time behind the ring (slots RING_ROWS .. RING_ROWS + RING_MIRROR), so that a reader that starts at
// any slot can go on for RING_MIRROR rows without wrapping — the MFMA loop wraps ONE wave-uniform (scalar) row index per tap
// and 4 k-steps and reaches its 4 rows through the immediate offsets of two ds_read2st64_b32.  (The previous layout — 256
// slots, "& 255" on every address — cost three VALU instructions and one ds_read_b32 per MFMA, and that instruction stream,
// not the matrix pipe, bounded the loop: 113 TF with every load and barrier removed.)
// RING_ROWS >= TK + span + TK (the prefetched TK rows are written only after the readers' barrier).
constexpr int RING_ROWS = 246, RING_MIRROR = 8, RING = RING_ROWS + RING_MIRROR;  // (246 + 8 + 64 rows + 2 rows of tables = 80 KB)
// the stride-2 (ConvTranspose) kernel walks 32-position chunks: RING_ROWS_S2 >= 32 + span + 32, and 4 x 32 gradient rows next to it
constexpr int RING_ROWS_S2 = 184, RING_S2 = RING_ROWS_S2 + RING_MIRROR;
template <int ROWS = RING_ROWS>
__device__ __forceinline__ int ring_slot(int q) { return (q + 4 * ROWS) % ROWS; }  // q >= -4 * ROWS

// rows [qstart, qstart+64) of class `cls`: 4 rows per thread (16 apart) into registers; okmask bit j = row j in bounds.
// <J0, NJ>: only this thread's rows J0 .. J0+NJ-1 (v[j - J0]); the other bits of okmask are left alone.
template <int J0 = 0, int NJ = 4>
__device__ __forceinline__ void rows64_load(f32x4 (&v)[NJ], unsigned& okmask, const float* __restrict__ src, int H, int W,
                                            int stride, int cls, int PW, int PH, int total_q, int qstart, const GridDiv gd) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));  // opaque: nothing derived from the thread index here is worth a register across the caller's loops
  const int slot = t & 15;
  const int cy = cls >> 1, cx = cls & 1;
  const int PHW = PH * PW;
  // (fastdiv: three true divisions here were ~120 VALU instructions per call — per 64-position chunk and thread)
  // (16 positions = sn images + sa rows + sb columns, as in stage_rows: one carry per digit on any grid)
  const int sn = fastdiv(16, gd.mPHW, gd.sPHW), srem = 16 - sn * PHW;
  const int sa = fastdiv(srem, gd.mPW, gd.sPW), sb = srem - sa * PW;
  const int qq = qstart + (t >> 4) + PHW;  // shifted by one image: non-negative for the first rows of the first chunk
  int n1 = fastdiv(qq, gd.mPHW, gd.sPHW);
  int rem = qq - n1 * PHW;
  int a = fastdiv(rem, gd.mPW, gd.sPW);
  int b = rem - a * PW;
  const int N1max = total_q / PHW;
  if (J0 == 0) okmask = 0;
#pragma unroll
  for (int j = 0; j < J0 + NJ; ++j) {
    if (j >= J0) {
      v[j - J0] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int y = (a << (stride - 1)) + cy, x = (b << (stride - 1)) + cx;  // (stride is 1 or 2: a shift-add, not a quarter-rate multiply)
      const bool ok = (unsigned)(n1 - 1) < (unsigned)N1max && y < H && x < W;
      okmask |= (ok ? 1u : 0u) << j;
      if (ok) v[j - J0] = *(const f32x4*)(src + (mad_u24(mad_u24((unsigned)(n1 - 1), H, (unsigned)y), W, (unsigned)x) * 64u + (unsigned)(slot * 4)));
    }
    b += sb; a += sa; n1 += sn;
    if (b >= PW) { b -= PW; ++a; }
    if (a >= PH) { a -= PH; ++n1; }
  }
}

// registers -> LDS rows (row index of this thread's j-th row = rbase + 16*j; RINGED: its ring slot, plus the mirror copy);
// bnp != NULL: relu(batchnorm(.)) applied to in-bounds rows on the way (OpFuse forward fusion)
// The scale / shift of a fused operand for this thread's four channels (identity when bnp == NULL): loaded ONCE by the caller — at
// every landing they would be an L2 round trip in front of the LDS writes, once per 32- or 64-position chunk.
struct BnQuad { f32x4 sc, sh; bool on; };
__device__ __forceinline__ BnQuad bn_quad(const float* __restrict__ bnp) {
  BnQuad q = {f32x4{1.f, 1.f, 1.f, 1.f}, f32x4{0.f, 0.f, 0.f, 0.f}, bnp != nullptr};
  const int slot = threadIdx.x & 15;
  if (bnp) { q.sc = *(const f32x4*)(bnp + 128 + slot * 4); q.sh = *(const f32x4*)(bnp + 192 + slot * 4); }
  return q;
}

template <bool RINGED, int J0 = 0, int NJ = 4, int ROWS = RING_ROWS>
__device__ __forceinline__ void rows64_store(float* __restrict__ lds, int rbase, f32x4 (&v)[NJ], unsigned okmask,
                                             const BnQuad& bq) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));  // (see rows64_load)
  const int slot = t & 15;
  const f32x4 sc4 = bq.sc, sh4 = bq.sh;
  const bool bnp = bq.on;
#pragma unroll
  for (int j = J0; j < J0 + NJ; ++j) {
    if (bnp && ((okmask >> j) & 1u)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float z = v[j - J0][e] * sc4[e] + sh4[e]; v[j - J0][e] = z > 0.f ? z : 0.f; }
    }
    int R = rbase + (t >> 4) + 16 * j;
    if (RINGED) R = ring_slot<ROWS>(R);
    *(f32x4*)(lds + R * 64 + slot * 4) = v[j - J0];
    if (RINGED && R < RING_MIRROR) *(f32x4*)(lds + (R + ROWS) * 64 + slot * 4) = v[j - J0];
  }
}

// The 64 rows a chunk of conv64_wgrad_ring_kernel requests per operand, decomposed ONCE (rows64_load does it per row and thread:
// ~22 vector-ALU instructions per row, 8 rows per thread and chunk next to 288 MFMAs): entry of row R at (R & 15) * 4 + (R >> 4) =
// pixel index << 1 | 1, 0 = outside the tensor.  One wave builds one table (lane = row).
__device__ __forceinline__ void ring_tab_build(unsigned* __restrict__ tab, const ConvProg& P, int H, int W, int stride, int cls,
                                               int qstart, int R) {
  // (the walk of grid_pix<true> written out: this kernel scales by a shift — stride is 1 or 2 — where grid_pix multiplies, and through
  // the helper its generated code changes; rows64_load keeps its own incremental walk for the same reason)
  const int qq = qstart + R + P.PHW;  // shifted by one image: non-negative for the first rows of the first chunk
  const int n1 = fastdiv(qq, P.mPHW, P.sPHW);
  const int rem = qq - n1 * P.PHW;
  const int a = fastdiv(rem, P.mPW, P.sPW);
  const int y = (a << (stride - 1)) + (cls >> 1), x = ((rem - a * P.PW) << (stride - 1)) + (cls & 1);
  const bool ok = (unsigned)(n1 - 1) < (unsigned)P.N && y < H && x < W;
  tab[(R & 15) * 4 + (R >> 4)] = ok ? pix_entry(n1 - 1, y, x, H, W) : 0u;
}

// rows64_load through such a table (same loads, same zeros for rows outside)
__device__ __forceinline__ void rows64_load_tab(f32x4 (&v)[4], unsigned& okmask, const float* __restrict__ src,
                                                const unsigned* __restrict__ tab) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const float* __restrict__ base = src + (t & 15) * 4;
  const uint4 q = *(const uint4*)(tab + (t >> 4) * 4);
  const unsigned e[4] = {q.x, q.y, q.z, q.w};
  okmask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    okmask |= (e[j] & 1u) << j;
    if (e[j] & 1u) v[j] = *(const f32x4*)(base + ((e[j] & ~1u) << 5));  // (pixel index * 64 floats)
  }
}

// (Stride-1 programs only: the stride-2 form of this kernel, which walked a 64-position chunk class by class, was superseded by
// conv64_wgrad_ring_s2_kernel in round 2 and removed in round 5 — every program it took, span <= 118, the s2 kernel takes too.)
__global__ __launch_bounds__(256, 2) void conv64_wgrad_ring_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ g,
                                                                  float* __restrict__ partial, const ConvProg P,
                                                                  int nchunks, int chunks_per_wg, int wgs_per_group,
                                                                  const float* __restrict__ x_bnp) {
  // nchunks / chunks_per_wg describe ONE BatchNorm group; workgroups [g*wgs_per_group, (g+1)*wgs_per_group) walk group g
  constexpr int TK = 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ss = (float*)smem;        // ring: source row q lives at slot (q & 255)
  float* Gs = Ss + RING * 64;      // TK x 64: gradient rows of the current (chunk, destination class)
  unsigned* tabx = (unsigned*)(Gs + TK * 64);  // the 64 new source rows / the 64 gradient rows the current chunk requests
  unsigned* tabg = tabx + 64;                  //       (ring_tab_build)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int mi = wave & 1, nj = wave >> 1;
  // the tables of the requests chunk `c` makes: its successor's 64 new source rows and 64 gradient rows; waves 0 / 1 build one each
  auto next_tables = [&](int c) {
    const int q0 = c * TK;
    if (wave == 0) ring_tab_build(tabx, P, P.Hs, P.Ws, P.ss, P.tsrc[0], q0 + P.min_off + TK + P.span, lane);
    if (wave == 1) ring_tab_build(tabg, P, P.Hd, P.Wd, P.ds, P.tdst[0], q0 + TK, lane);
  };

  f32x16 acc[NTAPS];
#pragma unroll
  for (int t = 0; t < NTAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // bias gradient (column sums of the gradient rows): every gradient row passes through exactly one thread's registers on its
  // way into Gs, so the sums are taken there (channels [4*slot, 4*slot+4) of this thread's rows) instead of re-reading Gs
  f32x4 bs4 = {0.f, 0.f, 0.f, 0.f};

  const int cs = P.tsrc[0];  // the single source class (and a single destination class: one tap group of nine per chunk)

  const int grp = (P.G > 1) ? blockIdx.x / wgs_per_group : 0;
  x += grp * P.src_gstride;
  g += grp * P.dst_gstride;
  if (x_bnp) x_bnp += grp * 256;
  const BnQuad xq = bn_quad(x_bnp), noq = bn_quad(nullptr);
  const int c_begin = (blockIdx.x - grp * wgs_per_group) * chunks_per_wg;
  const int c_end = (c_begin + chunks_per_wg < nchunks) ? c_begin + chunks_per_wg : nchunks;
  if (c_begin < c_end) {
    // prologue: source rows [q0+min_off, q0+min_off+TK+span) of the first chunk, gradient rows of its first class
    const int q0 = c_begin * TK;
    f32x4 v[4];
    unsigned ok;
    for (int r0 = 0; r0 < TK + P.span; r0 += 64) {
      rows64_load(v, ok, x, P.Hs, P.Ws, P.ss, cs, P.PW, P.PH, P.total_q, q0 + P.min_off + r0, grid_div(P));
      rows64_store<true>(Ss, q0 + P.min_off + r0, v, ok, xq);
    }
    rows64_load(v, ok, g, P.Hd, P.Wd, P.ds, P.tdst[0], P.PW, P.PH, P.total_q, q0, grid_div(P));
    rows64_store<false>(Gs, 0, v, ok, noq);
    bs4 += (v[0] + v[1]) + (v[2] + v[3]);  // (rows outside the tensor are zero)
    next_tables(c_begin);
  }
  __syncthreads();

  unsigned oks = 0;
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    const int q0 = chunk * TK;
    const bool last_chunk = chunk + 1 >= c_end;
    {
      constexpr int t0 = 0, t1 = NTAPS;
      // ---- requests for what the NEXT chunk needs: its gradient rows and its 64 new source rows (they overwrite ring slots nobody
      //      reads after this chunk: RING_ROWS >= TK + span + TK keeps them outside the window the chunk still reads)
      f32x4 pg[4], ps[4];
      unsigned okg = 0;
      const bool want_g = !last_chunk, want_s = !last_chunk;
      if (want_g) rows64_load_tab(pg, okg, g, tabg);  // (rows q0 + TK ..: what next_tables(chunk) decomposed)
      if (want_s) rows64_load_tab(ps, oks, x, tabx);
      // ---- this group's work
      // 8 blocks of 4 k-steps; k-step i of block b multiplies grid rows q0 + 8b + 2i + h.  Per tap the ring slot of row
      // q0 + toff + 8b is wave-uniform (u[t], wrapped with scalar instructions); the 4 rows of a lane are u + h + {0,2,4,6}
      // — never past the mirror — i.e. one address and two ds_read2st64_b32 per tap and block.
      const float* gcol = Gs + (h * 64 + nj * 32 + l31);
      const float* scol = Ss + (h * 64 + mi * 32 + l31);
      int u[NTAPS];
#pragma unroll
      for (int t = t0; t < t1; ++t) u[t] = ring_slot(q0 + P.toff[t]);
#pragma unroll 1
      for (int b = 0; b < TK / 8; ++b) {
        float bf[4];
        int go = b * (8 * 64);
        asm volatile("" : "+v"(go));  // one address; the 4 rows are immediate offsets (Gs sits 64 KB into LDS: left to fold that
                                      // constant itself, the compiler needs one add and one ds_read_b32 per row).  The opaque value
                                      // is the OFFSET: laundering the pointer would lose the LDS address space (flat loads).
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = gcol[go + 2 * i * 64];
#pragma unroll
        for (int t = t0; t < t1; ++t) {
          const float* ap = scol + u[t] * 64;
          float af[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = ap[2 * i * 64];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[i], acc[t], 0, 0, 0);
          u[t] += 8;
          if (u[t] >= RING_ROWS) u[t] -= RING_ROWS;
        }
      }
      // ---- land the prefetched rows
      __syncthreads();
      if (want_g) {
        rows64_store<false>(Gs, 0, pg, okg, noq);
        bs4 += (pg[0] + pg[1]) + (pg[2] + pg[3]);
      }
      if (want_s) rows64_store<true, 0, 4>(Ss, q0 + P.min_off + TK + P.span, ps, oks, xq);
      if (!last_chunk) next_tables(chunk + 1);  // (this chunk's requests have been issued — and their table reads returned — long ago)
      __syncthreads();
    }
  }
  // partial[wg][9 (reference tap index)][64 ci][64 co] + [wg][64] bias sums after all workgroups' tap blocks
  float* out = partial + (size_t)blockIdx.x * (NTAPS * 4096);
#pragma unroll
  for (int t = 0; t < NTAPS; ++t) {
    float* o = out + (size_t)P.tw[t] * 4096;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      o[row * 64 + nj * 32 + l31] = acc[t][r];
    }
  }
  __syncthreads();  // (every wave is done with the ring)
  float* red = Ss;  // [16 row groups][64 channels]
  *(f32x4*)(red + (tid >> 4) * 64 + (tid & 15) * 4) = bs4;
  __syncthreads();
  if (tid < 64) {
    float* bout = partial + (size_t)gridDim.x * (NTAPS * 4096) + (size_t)blockIdx.x * 64;
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += red[r * 64 + tid];
    bout[tid] = t;
  }
}


// ---------------------------------------------------------------------------------------------------------------
// The same for stride-2 scatter programs (ConvTranspose weight gradients: one source class, four destination classes with
// 4 / 2 / 2 / 1 taps).  (Its predecessor walked a 64-position chunk class by class — four barrier pairs per chunk,
// the last of them around 32 MFMAs per wave.  Here a chunk is 32 positions and carries the gradient rows of ALL four classes
// (4 x 8 KB) next to a 184 + 8 row source ring (48 KB): one barrier pair per 144 MFMAs, every tap of a k-block shares the block's
// loads, and the prefetch (8 gradient + 2 source float4 per thread) travels under a whole chunk.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void conv64_wgrad_ring_s2_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                     float* __restrict__ partial, const ConvProg P, int nchunks,
                                                                     int chunks_per_wg, int wgs_per_group,
                                                                     const float* __restrict__ x_bnp) {
  constexpr int TK = 32;
  constexpr int GRP[NTAPS] = {0, 0, 0, 0, 1, 1, 2, 2, 3};  // destination-class group of tap t (taps are sorted 4/2/2/1)
  constexpr int GFIRST[4] = {0, 4, 6, 8};
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ss = (float*)smem;          // ring: source row q at slot q mod RING_ROWS_S2 (+ mirror)
  float* Gs = Ss + RING_S2 * 64;     // [4 classes][TK rows][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int mi = wave & 1, nj = wave >> 1;

  f32x16 acc[NTAPS];
#pragma unroll
  for (int t = 0; t < NTAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  f32x4 bs4 = {0.f, 0.f, 0.f, 0.f};

  const int cs = P.tsrc[0];
  const int grp = (P.G > 1) ? blockIdx.x / wgs_per_group : 0;
  x += grp * P.src_gstride;
  g += grp * P.dst_gstride;
  if (x_bnp) x_bnp += grp * 256;
  const BnQuad xq = bn_quad(x_bnp), noq = bn_quad(nullptr);
  const int c_begin = (blockIdx.x - grp * wgs_per_group) * chunks_per_wg;
  const int c_end = (c_begin + chunks_per_wg < nchunks) ? c_begin + chunks_per_wg : nchunks;

  f32x4 pg[4][2], ps[2];
  unsigned okg[4] = {0, 0, 0, 0}, oks = 0;
  auto g_request = [&](int q0_) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      rows64_load<0, 2>(pg[c], okg[c], g, P.Hd, P.Wd, P.ds, P.tdst[GFIRST[c]], P.PW, P.PH, P.total_q, q0_, grid_div(P));
  };
  auto g_land = [&]() {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      rows64_store<false, 0, 2>(Gs + c * TK * 64, 0, pg[c], okg[c], noq);
      bs4 += pg[c][0] + pg[c][1];  // (rows outside the tensor are zero)
    }
  };
  if (c_begin < c_end) {
    const int q0 = c_begin * TK;
    for (int r0 = 0; r0 < TK + P.span; r0 += 32) {
      rows64_load<0, 2>(ps, oks, x, P.Hs, P.Ws, P.ss, cs, P.PW, P.PH, P.total_q, q0 + P.min_off + r0, grid_div(P));
      rows64_store<true, 0, 2, RING_ROWS_S2>(Ss, q0 + P.min_off + r0, ps, oks, xq);
    }
    g_request(q0);
    g_land();
  }
  __syncthreads();

  const float* gcol = Gs + (h * 64 + nj * 32 + l31);
  const float* scol = Ss + (h * 64 + mi * 32 + l31);
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    const int q0 = chunk * TK;
    const bool more = chunk + 1 < c_end;
    if (more) {
      g_request(q0 + TK);
      rows64_load<0, 2>(ps, oks, x, P.Hs, P.Ws, P.ss, cs, P.PW, P.PH, P.total_q, q0 + P.min_off + TK + P.span, grid_div(P));
    }
    int u[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) u[t] = ring_slot<RING_ROWS_S2>(q0 + P.toff[t]);
#pragma unroll 1
    for (int b = 0; b < TK / 8; ++b) {
      int go = b * (8 * 64);
      asm volatile("" : "+v"(go));  // (one address per class; see conv64_wgrad_ring_kernel)
      float bf[4][4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[c][i] = gcol[c * TK * 64 + go + 2 * i * 64];
#pragma unroll
      for (int t = 0; t < NTAPS; ++t) {
        const float* ap = scol + u[t] * 64;
        float af[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = ap[2 * i * 64];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[GRP[t]][i], acc[t], 0, 0, 0);
        u[t] += 8;
        if (u[t] >= RING_ROWS_S2) u[t] -= RING_ROWS_S2;
      }
    }
    __syncthreads();  // every wave is done with this chunk's gradient rows (and with the ring slots the new rows replace)
    if (more) {
      g_land();
      rows64_store<true, 0, 2, RING_ROWS_S2>(Ss, q0 + P.min_off + TK + P.span, ps, oks, xq);
    }
    __syncthreads();
  }
  float* out = partial + (size_t)blockIdx.x * (NTAPS * 4096);
#pragma unroll
  for (int t = 0; t < NTAPS; ++t) {
    float* o = out + (size_t)P.tw[t] * 4096;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      o[row * 64 + nj * 32 + l31] = acc[t][r];
    }
  }
  __syncthreads();
  float* red = Ss;  // [16 row groups][64 channels]
  *(f32x4*)(red + (tid >> 4) * 64 + (tid & 15) * 4) = bs4;
  __syncthreads();
  if (tid < 64) {
    float* bout = partial + (size_t)gridDim.x * (NTAPS * 4096) + (size_t)blockIdx.x * 64;
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += red[r * 64 + tid];
    bout[tid] = t;
  }
}

// dw_ref[...] = sum over workgroups (fixed order); layout: conv [co][ci][3][3], convT [ci][co][3][3].
// 1024 threads per block: 256 outputs x 4 slices of the workgroup range, 4 loads in flight per thread, fp64 combine.
__global__ __launch_bounds__(1024) void conv64_wgrad_reduce(const float* __restrict__ partial, int nwg,
                                                           float* __restrict__ dw_ref, float* __restrict__ dbias,
                                                           int transposed, int interleaved) {
  const int o = threadIdx.x & 255, part = threadIdx.x >> 8;
  const int id = blockIdx.x * 256 + o;
  constexpr int TOT = NTAPS * 4096;
  const int per = (nwg + 3) / 4;
  const int w0 = part * per, w1 = (w0 + per < nwg) ? w0 + per : nwg;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (id < TOT + 64) {
    // bias partials live after all workgroups' tap blocks: [nwg][64] — or, interleaved (= the record size), behind each workgroup's own
    const float* base = interleaved ? partial + id : (id < TOT) ? partial + id : partial + (size_t)nwg * TOT + (id - TOT);
    const size_t stride = interleaved ? (size_t)interleaved : (id < TOT) ? (size_t)TOT : 64;
    int w = w0;
    for (; w + 3 < w1; w += 4) {
      s0 += (double)base[(size_t)w * stride];
      s1 += (double)base[(size_t)(w + 1) * stride];
      s2 += (double)base[(size_t)(w + 2) * stride];
      s3 += (double)base[(size_t)(w + 3) * stride];
    }
    for (; w < w1; ++w) s0 += (double)base[(size_t)w * stride];
  }
  __shared__ double sm[4][256];
  sm[part][o] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (part == 0 && id < TOT + 64) {
    const double s = (sm[0][o] + sm[1][o]) + (sm[2][o] + sm[3][o]);
    if (id < TOT) {
      const int tap = id >> 12, ci = (id >> 6) & 63, co = id & 63;
      dw_ref[transposed ? ((ci * 64 + co) * 9 + tap) : ((co * 64 + ci) * 9 + tap)] = (float)s;
    } else if (dbias) {
      dbias[id - TOT] = (float)s;
    }
  }
}

static size_t wgrad_lds_bytes(const ConvProg& P) { return (size_t)(WG_TK + P.span + WG_TK) * 256; }

// The weight gradient is a chain of SHAPE fallbacks (no environment switches):
//   ring_s2  ConvTranspose programs (one source class, taps {4, 2, 2, 1} by destination class) whose span fits the 184-row ring
//            (PW <= 119): conv64_wgrad_ring_s2_kernel, 32-position chunks carrying all four destination classes;
//   ring     stride-1 programs whose span fits the 246-row ring (PW <= 58), with the 32-bit offsets of its row tables:
//            conv64_wgrad_ring_kernel;
//   gather   stride-2 gather programs (conv3) with a plain source, chunk + halo within a thread's registers, 32-bit offsets:
//            conv64_wgrad_gather_kernel (same grid, same partials as conv64_wgrad_kernel<true, 64>);
//   chunk    anything else (wider images, a gradient rebuilt from (dA, y)): the chunk-at-a-time conv64_wgrad_kernel.
// x_bnp: the source is relu(bn(x)); dy_bn_y: the gradient is rebuilt from (dA, y) (srlz_bn_bwd_operand).
enum class WgradRoute { ring_s2, ring, gather, chunk };
static WgradRoute wgrad_route(const ConvProg& P, bool x_bnp, bool dy_bn_y) {
  bool single_src = true;
  for (int t = 1; t < NTAPS; ++t) single_src = single_src && P.tsrc[t] == P.tsrc[0];
  if (single_src && !dy_bn_y && P.s2 && 32 + P.span + 32 <= RING_ROWS_S2) return WgradRoute::ring_s2;
  if (single_src && !dy_bn_y && !P.s2 && WG_TK + P.span + WG_TK <= RING_ROWS && fits_32bit_src_floats(P) && fits_32bit_dst_floats(P) &&
      fits_31bit_grid(P, P.PHW))
    return WgradRoute::ring;
  if (taps_grouped_4221(P) && WG_TK + P.span <= 16 * WG_SROWS && fits_32bit_src_floats(P) && fits_32bit_dst_floats(P) &&
      fits_31bit_grid(P, WG_TK + P.span) && !x_bnp && !dy_bn_y)
    return WgradRoute::gather;
  return WgradRoute::chunk;
}

// workgroups of the weight-gradient kernels (all groups together); a multiple of P.G
static int wgrad_grid(const ConvProg& P) {
  const int nchunks = (P.total_q + WG_TK - 1) / WG_TK;  // per group
  int g = 2 * srlz_device_cus() / P.G;           // two persistent workgroups per CU; per group
  // (Fewer, longer-running workgroups on the small layers — at least 8 chunks each, to halve the 147 KB partial every workgroup
  // leaves for the second stage — were measured in round 4 and lost: conv3's weight gradient 121 -> 172 us, ConvT1's 31 -> 102 us,
  // the bs = 32 step 2.49 -> 2.70 ms.  These launches are bound by how many CUs work, not by the partials' traffic.)
  if (g > nchunks) g = nchunks;
  if (g < 1) g = 1;
  return g * P.G;
}

// What srlz_conv64_bwd_weight launches, decided in one place (srlz_conv64_bwd_weight_plan answers from the same record):
// nch chunks of tk positions per BatchNorm group on `launched` workgroups.  The ring kernels give every workgroup a contiguous
// range of cpw chunks (ring re-use of the source rows), group by group, on wpg <= grid / G workgroups per group; the gather and
// chunk kernels stride over all G * nch chunks by the whole grid (cpw = the most chunks any workgroup takes).
struct WgradPlan {
  WgradRoute route;
  int grid;      // wgrad_grid(P): what the workspace is sized for
  int launched;  // workgroups launched (<= grid) = partial records for the second stage
  int nch, tk, cpw, wpg;
};
static WgradPlan wgrad_plan(const ConvProg& P, bool x_bnp, bool dy_bn_y) {
  WgradPlan w;
  w.route = wgrad_route(P, x_bnp, dy_bn_y);
  w.grid = wgrad_grid(P);
  w.tk = w.route == WgradRoute::ring_s2 ? 32 : WG_TK;
  w.nch = (P.total_q + w.tk - 1) / w.tk;  // per BatchNorm group
  const int gpg = w.grid / P.G;
  if (w.route == WgradRoute::ring_s2 || w.route == WgradRoute::ring) {
    w.cpw = (w.nch + gpg - 1) / gpg;
    w.wpg = (w.nch + w.cpw - 1) / w.cpw;
    w.launched = w.wpg * P.G;
  } else {
    w.cpw = (w.nch * P.G + w.grid - 1) / w.grid;
    w.wpg = gpg;
    w.launched = w.grid;
  }
  return w;
}

}  // namespace

// The second stage behind every kernel that leaves per-workgroup partials: srlz_conv64_bwd_weight below and the fused backward
// (conv64_pipe.hip), whose partials keep their bias block behind each workgroup's taps (interleaved = the record size)
int conv64::launch_wgrad_reduce(const float* partial, int nwg, float* dw_ref, float* dbias, int transposed, int interleaved,
                                hipStream_t st) {
  SRLZ_LAUNCH(conv64_wgrad_reduce, dim3((WGRAD_PARTIAL_FLOATS + 255) / 256), dim3(1024), 0, st, partial, nwg, dw_ref, dbias, transposed,
              interleaved);
  return 0;
}

extern "C" size_t srlz_conv64_bwd_weight_workspace(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 0, &P)) return 0;
  return (size_t)wgrad_grid(P) * WGRAD_PARTIAL_FLOATS * sizeof(float);
}

// Host only: the plan srlz_conv64_bwd_weight would launch.  out = {route (0 ring_s2, 1 ring, 2 gather, 3 chunk), workgroups launched,
// chunks per workgroup, positions per chunk}.
extern "C" int srlz_conv64_bwd_weight_plan(const srlz_conv64_desc* d, int has_x_bnp, int has_dy_bn, int out[4]) {
  SRLZ_REQUIRE(out, SRLZ_ERR_NULL, "conv64_bwd_weight_plan: null pointer");
  ConvProg P;
  if (int rc = conv64::with_program(d, 0, &P)) return rc;
  const WgradPlan w = wgrad_plan(P, has_x_bnp != 0, has_dy_bn != 0);
  out[0] = (int)w.route;
  out[1] = w.launched;
  out[2] = w.cpw;
  out[3] = w.tk;
  return 0;
}

extern "C" int srlz_conv64_bwd_weight(const float* x, const float* dy, float* dw_ref, float* dbias, const float* x_bnp,
                                      const srlz_bn_bwd_operand* dy_bn, void* ws, size_t ws_bytes,
                                      const srlz_conv64_desc* d, srlz_stream_t stream) {
  ConvProg P;
  if (int rc = conv64::with_program(d, 0, &P)) return rc;
  OpFuse gf;
  if (int rc = make_bwd_fuse(&gf, dy_bn, "conv64_bwd_weight")) return rc;
  SRLZ_REQUIRE(gf.dy_out == nullptr, SRLZ_ERR_BAD_DESC, "conv64_bwd_weight: dy_out is only produced by srlz_conv64_bwd_data");
  const OpFuse xf = OpFuse{x_bnp, nullptr, nullptr, 0.f, 0, nullptr};
  SRLZ_REQUIRE(x && dy && dw_ref && ws, SRLZ_ERR_NULL, "conv64_bwd_weight: null pointer");
  const WgradPlan w = wgrad_plan(P, x_bnp != nullptr, gf.y != nullptr);
  SRLZ_REQUIRE(ws_bytes >= (size_t)w.grid * WGRAD_PARTIAL_FLOATS * sizeof(float), SRLZ_ERR_WORKSPACE,
               "conv64_bwd_weight: workspace too small (%zu bytes)", ws_bytes);
  hipStream_t st = as_stream(stream);
  float* partial = (float*)ws;
  switch (w.route) {
    case WgradRoute::ring_s2: {
      const size_t lds = (size_t)(RING_S2 + 4 * 32) * 256;
      SRLZ_MAX_LDS(conv64_wgrad_ring_s2_kernel, lds);
      SRLZ_LAUNCH(conv64_wgrad_ring_s2_kernel, dim3(w.launched), dim3(256), lds, st, x, dy, partial, P, w.nch, w.cpw, w.wpg, x_bnp);
      break;
    }
    case WgradRoute::ring: {
      const size_t lds = (size_t)(RING + 64) * 256 + 2 * 64 * 4;  // ring + gradient rows + the two row tables = 80 KB
      SRLZ_MAX_LDS(conv64_wgrad_ring_kernel, lds);
      SRLZ_LAUNCH(conv64_wgrad_ring_kernel, dim3(w.launched), dim3(256), lds, st, x, dy, partial, P, w.nch, w.cpw, w.wpg, x_bnp);
      break;
    }
    case WgradRoute::gather: {
      const size_t lds = wgrad_lds_bytes(P) + (WG_SWORDS + WG_GWORDS) * 4;
      SRLZ_MAX_LDS(conv64_wgrad_gather_kernel, lds);
      SRLZ_LAUNCH(conv64_wgrad_gather_kernel, dim3(w.launched), dim3(256), lds, st, x, dy, partial, P, w.nch * P.G);
      break;
    }
    case WgradRoute::chunk: {
      const size_t lds = wgrad_lds_bytes(P);
      SRLZ_REQUIRE(lds <= 160 * 1024, SRLZ_ERR_BAD_DESC, "conv64 wgrad: chunk needs %zu bytes of LDS", lds);
      if (P.s2) {
        SRLZ_MAX_LDS((conv64_wgrad_kernel<true, WG_TK>), lds);
        SRLZ_LAUNCH((conv64_wgrad_kernel<true, WG_TK>), dim3(w.launched), dim3(256), lds, st, x, dy, partial, P, w.nch * P.G, xf, gf);
      } else {
        SRLZ_MAX_LDS((conv64_wgrad_kernel<false, WG_TK>), lds);
        SRLZ_LAUNCH((conv64_wgrad_kernel<false, WG_TK>), dim3(w.launched), dim3(256), lds, st, x, dy, partial, P, w.nch * P.G, xf, gf);
      }
      break;
    }
  }
  return conv64::launch_wgrad_reduce(partial, w.launched, dw_ref, dbias, d->transposed, 0, st);
}
