// conv64_pipe.hip — the software-pipelined persistent kernels of the 3x3, 64 -> 64 stride-2 programs (formulation: conv64.hip): the gather
// programs' two, described next, and the scatter programs' conv64_scatter_pipe_kernel (a ConvTranspose's forward), described at its place.
//
// ---------------------------------------------------------------------------------------------------------------
// Software-pipelined, persistent kernels of the stride-2 gather programs (conv64_bwd_fused_kernel: the whole backward of a
// ConvTranspose block; conv64_gather_pipe_kernel: plain operands).  A stride-2 gather tile stages its source FOUR times (one class of
// 128 + span rows per tap group 4 / 2 / 2 / 1), and in conv64_fwd_kernel every one of those stagings is a synchronous HBM round trip
// between two barriers.  Here
//  * the rows of class c+1 are REQUESTED into registers right after the barrier that opens the first tap of class c and LAND
//    in LDS after the barrier that closes its last tap: they travel under 4 / 2 / 2 taps of MFMAs; the requests are branch-free
//    (clamped addresses, masks applied at the landing), so hipcc's wait insertion keeps them in flight;
//  * workgroups are persistent and walk a contiguous run of their XCD's tiles, so class 0 of the NEXT tile travels under the single
//    tap of class 3 and the epilogue, and the weight slab of tap 0 under tap 8;
//  * the tap structure is compile-time (groups {0..3}, {4, 5}, {6, 7}, {8}): no run-time class switch inside the pipeline.
// (Round 3's conv64_dgrad_pipe_kernel — the fused data gradient alone, with the rebuilt gradient stored for a separate weight-gradient
// launch — was the first of this family; conv64_bwd_fused_kernel took over every shape it served and it was removed in round 5.)
// ---------------------------------------------------------------------------------------------------------------
#include "conv64_tile.h"

namespace {

constexpr int GP_THREADS = 512;                 // 8 waves: wave = 32 rows x 32 columns, one accumulator (the rows of a class in
constexpr int GP_RP = GP_THREADS / 16;          // flight cost 376 bytes per thread at 256 threads — with the 4-wave kernel's 64
constexpr int GP_BATCH = 6;                     // accumulator registers on top, that spills; at 512 threads it is 48 + 16)
constexpr int GP_CORE = TM / GP_RP;             // a tile's own rows are its first TM (these programs have min_off == 0)
                                                // rows per pass / rows (of 16 lanes) per thread and class: 128 + span <= 192

struct GatherRows {
  f32x4 v[GP_BATCH], yv[GP_BATCH];
  unsigned offs[GP_CORE];   // float offset of the rows that can lie in the tile's own range (dy_out is indexed like y)
  unsigned ok;              // bit j: row j lies inside the tensor
};

// The source-side row table of a gather tile (cf. rowtab_build): the walk over (image, row, column), the bounds tests and the pixel
// offset of a tile's rows were redone by every thread for each of the tile's four classes (~22 vector-ALU instructions per row and
// class); here the first 192 threads decompose one row each, once per tile (src_entry).
// Layout: row R at (R & 31) * GT_P + (R >> 5): the six rows of thread t (R = (t >> 4) + 32 j) are consecutive words.
// SHIFTED: the staged range [qstart, qstart + nrows) may begin before grid position 0 (qstart >= -PHW: a convolution with padding);
// the fused backward's programs have min_off == 0 and build it unshifted.
constexpr int GT_P = 8;
constexpr int GT_WORDS = GP_RP * GT_P;
template <bool SHIFTED>
__device__ __forceinline__ void gtab_build(unsigned* __restrict__ tab, const ConvProg& P, int qstart, int nrows) {
  int R = threadIdx.x;
  asm volatile("" : "+v"(R));  // opaque (as in gather_request): the word's address is not worth a register across the tile loop
  if (R < GT_WORDS) {
    unsigned e = 0;
    if (R < nrows) e = src_entry<SHIFTED>(P, qstart + R, 2);
    tab[(R & (GP_RP - 1)) * GT_P + (R >> 5)] = e;
  }
}

// NJ: how many of the thread's six rows (32 j + (t >> 4)) this class needs — a class whose taps reach at most `off` positions ahead
// reads rows [0, TM + off) of its buffer, so the 2-tap class with offsets {0, 1} needs 129 rows (NJ = 5) and the 1-tap class 128
// (NJ = 4): the rows beyond were requested, rebuilt and landed for nobody (3 of a tile's 24 row slots per thread; round 6).
template <int NJ = GP_BATCH>
__device__ __forceinline__ void gather_request(GatherRows& r, const float* __restrict__ src, const float* __restrict__ y,
                                               const unsigned* __restrict__ tab, int cls, int W) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));  // opaque: nothing derived from the thread index here is worth a register across the tile loop
  const int slot = t & 15;
  const unsigned delta = (unsigned)((cls >> 1) * W + (cls & 1));
  const unsigned* __restrict__ tp = tab + (t >> 4) * GT_P;
  const uint4 e03 = *(const uint4*)tp;
  uint2 e45 = {0u, 0u};
  if constexpr (NJ > 4) e45 = *(const uint2*)(tp + 4);
  const unsigned e[GP_BATCH] = {e03.x, e03.y, e03.z, e03.w, e45.x, e45.y};
  static_assert(GP_BATCH == 6 && NJ >= GP_CORE && NJ <= GP_BATCH, "the table read above takes six rows");
  unsigned okmask = 0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    // branch-free: m = all ones where the row's pixel of this class exists; any other row reads pixel 0 and is zeroed when it lands
    const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)e[j], (unsigned)cls, 1u);
    const unsigned off = ((((e[j] >> 4) + delta) << 6) & m) + slot * 4;
    r.v[j] = *(const f32x4*)(src + off);
    r.yv[j] = *(const f32x4*)(y + off);
    if (j < GP_CORE) r.offs[j] = off;
    okmask |= m & (1u << j);
  }
  r.ok = okmask;
}

// Branch-free conditional stores through a buffer resource (common.h: raw_buffer): offset = GP_DROP for a lane that must not write.
constexpr unsigned GP_DROP = 0xFFFFFF00u;

// ---------------------------------------------------------------------------------------------------------------
// The stride-2 gather programs with a PLAIN operand — conv3's forward (27x27 -> 14x14, with the BatchNorm statistics of its output)
// and the data gradient of the decoder's first ConvTranspose — software-pipelined like conv64_bwd_fused_kernel's data-gradient half (round 5).
// In conv64_fwd_kernel<4, false> such a tile stages its four source classes in four synchronous HBM round trips between barriers,
// and conv3 has only 900 tiles of them for 512 workgroup slots: 102 us for 47 us of matrix work.  Here, as in the fused kernel above:
// persistent workgroups (2 per CU) walk their XCD's tiles, class c + 1 is requested behind the barrier that opens class c and lands
// behind its last tap, class 0 of the next tile travels under the single tap of class 3 and the epilogue; branch-free requests and
// stores.  Differences: no BatchNorm-backward rebuild, no dy_out; the programs of a convolution with padding start their staged range
// at a NEGATIVE grid offset (min_off < 0: the row table is built SHIFTED); the epilogue takes the
// per-tile BatchNorm partial sums (sum y, sum y^2 over the tile's valid rows) like conv64_fwd_kernel's, in this kernel's own
// (fixed) summation order.  Same tiles, same accumulation order of the contraction: y is bit-identical to conv64_fwd_kernel's.
// ---------------------------------------------------------------------------------------------------------------
struct PlainRows {
  f32x4 v[GP_BATCH];
  unsigned ok;
};

__device__ __forceinline__ void plain_request(PlainRows& r, const float* __restrict__ src, const unsigned* __restrict__ tab, int cls,
                                              int W) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int slot = t & 15;
  const unsigned delta = (unsigned)((cls >> 1) * W + (cls & 1));
  const unsigned* __restrict__ tp = tab + (t >> 4) * GT_P;
  const uint4 e03 = *(const uint4*)tp;
  const uint2 e45 = *(const uint2*)(tp + 4);
  const unsigned e[GP_BATCH] = {e03.x, e03.y, e03.z, e03.w, e45.x, e45.y};
  unsigned okmask = 0;
#pragma unroll
  for (int j = 0; j < GP_BATCH; ++j) {
    const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)e[j], (unsigned)cls, 1u);  // all ones where the row's pixel of this class exists
    const unsigned off = ((((e[j] >> 4) + delta) << 6) & m) + slot * 4;                // (any other row reads pixel 0; zeroed at the landing)
    r.v[j] = *(const f32x4*)(src + off);
    okmask |= m & (1u << j);
  }
  r.ok = okmask;
}

__device__ __forceinline__ void plain_land(float* __restrict__ lds, PlainRows& r, int nrows) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int slot = t & 15;
#pragma unroll
  for (int j = 0; j < GP_BATCH; ++j) {
    const int R = (t >> 4) + GP_RP * j;
    const f32x4 v = ((r.ok >> j) & 1u) ? r.v[j] : f32x4{0.f, 0.f, 0.f, 0.f};
    if (R < nrows) *(f32x4*)(lds + R * 64 + ((slot ^ (R & 15)) << 2)) = v;
  }
}

__global__ __launch_bounds__(GP_THREADS, 4) void conv64_gather_pipe_kernel(const float* __restrict__ src_all,
                                                                          const float* __restrict__ wpack,
                                                                          float* __restrict__ dst_all,
                                                                          float* __restrict__ stats_partial, const ConvProg P,
                                                                          int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* As = (float*)smem;                 // (TM + span) x 64, swizzled: the rows of the current class
  float* Bs = As + (TM + P.span) * 64;      // 64 x 64 weight slab of the current tap
  int* rowinfo = (int*)(Bs + 4096);         // [2 (tile parity)][3][TM]: image index (or -1), a*ds, b*ds
  unsigned* gtab = (unsigned*)(rowinfo + 6 * TM);  // the source-side row table of the tile whose rows are being requested
  float* red = (float*)(gtab + GT_WORDS);   // [8 waves][sum 32 | sum of squares 32]: the tile's BatchNorm partials on their way out

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int nrows = TM + P.span;
  const int cls0 = P.tsrc[0], cls1 = P.tsrc[4], cls2 = P.tsrc[6], cls3 = P.tsrc[8];

  const int xcd = blockIdx.x & 7, wi = blockIdx.x >> 3, wpx = gridDim.x >> 3;
  const int tq = ntiles >> 3, tr = ntiles & 7;
  const int tbase = (xcd < tr) ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
  const int tcnt = tq + (xcd < tr ? 1 : 0);

  constexpr int BV = 1024 / GP_THREADS;
  const int bslot = wave * (BV * 64) + lane;
  f32x4 breg[BV];
  {
    const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[0] * 4096);
#pragma unroll
    for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot + i * 64];
  }
  const unsigned dst_bytes = (unsigned)P.dst_gstride * 4u;

  PlainRows rr;
  int k = wi;
  int parity = 0;
  if (k < tcnt) {  // the first tile's class 0 is staged the plain way
    const int tile = tbase + k;
    const int grp = (P.G > 1 && tile >= P.tpg) ? 1 : 0;  // (G <= 2, checked by the host)
    const int q0 = (tile - grp * P.tpg) * TM;
    gtab_build<true>(gtab, P, q0 + P.min_off, nrows);
    __syncthreads();
    plain_request(rr, src_all + grp * P.src_gstride, gtab, cls0, P.Ws);
    plain_land(As, rr, nrows);
  }
  for (; k < tcnt; k += wpx, parity ^= 1) {
    const int tile = tbase + k;
    const int grp = (P.G > 1 && tile >= P.tpg) ? 1 : 0;
    const int q0 = (tile - grp * P.tpg) * TM;
    const float* __restrict__ src = src_all + grp * P.src_gstride;
    const __amdgpu_buffer_rsrc_t dst = raw_buffer(dst_all + grp * P.dst_gstride, dst_bytes);
    const int k2 = k + wpx;  // this workgroup's next tile (past the end: this one again, with no rows)
    const int tile2 = tbase + (k2 < tcnt ? k2 : k);
    const int grp2 = (P.G > 1 && tile2 >= P.tpg) ? 1 : 0;
    const int q02 = (tile2 - grp2 * P.tpg) * TM;
    int* ri = rowinfo + parity * (3 * TM);
    if (tid < TM) {  // (the other parity's copy may still be read by a wave that is flushing the previous tile)
      const int q = q0 + tid;
      int n = -1, ya = 0, xb = 0;
      if (q < P.total_q) {
        const GridPix g = grid_pix<false>(P, q, P.ds);
        n = g.n; ya = g.y; xb = g.x;
      }
      ri[tid] = n; ri[TM + tid] = ya; ri[2 * TM + tid] = xb;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    int tid_t = tid;  // (one opaque copy of the thread index per tile: what the nine taps derive from it must not live in registers
                      // across the tile loop, or the rows in flight are pushed into scratch)
    asm volatile("" : "+v"(tid_t));
    const int lane_t = tid_t & 63, wave_t = tid_t >> 6;
    const int wrow_t = wave_t & 3, wcol_t = wave_t >> 2;
    const int h_t = lane_t >> 5, l31_t = lane_t & 31;
    const int arow0 = wrow_t * 32 + l31_t - P.min_off;
    const float* brow = Bs + (wcol_t * 32 + l31_t) * 64;
    const int bkey = lane_t & 15;
    const int bslot_t = wave_t * (BV * 64) + lane_t;

#pragma unroll
    for (int ti = 0; ti < NTAPS; ++ti) {
      __syncthreads();  // all waves are done with the previous tap's Bs — and with As when this tap opens a new class
      {
        f32x4* wdst = (f32x4*)Bs;
#pragma unroll
        for (int i = 0; i < BV; ++i) wdst[bslot_t + i * 64] = breg[i];
      }
      {  // the next tap's slab (tap 0 of the next tile behind tap 8: same weights)
        const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[(ti + 1) % NTAPS] * 4096);
#pragma unroll
        for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot_t + i * 64];
      }
      if (ti == 4 || ti == 6 || ti == 8) plain_land(As, rr, nrows);
      if (ti == 7) gtab_build<true>(gtab, P, q02 + P.min_off, k2 < tcnt ? nrows : 0);
      __syncthreads();
      if (ti == 0) plain_request(rr, src, gtab, cls1, P.Ws);
      if (ti == 4) plain_request(rr, src, gtab, cls2, P.Ws);
      if (ti == 6) plain_request(rr, src, gtab, cls3, P.Ws);
      if (ti == 8) plain_request(rr, src_all + grp2 * P.src_gstride, gtab, cls0, P.Ws);  // class 0 of this workgroup's NEXT tile
      __builtin_amdgcn_sched_barrier(0);  // every request goes out HERE, ahead of the tap's MFMAs
      const int R = arow0 + P.toff[ti];
      int abase = (R * 64 + ((h_t ^ (R & 15)) << 2)) * 4;  // bytes; slot (2kc + h) ^ (R & 15) is this XOR (kc << 5)
      asm volatile("" : "+v"(abase));
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        const f32x4 a = *(const f32x4*)((const char*)As + (abase ^ (kc << 5)));
        const f32x4 b = *(const f32x4*)(brow + (((kc * 2 + h_t) ^ bkey) << 2));
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[r], acc, 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done with the last tap's slab and with As: Bs becomes scratch, As takes the next tile
    if (k + wpx < tcnt) plain_land(As, rr, nrows);  // (the landing first: it waits for its rows only)
    {  // flush through this wave's own 2 KB of the idle slab, 16 tile rows x 32 columns at a time: 16-byte stores, branch-free
      int tid_f = tid;
      asm volatile("" : "+v"(tid_f));
      const int lane_f = tid_f & 63, wave_f = tid_f >> 6;
      const int wrow_f = wave_f & 3, wcol_f = wave_f >> 2, h_f = lane_f >> 5, l31_f = lane_f & 31;
      float* S = Bs + wave_f * 512;
      const int eg = lane_f >> 3, eslot = lane_f & 7;
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int rq = 0; rq < 8; ++rq) {
          const int rowl = (rq & 3) + 8 * (rq >> 2) + 4 * h_f;
          S[rowl * 32 + l31_f] = acc[8 * half + rq];
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int rowl = eg + 8 * kk;
          const int row = wrow_f * 32 + 16 * half + rowl;
          const f32x4 v = *(const f32x4*)(S + rowl * 32 + eslot * 4);
          const int n = ri[row];
          const int y = ri[TM + row], x = ri[2 * TM + row];
          const bool inside = n >= 0 && y < P.Hd && x < P.Wd;
          __builtin_amdgcn_raw_buffer_store_b128(v, dst, inside ? (unsigned)((n * P.Hd + y) * P.Wd + x) * 256u + wcol_f * 128 + eslot * 16 : GP_DROP,
                                                 0, 0);
          const f32x4 vv = inside ? v : f32x4{0.f, 0.f, 0.f, 0.f};
          s4 += vv;
          q4 += vv * vv;
        }
      }
      if (stats_partial) {
        // this lane's four channels (32 wcol + 4 eslot ..) over its four rows; the eight row groups of the wave (lane bits 3-5), then
        // the four row-waves of a column half through LDS; fixed order
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s4[e] += __shfl_xor(s4[e], 8, 64); s4[e] += __shfl_xor(s4[e], 16, 64); s4[e] += __shfl_xor(s4[e], 32, 64);
          q4[e] += __shfl_xor(q4[e], 8, 64); q4[e] += __shfl_xor(q4[e], 16, 64); q4[e] += __shfl_xor(q4[e], 32, 64);
        }
        if (lane_f < 8) {
          *(f32x4*)(red + wave_f * 64 + lane_f * 4) = s4;
          *(f32x4*)(red + wave_f * 64 + 32 + lane_f * 4) = q4;
        }
        __syncthreads();
        if (tid_f < 128) {
          const int c = tid_f & 63, which = tid_f >> 6;  // [0, 64): sum, [64, 128): sum of squares
          const float* base = red + ((c >> 5) * 4) * 64 + which * 32 + (c & 31);  // waves 4 wcol + wrow
          stats_partial[(size_t)tile * 128 + tid_f] = (base[0] + base[64]) + (base[128] + base[192]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The WHOLE backward of a decoder block's ConvTranspose2d(64, 64, 3, stride 2) in one launch: data gradient, weight gradient and
// bias gradient from ONE staging of the rebuilt d(loss)/dy.
// A separate fused data-gradient launch reads (dA, y) = 3.2 GB at the 111x111 layer, rebuilds dy and — only so that the weight-gradient
// kernel can read it back — stores it (1.6 GB written, 1.6 GB read again).  Both contractions consume the same operand:
//     da(p)  = sum_t dy_{c_t}(p + off_t) . Wb[t]          (M = positions, N = ci, K = co)
//     dW[t]  = sum_p a(p)^T . dy_{c_t}(p + off_t)         (M = ci, N = co, K = positions),    a = relu(bn(y_prev)),
// so here a tile (128 positions p of the low-resolution grid) stages each class of dy rows once in LDS, runs the data-gradient
// taps on it as the pipelined kernel does, and ALSO multiplies it with the tile's 128 rows of a.  dy never leaves the chip:
// 3.2 GB of the pair's 7.2 GB disappear, and the MFMA work per staged byte doubles.
//  * 512 threads, ONE workgroup per CU (256 registers per lane, 150 KB of LDS): the class rows are double-buffered in LDS, so a
//    class lands two taps after it was requested — where the in-order vmcnt completes its loads anyway — while the previous
//    class is still being read; the a-tile of the next tile lands at the tile boundary.
//  * data gradient: wave = 32 positions x 32 channels (as conv64_gather_pipe_kernel).  Weight gradient: the 36 blocks
//    (9 taps x 2x2 quadrants of 32x32) are spread over the 8 waves per CLASS so that every wave has 32 weight-gradient MFMAs
//    in every tap period: class of 4 taps — wave w owns tap (w >> 1), quadrants (w & 1, {0, 1}), a quarter of the positions per
//    period; classes of 2 taps — tap (w >> 2), quadrant (w & 1, (w >> 1) & 1), half of the positions per period; the 1-tap
//    class — quadrant as before, position half (w >> 2), the two halves added through LDS at the end.  80 accumulator
//    registers per lane instead of 144.
//  * positions are visited as p = 16 i + jj + 8 h (h = the MFMA's two k-lanes): for fixed (jj, h) the rows 16 i apart share the
//    XOR key of the swizzled dy rows, so a lane reaches its eight k-steps from ONE address with immediate offsets
//    (ds_read2st64_b32), for the dy operand as for the (unswizzled) a-tile.
// Results: dx bit-identical to conv64_fwd_kernel<4, true>'s; dW / db differ from the two-kernel path by summation order only
// (per-workgroup partials, fixed-order fp64 second stage: deterministic).
// ---------------------------------------------------------------------------------------------------------------
// which channels of a BatchNorm record cannot give xhat back from the activation (shared by the fused kernel and its companion)
__host__ __device__ __forceinline__ bool bnpart_zero_scale(float scale, float shift) {
  return fabsf(scale) <= 1e-3f * fabsf(shift) || scale == 0.f;
}

// Folding one lane bit of TWO per-lane values with one add (gfx950): fold32(a, b) = { a[l] + a[l + 32] in lanes l < 32, b[l - 32] + b[l]
// in lanes l >= 32 };  fold16(a, b) = { a's rows (16 lanes) 0 + 1 in row 0, b's rows 0 + 1 in row 1, a's 2 + 3 in row 2, b's 2 + 3 in row 3 }.
__device__ __forceinline__ float fold32(float a, float b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float fold16(float a, float b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

struct FusedBwd {
  const float* x;        // raw y_prev [N, Hd, Wd, 64] (the ConvTranspose's input before BatchNorm + ReLU)
  const float* x_bnp;    // its BatchNorm record(s): a = relu(bn(x))
  float* wpartial;       // [workgroups][9 * 4096 + 64]
  // Round 6: the data gradient this kernel writes is dA of the PREVIOUS layer's BatchNorm + ReLU (x is that layer's raw output), and the
  // tile that writes it holds relu(bn(x)) of the same 128 positions in LDS (the weight gradient's operand) — so the flush also leaves
  // the two BatchNorm-backward sums of that layer,  sum dz  and  sum dz * xhat  (dz = dA where relu(bn(x)) > 0; there the activation
  // IS gamma * xhat + beta, so xhat follows from it), as partial records for srlz_bn_bwd_finalize_partials: the separate pass of
  // srlz_bn_relu_bwd_sums over (x, dA) — 0.8 GB at the 55 x 55 layer — disappears.  bnpart: [groups][bn_rows][128] floats, rows
  // 4 * tile + (wave & 3) of a group from this kernel (channels whose BatchNorm scale is (almost) 0 contribute 0 here: xhat cannot be
  // recovered from the activation — the rows behind them come from conv64_bnpart_zero_scale_kernel); NULL = off.
  float* bnpart;
  int bn_rows;           // records per BatchNorm group
};

// rows per thread the second / fourth class of a tile need (gather_request<NJ>): their taps reach at most 1 / 0 positions ahead
// (fused_bwd_ok checks it: build_program puts the 2-tap class {0, +1} of a stride-2 ConvTranspose's data gradient second, the 1-tap class {0} last)
constexpr int FB_NJ1 = 5, FB_NJ3 = 4;
constexpr int FB_REACH1 = FB_NJ1 * GP_RP - TM, FB_REACH3 = FB_NJ3 * GP_RP - TM;  // 32 and 0 positions

struct YRows { f32x4 v[4]; unsigned ok; };  // a thread's share of the tile's 128 rows of y_prev (ytile_row)

// The a-tile is WAVE-PRIVATE between its landing and the flush that reads it back (round 6): wave (wrow = wave & 3, wcol = wave >> 2)
// requests, lands and — in the flush, for the BatchNorm-backward sums of the layer that produced y_prev — re-reads rows
// 32 wrow + 8 j + (lane >> 3), j = 0..3, channels 32 wcol + 4 (lane & 7) ..: exactly the block of the data gradient it flushes.  So a
// wave may read its block back BEHIND the tile's closing barrier and land the next tile's block over it without another barrier
// (every other reader of the a-tile — the weight-gradient steps of all waves — sits between the tap barriers).
// ... and the table of the tile's own 128 positions in the low-resolution tensor (y_prev): entry = pixel index << 1 | 1, 0 = outside;
// row R at ((R >> 5) * 8 + (R & 7)) * 4 + ((R >> 3) & 3): one 16-byte read per thread.  Built by threads [256, 384).
constexpr int YT_WORDS = GP_RP * 4;
__device__ __forceinline__ void ytab_build(unsigned* __restrict__ tab, const ConvProg& P, int q0, bool live) {
  int R = (int)threadIdx.x - 256;
  asm volatile("" : "+v"(R));
  if ((unsigned)R < (unsigned)YT_WORDS) {
    const GridPix g = grid_pix<false>(P, q0 + R, 1);
    const bool ok = live && g.n < P.N && g.y < P.Hd && g.x < P.Wd;
    tab[((R >> 5) * 8 + (R & 7)) * 4 + ((R >> 3) & 3)] = ok ? pix_entry(g.n, g.y, g.x, P.Hd, P.Wd) : 0u;
  }
}

__device__ __forceinline__ void ytile_request(YRows& r, const float* __restrict__ x, const unsigned* __restrict__ tab) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int lane = t & 63, wave = t >> 6;
  const int col = (wave >> 2) * 32 + (lane & 7) * 4;
  const uint4 q = *(const uint4*)(tab + ((wave & 3) * 8 + (lane >> 3)) * 4);
  const unsigned e[4] = {q.x, q.y, q.z, q.w};
  unsigned okmask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r.v[j] = *(const f32x4*)(x + ((e[j] >> 1) << 6) + col);  // (a row outside reads pixel 0; zeroed when it lands)
    okmask |= (e[j] & 1u) << j;
  }
  r.ok = okmask;
}

// xrec: [2][64] in LDS — scale, shift of the previous layer's BatchNorm for the tile's group
__device__ __forceinline__ void ytile_land(float* __restrict__ Ys, YRows& r, const float* __restrict__ xrec) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int lane = t & 63, wave = t >> 6;
  const int col = (wave >> 2) * 32 + (lane & 7) * 4;
  const int row0 = (wave & 3) * 32 + (lane >> 3);
  const f32x4 sc4 = *(const f32x4*)(xrec + col), sh4 = *(const f32x4*)(xrec + 64 + col);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool ok = (r.ok >> j) & 1u;
    f32x4 v = r.v[j];
    {
      const f32x4 z4 = __builtin_elementwise_fma(v, sc4, sh4);  // (v_pk_fma_f32; each element the same IEEE fma as before)
      const float hi = ok ? __builtin_inff() : 0.f;              // relu, and 0 for a row outside the tensor: one v_med3 per element
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(z4[e], 0.f, hi);
    }
    *(f32x4*)(Ys + (row0 + 8 * j) * 64 + col) = v;
  }
}

// the landing of a class's rows: BatchNorm + ReLU backward rebuilt from (dA, y), zero outside the tensor; bs4 += the tile's own rows (every dy element belongs to exactly one tile's range)
template <int NJ = GP_BATCH>
__device__ __forceinline__ void gather_land_sum(float* __restrict__ lds, GatherRows& r, int nrows, const float* __restrict__ lrec,
                                                f32x4& bs4) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int slot = t & 15;
  const f32x4 sc4 = *(const f32x4*)(lrec + slot * 4), sh4 = *(const f32x4*)(lrec + 64 + slot * 4);
  const f32x4 c0 = *(const f32x4*)(lrec + 128 + slot * 4), c1 = *(const f32x4*)(lrec + 192 + slot * 4);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {  // (rows 32 NJ .. of the buffer keep an earlier class's values: this class's taps never read them)
    const int R = (t >> 4) + GP_RP * j;
    const bool ok = (r.ok >> j) & 1u;
    f32x4 v = r.v[j];
    const f32x4 yy = r.yv[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // (scalar on purpose: the packed form needs aligned register pairs, and conv64_bwd_fused_kernel — at
      // its 256-register limit — spills 14 registers with it instead of 4)
      const float z = __builtin_fmaf(yy[e], sc4[e], sh4[e]);
      const float dz = z > 0.f ? v[e] : 0.f;
      v[e] = ok ? __builtin_fmaf(sc4[e], dz, -__builtin_fmaf(c1[e], yy[e], c0[e])) : 0.f;
    }
    if (j < GP_CORE) bs4 += v;  // (min_off == 0: rows [0, TM) are the tile's own; rows outside the tensor are zero)
    if (R < nrows) *(f32x4*)(lds + R * 64 + ((slot ^ (R & 15)) << 2)) = v;
  }
}

// NJJ k-groups (jj0 .. jj0 + NJJ - 1) of one tap's weight gradient for NB (1 or 2) column quadrants sharing the row quadrant mi:
// acc[b] += a-tile[p][32 mi ..]^T . dy[p + off][32 (nj0 + b) ..]  over p = 16 i + jj + 8 h.
template <int NB, int NJJ>
__device__ __forceinline__ void wgrad_steps(f32x16 (&acc)[NB], const float* __restrict__ Ys, const float* __restrict__ Ac, int off,
                                            int mi, int nj0, int jj0, int h, int l31) {
#pragma unroll
  for (int q = 0; q < NJJ; ++q) {
    const int jj = jj0 + q;
    const float* ap = Ys + (jj + 8 * h) * 64 + mi * 32 + l31;
    const int Rj = jj + 8 * h + off, key = Rj & 15;
    const float* bp[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int co = (nj0 + b) * 32 + l31;
      bp[b] = Ac + Rj * 64 + ((((co >> 2) ^ key) << 2) | (co & 3));
    }
#pragma unroll
    for (int i0 = 0; i0 < 8; i0 += 4) {  // (four k-steps at a time: the fragments of eight would cost 12 more registers)
      float av[4], bv[NB][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = ap[(i0 + i) * 1024];
#pragma unroll
        for (int b = 0; b < NB; ++b) bv[b][i] = bp[b][(i0 + i) * 1024];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[b][i], acc[b], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(GP_THREADS, 2) void conv64_bwd_fused_kernel(const float* __restrict__ src_all,
                                                                        const float* __restrict__ wpack,
                                                                        float* __restrict__ dst_all, const ConvProg P, int ntiles,
                                                                        const OpFuse fuse_all, const FusedBwd fb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nrows = TM + P.span;
  constexpr int nrows1 = TM + FB_REACH1;    // what the short-reach classes (second, fourth) can touch of their buffer
  float* As0 = (float*)smem;                // class rows, double-buffered: classes 0 / 2 here (TM + span rows),
  float* As1 = As0 + nrows * 64;            // classes 1 / 3 here (TM + 32 rows)
  float* Ys = As1 + nrows1 * 64;            // [TM][64]: relu(bn(y_prev)) of the tile's positions
  float* Bs0 = Ys + TM * 64;                // 2 x (64 x 64): the weight slabs of the current tap and of the next one (round 6: the slab of
                                            // tap t + 1 is written WHILE tap t runs, so a tap needs one barrier, not two)
  int* rowinfo = (int*)(Bs0 + 2 * 4096);    // [2 (tile parity)][3][TM]
  float* frec = (float*)(rowinfo + 6 * TM); // [G <= 2][4][64]: scale, shift, c0, c1 of this layer's BatchNorm backward
  float* xrec = frec + 512;                 // [G <= 2][2][64]: scale, shift of the previous layer's BatchNorm
  unsigned* gtab = (unsigned*)(xrec + 256); // row tables of the tile whose rows are being requested: source side (gtab_build)
  unsigned* ytab = gtab + GT_WORDS;         // ... and its own 128 positions in y_prev (ytab_build)
  float* prec = (float*)(ytab + YT_WORDS);  // [G <= 2][3][64]: pA, pB, threshold — xhat = a * pA + pB where a = relu(bn(x)) > threshold

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wrow = wave & 3, wcol = wave >> 2;
  const int cls0 = P.tsrc[0], cls1 = P.tsrc[4], cls2 = P.tsrc[6], cls3 = P.tsrc[8];
  // weight-gradient assignment of this wave (wave-uniform)
  const int wmi = wave & 1, wnj = (wave >> 1) & 1, wk = wave >> 2;
  const int tap_c0 = wave >> 1, tap_c1 = 4 + wk, tap_c2 = 6 + wk;
  const int off_c0 = P.toff[tap_c0], off_c1 = P.toff[tap_c1], off_c2 = P.toff[tap_c2], off_c3 = P.toff[8];

  const int xcd = blockIdx.x & 7, wi = blockIdx.x >> 3, wpx = gridDim.x >> 3;
  const int tq = ntiles >> 3, tr = ntiles & 7;
  const int tbase = (xcd < tr) ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
  const int tcnt = tq + (xcd < tr ? 1 : 0);

  if (tid < 64 * P.G) {
    const int g = tid >> 6, c = tid & 63;
    const float* bnp = fuse_all.bnp + g * 256;
    const float* sums = fuse_all.sums + g * 128;
    const float sc = bnp[128 + c], sh = bnp[192 + c];
    float c0 = 0.f, c1 = 0.f;
    if (fuse_all.training) {
      c1 = sc * bnp[64 + c] * sums[64 + c] * fuse_all.inv_count;
      c0 = sc * sums[c] * fuse_all.inv_count - c1 * bnp[c];
    }
    float* fr = frec + g * 256;
    fr[c] = sc; fr[64 + c] = sh; fr[128 + c] = c0; fr[192 + c] = c1;
    xrec[g * 128 + c] = fb.x_bnp[g * 256 + 128 + c];
    xrec[g * 128 + 64 + c] = fb.x_bnp[g * 256 + 192 + c];
    {  // a = scale * x + shift = gamma * xhat + beta  =>  xhat = a * (invstd / scale) - (shift / scale + mean) * invstd; a channel whose
       // |scale| is tiny against |shift| (exactly 0 included) would lose xhat in the cancellation: it contributes nothing here
       // (threshold +inf) and is summed by conv64_bnpart_zero_scale_kernel from x itself (cf. the pooled-block epilogue, PSUM)
      const float xmean = fb.x_bnp[g * 256 + c], xinv = fb.x_bnp[g * 256 + 64 + c];
      const float xsc = fb.x_bnp[g * 256 + 128 + c], xsh = fb.x_bnp[g * 256 + 192 + c];
      const bool zero = bnpart_zero_scale(xsc, xsh);
      const float isc = zero ? 0.f : 1.f / xsc;
      prec[g * 192 + c] = xinv * isc;
      prec[g * 192 + 64 + c] = -(xsh * isc + xmean) * xinv;
      prec[g * 192 + 128 + c] = zero ? __builtin_inff() : 0.f;
    }
  }

  constexpr int BV = 1024 / GP_THREADS;
  f32x4 breg[BV];
  {
    const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[0] * 4096);
#pragma unroll
    for (int i = 0; i < BV; ++i) breg[i] = wsrc[wave * (BV * 64) + lane + i * 64];
  }
  const unsigned dst_bytes = (unsigned)P.dst_gstride * 4u;
  const __amdgpu_buffer_rsrc_t bnbuf = raw_buffer(fb.bnpart, fb.bnpart ? (unsigned)(P.G * fb.bn_rows) * 512u : 0u);

  f32x16 aw0[2], aw1[1], aw2[1], aw3[1];  // weight-gradient accumulators of the four classes
#pragma unroll
  for (int r = 0; r < 16; ++r) { aw0[0][r] = 0.f; aw0[1][r] = 0.f; aw1[0][r] = 0.f; aw2[0][r] = 0.f; aw3[0][r] = 0.f; }
  f32x4 bs4 = {0.f, 0.f, 0.f, 0.f};  // bias gradient: column sums of the tile's own dy rows (channels 4 slot .. of this thread's rows)

  GatherRows rr;
  YRows yr;
  int k = wi;
  int parity = 0;
  if (k < tcnt) {  // the first tile's class 0 and a-tile are staged the plain way
    const int tile = tbase + k;
    const int grp = (P.G > 1 && tile >= P.tpg) ? 1 : 0;
    const int q0 = (tile - grp * P.tpg) * TM;
    gtab_build<false>(gtab, P, q0, nrows);
    ytab_build(ytab, P, q0, true);
    __syncthreads();  // the tables, frec and xrec are complete
    gather_request(rr, src_all + grp * P.src_gstride, fuse_all.y + grp * P.src_gstride, gtab, cls0, P.Ws);
    ytile_request(yr, fb.x + grp * P.dst_gstride, ytab);
    gather_land_sum(As0, rr, nrows, frec + grp * 256, bs4);
    ytile_land(Ys, yr, xrec + grp * 128);
  }
  // The slab of the first tile's tap 0 goes to slab buffer 0 now (published by that tap's barrier) and tap 1's is requested: from here
  // on tap t writes the slab of tap t + 1 into the buffer tap t - 1 read, so a tap needs ONE barrier — the one that says "everybody is
  // done with tap t - 1" — instead of two (until round 6: slab write and landings sat between two barriers, with every matrix pipe idle)
  // Tap t reads slab buffer t & 1 (compile-time); a tile has nine taps, so its last tap and the next tile's first both read buffer 0:
  // tap 8 writes no slab, the next tile's first slab is written behind the tile's closing barrier instead.
  {
    f32x4* wdst = (f32x4*)Bs0;
#pragma unroll
    for (int i = 0; i < BV; ++i) wdst[wave * (BV * 64) + lane + i * 64] = breg[i];
    const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[1] * 4096);
#pragma unroll
    for (int i = 0; i < BV; ++i) breg[i] = wsrc[wave * (BV * 64) + lane + i * 64];
  }
  for (; k < tcnt; k += wpx, parity ^= 1) {
    const int tile = tbase + k;
    const int grp = (P.G > 1 && tile >= P.tpg) ? 1 : 0;
    const int q0 = (tile - grp * P.tpg) * TM;
    const float* __restrict__ src = src_all + grp * P.src_gstride;
    const float* __restrict__ ysrc = fuse_all.y + grp * P.src_gstride;
    const __amdgpu_buffer_rsrc_t dst = raw_buffer(dst_all + grp * P.dst_gstride, dst_bytes);
    const float* lrec = frec + grp * 256;
    const int k2 = k + wpx;
    const bool more = k2 < tcnt;
    const int tile2 = tbase + (more ? k2 : k);
    const int grp2 = (P.G > 1 && tile2 >= P.tpg) ? 1 : 0;
    const int q02 = (tile2 - grp2 * P.tpg) * TM;
    int* ri = rowinfo + parity * (3 * TM);
    if (tid < TM) {
      const int q = q0 + tid;
      int n = -1, ya = 0, xb = 0;
      if (q < P.total_q) {  // (grid_pix written out: through the helper hipcc orders this kernel's scalar loads differently — three
        // instructions more in a kernel at its register limit; the generated code is kept as it was)
        n = fastdiv(q, P.mPHW, P.sPHW);
        const int rem = q - n * P.PHW;
        const int a = fastdiv(rem, P.mPW, P.sPW);
        ya = a * P.ds;
        xb = (rem - a * P.PW) * P.ds;
      }
      ri[tid] = n; ri[TM + tid] = ya; ri[2 * TM + tid] = xb;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // (one opaque copy of the lane index per tile: see conv64_gather_pipe_kernel)
    int lane_t = lane;
    asm volatile("" : "+v"(lane_t));
    const int h_t = lane_t >> 5, l31_t = lane_t & 31;
    const int arow0 = wrow * 32 + l31_t;
    const int brow_off = (wcol * 32 + l31_t) * 64;
    const int bkey = lane_t & 15;
    const int bslot_t = wave * (BV * 64) + lane_t;

#pragma unroll
    for (int ti = 0; ti < NTAPS; ++ti) {
      // class of this tap and the LDS buffer that holds it (compile-time after unrolling)
      const float* Ac = (ti < 4 || ti == 6 || ti == 7) ? As0 : As1;
      const float* Bcur = Bs0 + (ti & 1) * 4096;
      float* Bnext = Bs0 + ((ti + 1) & 1) * 4096;
      // ONE barrier per tap: every wave has finished tap ti - 1, so the slab buffer that tap read (Bnext) and the class buffer that is
      // about to be refilled are free, and this tap's slab (written during tap ti - 1) and the rows landed meanwhile are visible.
      // Everything up to the MFMAs below runs per wave, un-synchronised: a wave that is done landing starts its matrix work while its
      // neighbours are still landing.
      __syncthreads();
      if (ti < NTAPS - 1) {
        f32x4* wdst = (f32x4*)Bnext;  // the slab of tap ti + 1
#pragma unroll
        for (int i = 0; i < BV; ++i) wdst[bslot_t + i * 64] = breg[i];
        // ... and the request for the one after it (behind tap 7: tap 0 of the next tile — same weights — which is written behind the
        // tile's closing barrier)
        const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[(ti + 2) % NTAPS] * 4096);
#pragma unroll
        for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot_t + i * 64];
      }
      // rows requested two taps ago land now (the in-order vmcnt has completed them with the slab just written): class 1 -> As1
      // while taps 2, 3 still read class 0 in As0; class 2 -> As0 once class 0 is done; class 3 -> As1; the next tile's class 0 -> As0.
      // (Two barriers — those of taps ti + 1 and ti + 2 — lie between a landing and the first tap that reads it.)
      if (ti == 2) gather_land_sum<FB_NJ1>(As1, rr, nrows1, lrec, bs4);
      if (ti == 4) gather_land_sum(As0, rr, nrows, lrec, bs4);
      if (ti == 6) gather_land_sum<FB_NJ3>(As1, rr, nrows1, lrec, bs4);
      if (ti == 8) gather_land_sum(As0, rr, nrows, frec + grp2 * 256, bs4);  // (past the last tile: every row masked off -> zeros; no
                                                                             // run-time branch around a landing, or its join costs a full vmcnt(0))
      // the NEXT tile's row tables, between the last request of this tile (tap 4) and the first of the next (tap 6) — the barriers of
      // taps 5 and 6 fence both sides; past the end: no rows -> every entry 0 -> every row reads pixel 0 and is dropped
      if (ti == 5) { gtab_build<false>(gtab, P, q02, more ? nrows : 0); ytab_build(ytab, P, q02, more); }
      if (ti == 0) gather_request<FB_NJ1>(rr, src, ysrc, gtab, cls1, P.Ws);
      if (ti == 2) gather_request(rr, src, ysrc, gtab, cls2, P.Ws);
      if (ti == 4) gather_request<FB_NJ3>(rr, src, ysrc, gtab, cls3, P.Ws);
      if (ti == 6) gather_request(rr, src_all + grp2 * P.src_gstride, fuse_all.y + grp2 * P.src_gstride, gtab, cls0, P.Ws);
      if (ti == 8) ytile_request(yr, fb.x + grp2 * P.dst_gstride, ytab);
      __builtin_amdgcn_sched_barrier(0);
      {  // ---- data gradient: 32 positions x 32 channels of this wave
        const int R = arow0 + P.toff[ti];
        int abase = (R * 64 + ((h_t ^ (R & 15)) << 2)) * 4;
        asm volatile("" : "+v"(abase));
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          const f32x4 a = *(const f32x4*)((const char*)Ac + (abase ^ (kc << 5)));
          const f32x4 b = *(const f32x4*)(Bcur + brow_off + (((kc * 2 + h_t) ^ bkey) << 2));
#pragma unroll
          for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[r], acc, 0, 0, 0);
        }
      }
      // ---- weight gradient: this wave's share of the class that is resident during this tap period
      // (the lane index opaque once more, per tap: the operand addresses of all nine taps are tile-invariant functions of it, and
      // computed early and kept they cost more registers than there are)
      int lane_p = lane_t;
      asm volatile("" : "+v"(lane_p));
      const int h_p = lane_p >> 5, l31_p = lane_p & 31;
      if (ti < 4) wgrad_steps<2, 2>(aw0, Ys, As0, off_c0, wmi, 0, 2 * ti, h_p, l31_p);
      else if (ti < 6) wgrad_steps<1, 4>(aw1, Ys, As1, off_c1, wmi, wnj, 4 * (ti - 4), h_p, l31_p);
      else if (ti < 8) wgrad_steps<1, 4>(aw2, Ys, As0, off_c2, wmi, wnj, 4 * (ti - 6), h_p, l31_p);
      else wgrad_steps<1, 4>(aw3, Ys, As1, off_c3, wmi, wnj, 4 * wk, h_p, l31_p);
    }
    __syncthreads();  // every wave is done with the last tap's slab (buffer 0), with class 3 and with the a-tile
    {  // the next tile's first slab -> buffer 0, its second requested (cf. the prologue)
      f32x4* wdst = (f32x4*)Bs0;
#pragma unroll
      for (int i = 0; i < BV; ++i) wdst[bslot_t + i * 64] = breg[i];
      const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[1] * 4096);
#pragma unroll
      for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot_t + i * 64];
    }
    {  // flush of the data gradient (see conv64_gather_pipe_kernel) through this wave's own 2 KB of slab buffer 1 (tap 7 was its last
       // reader).  Round 6: the lane that stores four channels of a position also reads relu(bn(x)) of the same four out of the a-tile —
       // this wave's own block of it (ytile_request), so no barrier is needed before the next tile's block lands over it below — for the
       // BatchNorm-backward sums of the layer that produced x (FusedBwd::bnpart): s = sum of dA where a > 0, q = sum of dA * a (a is 0
       // where the ReLU is closed and outside the tensor, so q needs no mask); sum dz * xhat = pA q + pB s per lane.
      float* S = Bs0 + 4096 + wave * 512;
      const int eg = lane_t >> 3, eslot = lane_t & 7;
      const int cbase = wcol * 32 + eslot * 4;  // this lane's four channels
      const f32x4 pT = *(const f32x4*)(prec + grp * 192 + 128 + cbase);
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int rq = 0; rq < 8; ++rq) {
          const int rowl = (rq & 3) + 8 * (rq >> 2) + 4 * h_t;
          S[rowl * 32 + l31_t] = acc[8 * half + rq];
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int rowl = eg + 8 * kk;
          const int row = wrow * 32 + 16 * half + rowl;
          const f32x4 v = *(const f32x4*)(S + rowl * 32 + eslot * 4);
          const f32x4 av = *(const f32x4*)(Ys + row * 64 + cbase);  // relu(bn(x)) of the position; 0 outside the tensor
          const int n = ri[row];
          const int y = ri[TM + row], x = ri[2 * TM + row];
          const bool inside = n >= 0 && y < P.Hd && x < P.Wd;
          __builtin_amdgcn_raw_buffer_store_b128(v, dst, inside ? (unsigned)((n * P.Hd + y) * P.Wd + x) * 256u + wcol * 128 + eslot * 16 : GP_DROP,
                                                 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s4[e] += av[e] > pT[e] ? v[e] : 0.f;
            q4[e] = __builtin_fmaf(v[e], av[e], q4[e]);
          }
        }
      }
      {
        const f32x4 pA = *(const f32x4*)(prec + grp * 192 + cbase), pB = *(const f32x4*)(prec + grp * 192 + 64 + cbase);
#pragma unroll
        for (int e = 0; e < 4; ++e) q4[e] = __builtin_fmaf(pA[e], q4[e], pB[e] * s4[e]);
      }
      // this wave's 32 rows = the eight row groups (lane bits 3-5) of the eight sums, as a transposing butterfly (gfx950's
      // v_permlane32_swap / v_permlane16_swap: one add folds a lane bit of TWO values): 14 vector instructions instead of 24 ds_bpermute + 24
      // adds, fixed order.  Afterwards lane L holds channel 4 eslot + {0, 2, 1, 3}[L >> 4] of s (in s4[0]) and of q (in q4[0]); the lanes
      // with bit 3 clear leave the wave's half of record 4 * tile + wrow (branch-free: the other lanes — and every lane when bnpart is
      // NULL, a zero-sized buffer — store out of range)
      {
        const float u0 = fold32(s4[0], s4[1]), u1 = fold32(s4[2], s4[3]), u2 = fold32(q4[0], q4[1]), u3 = fold32(q4[2], q4[3]);
        float w0 = fold16(u0, u1), w1 = fold16(u2, u3);
        w0 += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(w0), 0x128 /* row_ror:8 */, 0xf, 0xf, false));
        w1 += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(w1), 0x128, 0xf, 0xf, false));
        const int erow = lane_t >> 4;
        const unsigned rec = (unsigned)(grp * fb.bn_rows + 4 * (tile - grp * P.tpg) + wrow) * 512u +
                             (unsigned)(cbase + ((erow & 1) << 1) + (erow >> 1)) * 4u;
        const bool mine = (lane_t & 8) == 0;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(w0), bnbuf, mine ? rec : GP_DROP, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(w1), bnbuf, mine ? rec + 256u : GP_DROP, 0, 0);
      }
    }
    ytile_land(Ys, yr, xrec + grp2 * 128);  // (past the last tile: zeros)
  }

  // ---- the workgroup's weight-gradient partial [9 (reference tap index)][64 ci][64 co] and bias partial [64]
  __syncthreads();  // (everything in LDS is dead from here on)
  {
    const int h = lane >> 5, l31 = lane & 31;
    float* out = fb.wpartial + (size_t)blockIdx.x * WGRAD_PARTIAL_FLOATS;
    auto put = [&](const f32x16& a, int tap, int mi, int nj) {
      float* o = out + (size_t)P.tw[tap] * 4096;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[(mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 64 + nj * 32 + l31] = a[r];
    };
    put(aw0[0], tap_c0, wmi, 0);
    put(aw0[1], tap_c0, wmi, 1);
    put(aw1[0], tap_c1, wmi, wnj);
    put(aw2[0], tap_c2, wmi, wnj);
    // tap 8: the two position halves (waves w and w + 4) are added through LDS
    float* X = As0;  // [4 quadrants][16 regs][64 lanes]
    if (wk == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) X[((wave & 3) * 16 + r) * 64 + lane] = aw3[0][r];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) aw3[0][r] += X[((wave & 3) * 16 + r) * 64 + lane];
      put(aw3[0], 8, wmi, wnj);
    }
    __syncthreads();
    float* red = As0;  // [32 row groups][64 channels]
    *(f32x4*)(red + (tid >> 4) * 64 + (tid & 15) * 4) = bs4;
    __syncthreads();
    if (tid < 64) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < GP_RP; ++r) t += red[r * 64 + tid];
      out[NTAPS * 4096 + tid] = t;
    }
  }
}

// Companion of conv64_bwd_fused_kernel's BatchNorm-backward records (FusedBwd::bnpart): the channels whose BatchNorm scale is (almost)
// 0 — xhat cannot be recovered from relu(bn(x)) there — summed from x itself, as srlz_bn_relu_bwd_sums does for every channel, into
// the BNZ_BLOCKS records behind the fused kernel's.  A group without such a channel (the normal case) costs one ~4 us launch that
// writes zero records; with one, this is a pass over (x, dA): rare, and slow on purpose.
constexpr int BNZ_BLOCKS = 64;
__global__ __launch_bounds__(256) void conv64_bnpart_zero_scale_kernel(const float* __restrict__ x, const float* __restrict__ x_bnp,
                                                                      const float* __restrict__ da, float* __restrict__ bnpart,
                                                                      long long pixels, int bn_rows, int first_row) {
  const int g = blockIdx.y;  // BatchNorm group; pixels = positions of ONE group
  x_bnp += g * 256;
  x += (size_t)g * pixels * 64;
  da += (size_t)g * pixels * 64;
  const int c4 = threadIdx.x & 15;
  const auto [mean, invstd, sc, sh] = load_bn_quads(x_bnp, c4);
  unsigned zmask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) zmask |= (bnpart_zero_scale(sc[j], sh[j]) ? 1u : 0u) << j;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  if (__syncthreads_or(zmask != 0)) {
    for (long long pix = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); pix < pixels; pix += (long long)gridDim.x * 16) {
      const f32x4 v = *(const f32x4*)(x + pix * 64 + c4 * 4);
      const f32x4 d = *(const f32x4*)(da + pix * 64 + c4 * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (((zmask >> j) & 1u) && v[j] * sc[j] + sh[j] > 0.f) {
          s1[j] += (double)d[j];
          s2[j] += (double)(d[j] * ((v[j] - mean[j]) * invstd[j]));
        }
    }
  }
  bn_bwd_combine_store(s1, s2, bnpart + ((size_t)g * bn_rows + first_row + blockIdx.x) * 128);
}

// ---------------------------------------------------------------------------------------------------------------
// The stride-2 SCATTER programs — the forward of a ConvTranspose2d(64, 64, 3, stride 2): one source class, four destination classes
// with 4 / 2 / 2 / 1 taps — persistent and software-pipelined.  conv64_fwd_kernel<4, false> runs such a tile as: row table, rowinfo,
// ONE synchronous staging of the 128 + span source rows (an HBM round trip between two barriers, with the fused relu(bn(.)) of the
// previous block on the way in), nine taps through a run-time class switch (zeroing of 32 accumulator registers per class, a flush
// with an exec branch around each 16-byte store).  Here
//  * workgroups are persistent (2 per CU) and walk their XCD's run of tiles; the NEXT tile's row table is built under tap 6, its rows
//    are requested into registers behind the barrier that opens tap 7 (branch-free: clamped addresses, masks applied at the landing)
//    and land in LDS — through the same relu(bn(.)) expression, rows outside the tensor as zeros — behind the barrier that closes
//    tap 8; tap 0's slab of the next tile travels under tap 8;
//  * the tap structure is compile-time ({0..3}, {4, 5}, {6, 7}, {8}): no class switch, and the first MFMA of a class takes C = 0
//    instead of 32 zeroed registers;
//  * the flush is branch-free: a lane that must not write stores out of its buffer's range (GP_DROP).
// The wave tile stays conv64_fwd_kernel's — 4 waves of 32 rows x 64 channels, NOT the 8 waves of 32 x 32 of the gather kernels above:
// a tile's BatchNorm partial is one sequential chain per lane (channels 4 (lane & 15) .., rows (lane >> 4) + 4 k of each 16-row
// half, class after class); a wave of 32 x 32 has only 32 such chains, so half its lanes would idle through twice as many flush
// instructions per MFMA, or every flushed value would first have to move to the lane that owns its chain.  Same tiles, same MFMAs
// in the same order, same flush layout, same summation order: y AND stats_partial are bit-identical to conv64_fwd_kernel<4, false>'s.
// ---------------------------------------------------------------------------------------------------------------
constexpr int SP_THREADS = 256;
constexpr int SP_RP = SP_THREADS / 16;   // rows per pass
constexpr int SP_BATCH = 12;             // rows (of 16 lanes) per thread: 128 + span <= 192
constexpr int ST_WORDS = SP_RP * SP_BATCH;

struct ScatterRows {
  f32x4 v[SP_BATCH];
  unsigned ok;  // bit j: row j lies inside the tensor
};

// The source-side row table of a scatter tile (cf. gtab_build): row R at (R & 15) * SP_BATCH + (R >> 4) — the twelve rows of thread t
// (R = (t >> 4) + 16 j) are consecutive words.  The staged range begins at q0 + min_off < q0: built SHIFTED.
__device__ __forceinline__ void stab_build(unsigned* __restrict__ tab, const ConvProg& P, int qstart, int nrows) {
  int R = threadIdx.x;
  asm volatile("" : "+v"(R));
  if (R < ST_WORDS) {
    unsigned e = 0;
    if (R < nrows) e = src_entry<true>(P, qstart + R, P.ss);
    tab[(R & (SP_RP - 1)) * SP_BATCH + (R >> 4)] = e;
  }
}

__device__ __forceinline__ void scatter_request(ScatterRows& r, const float* __restrict__ src, const unsigned* __restrict__ tab) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int slot = t & 15;
  const unsigned* __restrict__ tp = tab + (t >> 4) * SP_BATCH;
  const uint4 e0 = *(const uint4*)tp, e1 = *(const uint4*)(tp + 4), e2 = *(const uint4*)(tp + 8);
  const unsigned e[SP_BATCH] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w};
  static_assert(SP_BATCH == 12, "the table read above takes twelve rows");
  unsigned okmask = 0;
#pragma unroll
  for (int j = 0; j < SP_BATCH; ++j) {
    // the one source class of a scatter program is class 0 (bit 0 of the entry); any row outside reads pixel 0 and lands as zeros
    const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)e[j], 0u, 1u);
    const unsigned off = (((e[j] >> 4) << 6) & m) + slot * 4;
    r.v[j] = *(const f32x4*)(src + off);
    okmask |= m & (1u << j);
  }
  r.ok = okmask;
}

// lrec (FUSE): scale, shift of the tile's BatchNorm group in LDS — relu(bn(raw)) as stage_rows_tab has it: hipcc contracts that one's
// v * scale + shift into a fused multiply-add everywhere; written out here, because contraction is the compiler's choice per site
template <bool FUSE>
__device__ __forceinline__ void scatter_land(float* __restrict__ lds, ScatterRows& r, int nrows, const float* __restrict__ lrec) {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int slot = t & 15;
  f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (FUSE) { sc4 = *(const f32x4*)(lrec + slot * 4); sh4 = *(const f32x4*)(lrec + 64 + slot * 4); }
#pragma unroll
  for (int j = 0; j < SP_BATCH; ++j) {
    const int R = (t >> 4) + SP_RP * j;
    const bool ok = (r.ok >> j) & 1u;
    f32x4 v = r.v[j];
    if constexpr (FUSE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float z = __builtin_fmaf(v[e], sc4[e], sh4[e]); v[e] = z > 0.f ? z : 0.f; }
    }
    if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (j < TM / SP_RP || R < nrows) *(f32x4*)(lds + R * 64 + ((slot ^ (R & 15)) << 2)) = v;
  }
}

// One destination class d = (dy << 1) | dx of the tile leaves (conv64_fwd_kernel's flush16, branch-free): through the wave's own 4 KB of
// the idle slab, 16 tile rows at a time; lane (eg = lane >> 4, eslot = lane & 15) stores channels 4 eslot .. of rows eg + 4 k.
__device__ __forceinline__ void scatter_flush(const f32x16 (&acc)[2], const float (&bcol)[2], float* __restrict__ S,
                                              const float* __restrict__ zero4, const int* __restrict__ ri,
                                              const __amdgpu_buffer_rsrc_t dst, int d, int Wd, f32x4& s4, f32x4& q4) {
  int tid_f = threadIdx.x;
  asm volatile("" : "+v"(tid_f));
  const int lane = tid_f & 63, wrow = tid_f >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int need = d >> 1 | (d & 1) << 1;  // the rowinfo bits this class needs: the row below / the column to the right exists
  const unsigned ddelta = (unsigned)((d >> 1) * Wd + (d & 1));
  const int eg = lane >> 4, eslot = lane & 15;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int rowl = (rr & 3) + 8 * (rr >> 2) + 4 * h;
      const int swz = (rowl & 4) << 3;  // 32 for rows 4..7, 12..15 (their two 32-channel halves swapped: bank conflicts)
#pragma unroll
      for (int j = 0; j < 2; ++j) S[rowl * 64 + ((32 * j + l31) ^ swz)] = acc[j][8 * half + rr] + bcol[j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rowl = eg + 4 * k;
      const int row = wrow * 32 + 16 * half + rowl;
      const int w = ri[row];
      const bool inside = w >= 0 && (w & need) == need;
      // a lane whose position has no pixel of this class reads four zeros instead (one select on the address, not four on the value):
      // its store is dropped, and s + 0, fma(0, 0, q) leave the sums as they are, bit for bit (neither sum is ever -0)
      const f32x4 v = *(const f32x4*)(inside ? S + rowl * 64 + ((eslot ^ ((rowl & 4) << 1)) << 2) : zero4);
      __builtin_amdgcn_raw_buffer_store_b128(v, dst, inside ? ((unsigned)(w >> 2) + ddelta) * 256u + eslot * 16 : GP_DROP, 0, 0);
      // (conv64_fwd_kernel's q += v * v is a fused multiply-add at every site: written out, see scatter_land)
#pragma unroll
      for (int e = 0; e < 4; ++e) { s4[e] += v[e]; q4[e] = __builtin_fmaf(v[e], v[e], q4[e]); }
    }
  }
}

template <bool FUSE>
__global__ __launch_bounds__(SP_THREADS, 2) void conv64_scatter_pipe_kernel(const float* __restrict__ src_all,
                                                                           const float* __restrict__ wpack,
                                                                           const float* __restrict__ bias,
                                                                           float* __restrict__ dst_all,
                                                                           float* __restrict__ stats_partial, const ConvProg P,
                                                                           int ntiles, const float* __restrict__ bnp_all) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* As = (float*)smem;                 // (TM + span) x 64, swizzled: the tile's source rows
  float* Bs = As + (TM + P.span) * 64;      // 64 x 64 weight slab of the current tap; between taps: 4 KB of flush scratch per wave
  int* rowinfo = (int*)(Bs + 4096);         // [2 (tile parity)][TM]: destination word of a grid position (conv64_fwd_kernel's)
  unsigned* stab = (unsigned*)(rowinfo + 2 * TM);  // the source-side row table of the tile whose rows are being requested
  float* frec = (float*)(stab + ST_WORDS);  // [G <= 2][scale 64 | shift 64] of the fused operand
  float* red = frec + 256;                  // [4 row groups][sum 64 | sum of squares 64]: the tile's BatchNorm partials on their way out
  float* zero4 = red + 512;                 // four zeros (scatter_flush)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int nrows = TM + P.span;
  const int d0 = P.tdst[0], d1 = P.tdst[4], d2 = P.tdst[6], d3 = P.tdst[8];

  const int xcd = blockIdx.x & 7, wi = blockIdx.x >> 3, wpx = gridDim.x >> 3;
  const int tq = ntiles >> 3, tr = ntiles & 7;
  const int tbase = (xcd < tr) ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
  const int tcnt = tq + (xcd < tr ? 1 : 0);

  if (tid < 4) zero4[tid] = 0.f;  // (published by the barrier of the first staging)
  if constexpr (FUSE) {
    if (tid < 64 * P.G) {
      const int g = tid >> 6, c = tid & 63;
      frec[g * 128 + c] = bnp_all[g * 256 + 128 + c];
      frec[g * 128 + 64 + c] = bnp_all[g * 256 + 192 + c];
    }
  }
  float bcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bcol[j] = bias ? bias[j * 32 + (lane & 31)] : 0.f;

  constexpr int BV = 1024 / SP_THREADS;
  f32x4 breg[BV];
  {
    const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[0] * 4096);
#pragma unroll
    for (int i = 0; i < BV; ++i) breg[i] = wsrc[wave * (BV * 64) + lane + i * 64];
  }
  const unsigned dst_bytes = (unsigned)P.dst_gstride * 4u;

  ScatterRows rr;
  int k = wi;
  int parity = 0;
  if (k < tcnt) {  // the first tile's rows are staged the plain way
    const int tile = tbase + k;
    const int grp = (P.G > 1 && tile >= P.tpg) ? 1 : 0;  // (G <= 2, checked by the host)
    const int q0 = (tile - grp * P.tpg) * TM;
    stab_build(stab, P, q0 + P.min_off, nrows);
    __syncthreads();  // the table and frec are complete
    scatter_request(rr, src_all + grp * P.src_gstride, stab);
    scatter_land<FUSE>(As, rr, nrows, frec + grp * 128);
  }
  for (; k < tcnt; k += wpx, parity ^= 1) {
    const int tile = tbase + k;
    const int grp = (P.G > 1 && tile >= P.tpg) ? 1 : 0;
    const int q0 = (tile - grp * P.tpg) * TM;
    const __amdgpu_buffer_rsrc_t dst = raw_buffer(dst_all + grp * P.dst_gstride, dst_bytes);
    const int k2 = k + wpx;  // this workgroup's next tile (past the end: this one again, with no rows)
    const int tile2 = tbase + (k2 < tcnt ? k2 : k);
    const int grp2 = (P.G > 1 && tile2 >= P.tpg) ? 1 : 0;
    const int q02 = (tile2 - grp2 * P.tpg) * TM;
    int* ri = rowinfo + parity * TM;
    if (tid < TM) {  // (the other parity's copy may still be read by a wave that is flushing the previous tile)
      const int q = q0 + tid;
      int w = -1;
      if (q < P.total_q) {
        const GridPix g = grid_pix<false>(P, q, P.ds);
        if (g.y < P.Hd && g.x < P.Wd) w = (((g.n * P.Hd + g.y) * P.Wd + g.x) << 2) | (g.y + 1 < P.Hd ? 1 : 0) | (g.x + 1 < P.Wd ? 2 : 0);
      }
      ri[tid] = w;
    }
    f32x16 acc[2];
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
    int tid_t = tid;  // (one opaque copy of the thread index per tile: see conv64_gather_pipe_kernel)
    asm volatile("" : "+v"(tid_t));
    const int lane_t = tid_t & 63, wave_t = tid_t >> 6;
    const int h_t = lane_t >> 5, l31_t = lane_t & 31;
    const int arow0 = wave_t * 32 + l31_t - P.min_off;
    const float* brow = Bs + l31_t * 64;  // column tile j is 32 rows (2048 floats) further
    const int bkey = lane_t & 15;
    const int bslot_t = wave_t * (BV * 64) + lane_t;
    float* S = Bs + wave_t * 1024;

#pragma unroll
    for (int ti = 0; ti < NTAPS; ++ti) {
      constexpr f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const bool first = ti == 0 || ti == 4 || ti == 6 || ti == 8;  // this tap opens a destination class
      __syncthreads();  // all waves are done with the previous tap's Bs: until its slab write a wave's quarter of it is its scratch
      if (ti == 4) scatter_flush(acc, bcol, S, zero4, ri, dst, d0, P.Wd, s4, q4);
      if (ti == 6) scatter_flush(acc, bcol, S, zero4, ri, dst, d1, P.Wd, s4, q4);
      if (ti == 8) scatter_flush(acc, bcol, S, zero4, ri, dst, d2, P.Wd, s4, q4);
      {
        f32x4* wdst = (f32x4*)Bs;
#pragma unroll
        for (int i = 0; i < BV; ++i) wdst[bslot_t + i * 64] = breg[i];
      }
      {  // the next tap's slab (tap 0 of the next tile behind tap 8: same weights)
        const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[(ti + 1) % NTAPS] * 4096);
#pragma unroll
        for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot_t + i * 64];
      }
      if (ti == 6) stab_build(stab, P, q02 + P.min_off, k2 < tcnt ? nrows : 0);
      __syncthreads();
      if (ti == 7) scatter_request(rr, src_all + grp2 * P.src_gstride, stab);  // the rows of this workgroup's NEXT tile
      __builtin_amdgcn_sched_barrier(0);  // every request goes out HERE, ahead of the tap's MFMAs
      const int R = arow0 + P.toff[ti];
      int abase = (R * 64 + ((h_t ^ (R & 15)) << 2)) * 4;  // bytes; slot (2kc + h) ^ (R & 15) is this XOR (kc << 5)
      asm volatile("" : "+v"(abase));
      f32x4 a = *(const f32x4*)((const char*)As + abase);
      f32x4 b[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = *(const f32x4*)(brow + j * 2048 + ((h_t ^ bkey) << 2));
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        f32x4 an = a, bn[2] = {b[0], b[1]};
        if (kc < 7) {
          an = *(const f32x4*)((const char*)As + (abase ^ ((kc + 1) << 5)));
#pragma unroll
          for (int j = 0; j < 2; ++j) bn[j] = *(const f32x4*)(brow + j * 2048 + ((((kc + 1) * 2 + h_t) ^ bkey) << 2));
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ahead of this chunk's MFMAs
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[j][r], (first && kc == 0 && r == 0) ? zero16 : acc[j], 0, 0, 0);
        a = an;
        b[0] = bn[0]; b[1] = bn[1];
      }
    }
    __syncthreads();  // every wave is done with the last tap's slab and with As: Bs becomes scratch, As takes the next tile
    scatter_land<FUSE>(As, rr, nrows, frec + grp2 * 128);  // (past the last tile: every row masked off -> zeros)
    scatter_flush(acc, bcol, S, zero4, ri, dst, d3, P.Wd, s4, q4);
    if (stats_partial) {
      // conv64_fwd_kernel's order: the 4 row groups of a wave (lane bits 4, 5), then the 4 waves through LDS
      int tid_s = tid;
      asm volatile("" : "+v"(tid_s));
      const int lane_s = tid_s & 63, wrow_s = tid_s >> 6;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s4[e] += __shfl_xor(s4[e], 16, 64); s4[e] += __shfl_xor(s4[e], 32, 64);
        q4[e] += __shfl_xor(q4[e], 16, 64); q4[e] += __shfl_xor(q4[e], 32, 64);
      }
      if (lane_s < 16) {
        *(f32x4*)(red + wrow_s * 128 + lane_s * 4) = s4;
        *(f32x4*)(red + wrow_s * 128 + 64 + lane_s * 4) = q4;
      }
      __syncthreads();
      if (tid_s < 128) {
        const float v = red[tid_s] + red[128 + tid_s] + red[256 + tid_s] + red[384 + tid_s];
        stats_partial[(size_t)tile * 128 + tid_s] = v;  // [0,64): sum, [64,128): sum of squares
      }
    }
  }
}

}  // namespace

// ---- Which programs these kernels take ----
// conv64_gather_pipe_kernel takes a program when it is a stride-2 gather with the tap groups {4, 2, 2, 1}, at most two BatchNorm groups,
// a staged class of at most 192 rows (PW <= 63), 32-bit byte offsets — and at least 256 tiles PER BatchNorm GROUP: the pipeline pays
// when a workgroup walks several tiles (conv3 forward at bs = 256: 450 tiles per group, 102 -> 92 us); with about one tile per
// workgroup the 4-wave synchronous kernel is faster (bs = 32: 33 us against 51).  Per group, not per launch: one group alone and the
// batched pair of a step must take the same kernel (their statistics are compared bit for bit, and the two kernels sum a tile's
// partial in different orders).
constexpr int GATHER_PIPE_MIN_TILES_PER_GROUP = 256;
bool conv64::gather_pipe_ok(const Prog& P) {
  if (P.tpg < GATHER_PIPE_MIN_TILES_PER_GROUP) return false;
  return taps_grouped_4221(P) && P.G <= 2 && fits_32bit_buffer_bytes(P) && TM + P.span <= GP_RP * GP_BATCH && GP_RP <= P.PHW &&
         -P.min_off <= P.PHW;
}

// The launch of a program gather_pipe_ok accepts (conv64.hip: launch_fwd)
int conv64::launch_gather_pipe(const float* src, const float* wpack, float* dst, float* stats, const Prog& P, hipStream_t st) {
  const int ntiles = P.G * P.tpg;
  int pgrid = 2 * srlz_device_cus();
  if (pgrid > ntiles) pgrid = ntiles;
  pgrid &= ~7;
  if (pgrid < 8) pgrid = 8;  // (the XCD walk wants a multiple of 8 workgroups; those without a tile leave at once)
  const size_t plds = (size_t)(TM + P.span) * 256 + 16384 + 6 * TM * 4 + GT_WORDS * 4 + 8 * 64 * 4;
  SRLZ_MAX_LDS(conv64_gather_pipe_kernel, plds);
  SRLZ_LAUNCH(conv64_gather_pipe_kernel, dim3(pgrid), dim3(GP_THREADS), plds, st, src, wpack, dst, stats, ConvProg{P}, ntiles);
  return 0;
}

// conv64_scatter_pipe_kernel takes the forward program of a stride-2 ConvTranspose — one source class, the destination classes in tap
// groups {4, 2, 2, 1} — with at most two BatchNorm groups, at most 192 staged rows (PW <= 63), 32-bit buffer offsets and the tile
// tables' limits of conv64_fwd_kernel, from SCATTER_PIPE_MIN_TILES_PER_GROUP tiles per BatchNorm group on (per group, as above: one
// group alone and the batched pair take the same kernel — here they would agree bit for bit either way).  Single-kernel timing at
// N = 512 in two groups, fused operand + bias + statistics, against conv64_fwd_kernel: 111 x 111 (6272 tiles per group) 1011 us against
// 1102, 55 x 55 (1568) 274 against 291, 27 x 27 (392) 88 against 90; just above the threshold (27 x 27 and 55 x 55 at 261 / 264 tiles
// per group) 68.1 / 68.6 against 70.6 / 70.7.  Below it the 512 persistent workgroups have about one tile each and nothing to prefetch
// under: the synchronous kernel keeps those (ConvT1 at bs = 256: 98 tiles per group).
constexpr int SCATTER_PIPE_MIN_TILES_PER_GROUP = 256;
bool conv64::scatter_pipe_ok(const Prog& P) {
  if (P.tpg < SCATTER_PIPE_MIN_TILES_PER_GROUP) return false;
  bool grouped = P.s2 && P.ss == 1 && P.ds == 2 && !P.dbg;
  for (int t = 0; t < NTAPS; ++t) grouped = grouped && P.tsrc[t] == 0 && P.tdst[t] == P.tdst[t < 4 ? 0 : t < 6 ? 4 : t < 8 ? 6 : 8];
  return grouped && P.G <= 2 && fits_32bit_buffer_bytes(P) && fits_32bit_src_floats(P) && fits_32bit_dst_rowinfo(P) &&
         fits_31bit_grid(P, TM + P.span) && TM + P.span <= SP_RP * SP_BATCH && -P.min_off <= P.PHW;
}

// The launch of a program scatter_pipe_ok accepts (conv64.hip: launch_fwd); bnp: the fused operand's BatchNorm records or NULL
int conv64::launch_scatter_pipe(const float* src, const float* wpack, const float* bias, float* dst, float* stats, const float* bnp,
                                const Prog& P, hipStream_t st) {
  const int ntiles = P.G * P.tpg;
  int pgrid = 2 * srlz_device_cus();
  if (pgrid > ntiles) pgrid = ntiles;
  pgrid &= ~7;
  if (pgrid < 8) pgrid = 8;
  // source rows, slab, rowinfo (two tiles), row table, fused-operand records, statistics on their way out
  const size_t plds = (size_t)(TM + P.span) * 256 + 16384 + 2 * TM * 4 + ST_WORDS * 4 + 256 * 4 + 512 * 4 + 16;
  if (bnp) {
    SRLZ_MAX_LDS(conv64_scatter_pipe_kernel<true>, plds);
    SRLZ_LAUNCH(conv64_scatter_pipe_kernel<true>, dim3(pgrid), dim3(SP_THREADS), plds, st, src, wpack, bias, dst, stats, ConvProg{P},
                ntiles, bnp);
  } else {
    SRLZ_MAX_LDS(conv64_scatter_pipe_kernel<false>, plds);
    SRLZ_LAUNCH(conv64_scatter_pipe_kernel<false>, dim3(pgrid), dim3(SP_THREADS), plds, st, src, wpack, bias, dst, stats, ConvProg{P},
                ntiles, bnp);
  }
  return 0;
}

extern "C" int srlz_conv64_scatter_pipe_supported(const srlz_conv64_desc* d, int backward_data) {
  ConvProg P;
  if (backward_data || conv64::with_program(d, 0, &P)) return 0;  // (the data-gradient launches keep conv64_fwd_kernel)
  return conv64::scatter_pipe_ok(P) ? 1 : 0;
}

// conv64_bwd_fused_kernel: the same programs without padding (min_off == 0), and at least 8 tiles
static bool fused_bwd_ok(const ConvProg& P) {
  // the second and fourth class are requested and landed for the rows their taps can reach only (FB_NJ1 / FB_NJ3); they share the
  // short LDS buffer As1 (TM + FB_REACH1 rows)
  const bool reach = P.toff[4] >= 0 && P.toff[5] >= 0 && P.toff[4] < FB_REACH1 && P.toff[5] < FB_REACH1 && P.toff[8] >= 0 &&
                     P.toff[8] <= FB_REACH3;
  return taps_grouped_4221(P) && P.G <= 2 && P.min_off == 0 && fits_32bit_buffer_bytes(P) && reach &&
         TM + P.span <= GP_RP * GP_BATCH && GP_RP <= P.PHW && P.G * P.tpg >= 8;
}

// ---- the fused backward of a decoder block's ConvTranspose (conv64_bwd_fused_kernel) ----
static int fused_bwd_grid(const ConvProg& P) {
  int g = srlz_device_cus() & ~7;  // ONE workgroup per CU (150 KB of LDS, 256 registers per lane); a multiple of 8 for the XCD walk
  const int ntiles = P.G * P.tpg;
  // fewer tiles than CUs: rounded UP to the multiple of 8 (a workgroup without a tile leaves a zero partial) — rounded down, 98 tiles
  // (ConvT1's backward at bs = 32) ran on 96 workgroups, two of which took a second tile: 99 us for 50 us of work
  if (g > ntiles) g = (ntiles + 7) & ~7;
  return g;
}

extern "C" int srlz_conv64_gather_pipe_supported(const srlz_conv64_desc* d, int backward_data) {
  ConvProg P;
  if (conv64::with_program(d, backward_data, &P)) return 0;
  return conv64::gather_pipe_ok(P) ? 1 : 0;
}

extern "C" int srlz_conv64_bwd_fused_supported(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 1, &P) || !d->transposed || d->stride != 2) return 0;
  return fused_bwd_ok(P) ? 1 : 0;
}

extern "C" int srlz_conv64_bwd_fused_bn_rows(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 1, &P)) return -1;
  return P.G * (4 * P.tpg + BNZ_BLOCKS);
}

extern "C" size_t srlz_conv64_bwd_fused_workspace(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 1, &P)) return 0;
  return (size_t)fused_bwd_grid(P) * WGRAD_PARTIAL_FLOATS * sizeof(float);
}

// Host only: the persistent workgroups srlz_conv64_bwd_fused launches (they share the srlz_conv64_bwd_data_tiles(d) tiles).
extern "C" int srlz_conv64_bwd_fused_workgroups(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 1, &P)) return -1;
  return fused_bwd_grid(P);
}

extern "C" int srlz_conv64_bwd_fused(const float* x, const float* x_bnp, const float* dy, const srlz_bn_bwd_operand* dy_bn,
                                     const float* wpack_bwd, float* dx, float* dw_ref, float* dbias, float* x_bn_bwd_partial,
                                     void* ws, size_t ws_bytes, const srlz_conv64_desc* d, srlz_stream_t stream) {
  ConvProg P;
  if (int rc = conv64::with_program(d, 1, &P)) return rc;
  SRLZ_REQUIRE(d->transposed && d->stride == 2, SRLZ_ERR_BAD_DESC, "conv64_bwd_fused: ConvTranspose2d(64, 64, 3, stride 2) only");
  SRLZ_REQUIRE(x && x_bnp && dy && dy_bn && wpack_bwd && dx && dw_ref && ws, SRLZ_ERR_NULL, "conv64_bwd_fused: null pointer");
  OpFuse gf;
  if (int rc = make_bwd_fuse(&gf, dy_bn, "conv64_bwd_fused")) return rc;
  SRLZ_REQUIRE(gf.dy_out == nullptr, SRLZ_ERR_BAD_DESC, "conv64_bwd_fused: d(loss)/dy is not materialised by this entry point");
  SRLZ_REQUIRE(fused_bwd_ok(P), SRLZ_ERR_BAD_DESC, "conv64_bwd_fused: shape not supported (ask srlz_conv64_bwd_fused_supported)");
  const int grid = fused_bwd_grid(P);
  SRLZ_REQUIRE(ws_bytes >= (size_t)grid * WGRAD_PARTIAL_FLOATS * sizeof(float), SRLZ_ERR_WORKSPACE,
               "conv64_bwd_fused: workspace too small (%zu bytes)", ws_bytes);
  hipStream_t st = as_stream(stream);
  // class rows (TM + span; TM + 32 for the short-reach classes), the a-tile, two weight slabs, rowinfo, records, row tables
  const size_t lds = (size_t)(TM + P.span) * 256 + (size_t)(TM + FB_REACH1) * 256 + (size_t)TM * 256 + 2 * 16384 + 6 * TM * 4 + 512 * 4 +
                     256 * 4 + (GT_WORDS + YT_WORDS) * 4 + 2 * 192 * 4;
  SRLZ_REQUIRE(lds <= 160 * 1024, SRLZ_ERR_BAD_DESC, "conv64_bwd_fused: tile needs %zu bytes of LDS", lds);
  FusedBwd fb;
  fb.x = x; fb.x_bnp = x_bnp; fb.wpartial = (float*)ws;
  fb.bnpart = x_bn_bwd_partial; fb.bn_rows = 4 * P.tpg + BNZ_BLOCKS;
  SRLZ_MAX_LDS(conv64_bwd_fused_kernel, lds);
  SRLZ_LAUNCH(conv64_bwd_fused_kernel, dim3(grid), dim3(GP_THREADS), lds, st, dy, wpack_bwd, dx, P, P.G * P.tpg, gf, fb);
  // second stage: fixed-order fp64 sum over the workgroups (the partial's bias block sits behind EACH workgroup's taps here)
  if (int rc = conv64::launch_wgrad_reduce((const float*)ws, grid, dw_ref, dbias, 1, WGRAD_PARTIAL_FLOATS, st)) return rc;
  if (x_bn_bwd_partial) {  // the records of the channels the fused kernel cannot sum from the activation (normally: zeros)
    SRLZ_LAUNCH(conv64_bnpart_zero_scale_kernel, dim3(BNZ_BLOCKS, P.G), dim3(256), 0, st, x, x_bnp, (const float*)dx, x_bn_bwd_partial,
                (long long)P.N * P.Hd * P.Wd, fb.bn_rows, 4 * P.tpg);
  }
  return 0;
}
