// conv64_tile.h — what the kernel families of the 64 -> 64 convolutions share (conv64.hip, conv64_pipe.hip, conv64_wgrad.hip, convn.hip):
// the virtual-grid program (formulation: conv64.hip), the fused operand, the grid walk, the tile stagings and their row table, the 32-bit
// limits the route predicates ask about, and the few host functions that are called from one of those files into another.
#pragma once
#include "common.h"

namespace {

#ifndef SRLZ_BATCH_FWD
#define SRLZ_BATCH_FWD 16
#endif
#ifndef SRLZ_BATCH_BWD
#define SRLZ_BATCH_BWD 12
#endif
constexpr int TM = 128;       // grid positions per forward tile
constexpr int BATCH_FWD = SRLZ_BATCH_FWD;  // rows (of 16 lanes) a thread requests per round trip of a plain / forward-fused staging
constexpr int NTAPS = 9;
constexpr int WGRAD_PARTIAL_FLOATS = NTAPS * 4096 + 64;  // one workgroup's weight-gradient partial: nine 64 x 64 tap blocks, 64 bias sums

}  // namespace

namespace conv64 {

// The virtual-grid program of one launch (formulation: conv64.hip), filled in by build_program
struct Prog {
  int N, PH, PW, PHW, total_q;  // N / total_q: images / grid positions of ONE BatchNorm group
  int G, tpg;                   // groups batched along the image axis (images [g*N, (g+1)*N)); forward tiles per group
  long long src_gstride, dst_gstride;  // floats between two groups' images in src / dst
  int ss, Hs, Ws;  // source: stride, image dims
  int ds, Hd, Wd;  // dest
  int tsrc[NTAPS], tdst[NTAPS], toff[NTAPS], tw[NTAPS];
  int tp[NTAPS + 2];  // the same per tap in one word: toff (low 16 bits, signed) | tw << 16 | tsrc << 20 | tdst << 22; two zero words
                      // behind the last tap (conv64_fwd_kernel fetches two taps ahead)
  int min_off, span;
  int s2;          // 1 if taps are grouped {4,2,2,1} by class, 0 if a single group of 9
  int dbg;         // ablation switches for tools/kbench.py (env SRLZ_ABLATE): 1 skip A staging, 2 skip epilogue
  unsigned mPHW, mPW;  // q / PHW and r / PW for 0 <= q, r < 2^31 as (__umulhi(q, m) >> sh): a run-time integer division is ~20
  int sPHW, sPW;       // VALU instructions and a reciprocal the compiler keeps in a register for the whole kernel (fastdiv)
};

// The host functions that are called across translation units.
// conv64.hip
int build_program(Prog* P, int gather, int stride, int pad, int N, int Hs, int Ws, int Hd, int Wd, int G = 1);
int with_program(const srlz_conv64_desc* d, int backward_data, Prog* P);
// conv64_pipe.hip: does conv64_gather_pipe_kernel take this program (plain operand, no bias), and its launch (launch_fwd decides)
bool gather_pipe_ok(const Prog& P);
int launch_gather_pipe(const float* src, const float* wpack, float* dst, float* stats, const Prog& P, hipStream_t st);
// conv64_pipe.hip: does conv64_scatter_pipe_kernel take this forward program (a stride-2 ConvTranspose's; any bias, plain operand or
// relu(bn(.)) fused), and its launch
bool scatter_pipe_ok(const Prog& P);
int launch_scatter_pipe(const float* src, const float* wpack, const float* bias, float* dst, float* stats, const float* bnp,
                        const Prog& P, hipStream_t st);
// conv64_wgrad.hip: the second stage of every weight gradient, conv64_wgrad_reduce over nwg workgroups' partials
int launch_wgrad_reduce(const float* partial, int nwg, float* dw_ref, float* dbias, int transposed, int interleaved, hipStream_t st);

}  // namespace conv64

namespace {

// The program as a kernel takes it, by value.  Everything device-side lives in the anonymous namespace (a kernel's name carries its
// argument types); a function that is called across translation units cannot take a type from there, so those take the named base.
struct ConvProg : conv64::Prog {};

// ---------------------------------------------------------------------------------------------------------------
// Tile staging: rows [qstart, qstart+nrows) of class `cls` of an NHWC/64 tensor -> LDS (256 B per row).
// 16 lanes fetch one row (256 contiguous bytes); out-of-range rows are zero-filled.
// ---------------------------------------------------------------------------------------------------------------
// How raw rows become the operand (OpFuse):
//  * bnp != NULL, y == NULL: the source is the RAW output of a convolution and the consumer wants relu(batchnorm(.)):
//    the affine (scale = bnp[128..], shift = bnp[192..]) and the ReLU are applied to in-bounds rows on the way into
//    LDS, so the activated tensor is never materialised in HBM (padding rows stay exactly zero).
//  * y != NULL: the source is dA = d(loss)/d(relu(bn(y))) and the consumer wants dy = d(loss)/dy, the BatchNorm + ReLU
//    BACKWARD: dy = scale*(dA*[bn(y)>0] - S1/count - xhat*S2/count) = scale*dz - (c0 + c1*y), rebuilt from (dA, y) and
//    the two per-channel sums of srlz_bn_relu_bwd_sums, so dy is never materialised either.
//    With dy_out != NULL every rebuilt element whose grid position lies in this tile's own range [core_lo, core_lo+TM)
//    is also written to dy_out (each element exactly once across the launch): the data-gradient kernel materialises
//    the tensor for the weight-gradient kernel as a by-product of its staging, replacing the separate apply pass.
struct OpFuse {
  const float* bnp;
  const float* y;
  const float* sums;
  float inv_count;
  int training;
  float* dy_out;
};
#define SRLZ_NO_FUSE OpFuse{nullptr, nullptr, nullptr, 0.f, 0, nullptr}

// The records of BatchNorm group `grp` (bnp: 256 floats per group, sums: 128) and the group's slice of the tensors that are
// indexed like the staged source (y, dy_out): `goff` floats further.
__device__ __forceinline__ OpFuse fuse_for_group(OpFuse f, int grp, long long goff) {
  if (f.bnp) f.bnp += grp * 256;
  if (f.sums) f.sums += grp * 128;
  if (f.y) f.y += goff;
  if (f.dy_out) f.dy_out += goff;
  return f;
}

// ---------------------------------------------------------------------------------------------------------------
// The grid walk: position q of ONE BatchNorm group's virtual grid -> image n, grid row a, grid column b (q = (n * PH + a) * PW + b)
// -> the position's class-(0,0) pixel (y, x) = (a * stride, b * stride) in a tensor of that stride.
// SHIFTED: q may lie up to one image BEFORE position 0 (the staged range of a padded program starts at min_off < 0): the divisions
// are done on q + PHW, which stays non-negative, and n is -1 for those positions.
// Every table builder below and the kernels' destination-side rowinfo go through here.
// ---------------------------------------------------------------------------------------------------------------
struct GridPix { int n, y, x; };
template <bool SHIFTED>
__device__ __forceinline__ GridPix grid_pix(const ConvProg& P, int q, int stride) {
  const int qq = SHIFTED ? q + P.PHW : q;
  const int n1 = fastdiv(qq, P.mPHW, P.sPHW);
  const int rem = qq - n1 * P.PHW;
  const int a = fastdiv(rem, P.mPW, P.sPW);
  const int y = a * stride, x = (rem - a * P.PW) * stride;
  return GridPix{SHIFTED ? n1 - 1 : n1, y, x};
}

// Source-side table entry of position q for a source of stride `ss`: pixel index of the position's class-(0,0) source pixel << 4 |
// bit k: source class k = (cy << 1) | cx is inside the image; 0 = no image (then no class is).  A staging of class k is then, per row:
// a bit-field extract, an add-shift and an AND (stage_rows_tab, gather_request, plain_request, conv64_wgrad_gather_kernel).
template <bool SHIFTED>
__device__ __forceinline__ unsigned src_entry(const ConvProg& P, int q, int ss) {
  const GridPix g = grid_pix<SHIFTED>(P, q, ss);
  if (SHIFTED ? (unsigned)g.n < (unsigned)P.N : g.n < P.N) {
    unsigned f = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) f |= (g.y + (k >> 1) < P.Hs && g.x + (k & 1) < P.Ws) ? 1u << k : 0u;
    return ((unsigned)((g.n * P.Hs + g.y) * P.Ws + g.x) << 4) | f;
  }
  return 0;
}

// One-pixel table entry of a row inside the tensor: pixel index << 1 | 1 (0 = outside: such a row reads pixel 0 and is dropped)
__device__ __forceinline__ unsigned pix_entry(int n, int y, int x, int H, int W) { return ((unsigned)((n * H + y) * W + x) << 1) | 1u; }

// Reciprocals of the virtual grid's PH * PW and PW (fastdiv) for rows64_load.
struct GridDiv { unsigned mPHW, mPW; int sPHW, sPW; };
__device__ __forceinline__ GridDiv grid_div(const ConvProg& P) { return GridDiv{P.mPHW, P.mPW, P.sPHW, P.sPW}; }

template <bool SWZ, int BATCH = 8, int NTHREADS = 256, bool BWD = false>
__device__ __forceinline__ void stage_rows(float* __restrict__ lds, const float* __restrict__ src, int H, int W,
                                           int stride, int cls, int PW, int PH, int total_q, int qstart,
                                           int nrows, const OpFuse f = SRLZ_NO_FUSE, int core_lo = 0, int core_n = 0,
                                           int cstride = 64, int coff = 0, const float* __restrict__ lrec = nullptr) {
  // lrec != NULL: the per-channel coefficients of the fused operand (scale, shift, c0, c1: 4 x 64 floats) have been put in LDS by
  // the caller, once per workgroup — read from the global records at every call they cost two to three dependent L2 round trips in
  // front of each staging (four stagings per tile for the stride-2 gather programs)
  // cstride / coff: the tensor has `cstride` channels per pixel and this call stages channels [coff, coff + 64) (convN_*)
  const float* __restrict__ bnp = f.bnp;
  // Loads are issued in batches of 8 rows per thread before any LDS store, so the HBM/L2 latency is paid once per
  // batch instead of once per row; (n, a, b) of a thread's rows are advanced incrementally (rows are NTHREADS/16 apart), the
  // only integer divisions are the two for its first row.
  const int t = threadIdx.x;
  const int slot = t & 15;
  const int cy = cls >> 1, cx = cls & 1;
  const int PHW = PH * PW;
  constexpr int RP = NTHREADS / 16;  // rows per pass
  // (its own walk, not grid_pix — true divisions: with the uniform divisors hipcc keeps one reciprocal per kernel, and fastdiv here measured 0.5 % SLOWER in
  // conv64_fwd_kernel — unlike in rows64_load, where it is worth 1.5 % of the weight-gradient ring)
  // a pass advances RP grid positions = sn images + sa rows + sb columns (sa < PH, sb < PW): one carry per digit below is then enough
  // on any grid — with sa = RP / PW alone a grid of fewer than RP / PW + 1 rows (maps of a few pixels, several images) carried past
  // two images at once and the rows behind the first pass were staged from the wrong pixels
  const int sn = RP / PHW, srem = RP - sn * PHW;
  const int sa = srem / PW, sb = srem - sa * PW;
  // shift by one image so the first rows of the first tile (negative q) stay non-negative: n1 = n + 1
  const int qq = qstart + (t >> 4) + PHW;
  int n1 = qq / PHW;
  int rem = qq - n1 * PHW;
  int a = rem / PW;
  int b = rem - a * PW;
  const int N1max = total_q / PHW;  // images
  f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
  if (lrec) {
    sc4 = *(const f32x4*)(lrec + slot * 4); sh4 = *(const f32x4*)(lrec + 64 + slot * 4);
    if (BWD) { c0 = *(const f32x4*)(lrec + 128 + slot * 4); c1 = *(const f32x4*)(lrec + 192 + slot * 4); }
  } else if (bnp) { sc4 = *(const f32x4*)(bnp + 128 + slot * 4); sh4 = *(const f32x4*)(bnp + 192 + slot * 4); }
  if (!lrec && BWD && f.training) {
    const f32x4 mean = *(const f32x4*)(bnp + slot * 4), invstd = *(const f32x4*)(bnp + 64 + slot * 4);
    const f32x4 m1 = *(const f32x4*)(f.sums + slot * 4), m2 = *(const f32x4*)(f.sums + 64 + slot * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c1[e] = sc4[e] * invstd[e] * m2[e] * f.inv_count;
      c0[e] = sc4[e] * m1[e] * f.inv_count - c1[e] * mean[e];
    }
  }
  for (int base = t >> 4; base < nrows; base += RP * BATCH) {
    f32x4 v[BATCH], yv[BWD ? BATCH : 1];
    unsigned offs[BWD ? BATCH : 1];  // float offsets of the rows (a group's tensor has < 2^32 floats: checked by the host)
    unsigned okmask = 0;
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int y = a * stride + cy, x = b * stride + cx;
      const bool ok = base + RP * j < nrows && n1 >= 1 && n1 <= N1max && y < H && x < W;
      okmask |= (ok ? 1u : 0u) << j;
      // Branch-free: a padding row reads pixel 0 (always valid) and is zeroed when it is consumed.  With a load inside a branch the
      // compiler cannot tell, after the join, which loads are still in flight; every later first write of a register such a load
      // once targeted then gets "s_waitcnt vmcnt(0)" — in the caller that was the first MFMA of each tap, i.e. the prefetch of the
      // next weight slab was waited for before the MFMAs it is meant to hide behind.
      const size_t off = (ok ? ((size_t)((n1 - 1) * H + y) * W + x) * cstride : (size_t)0) + coff + slot * 4;
      v[j] = *(const f32x4*)(src + off);
      if (BWD) { yv[j] = *(const f32x4*)(f.y + off); offs[j] = (unsigned)off; }
      b += sb; a += sa; n1 += sn;
      if (b >= PW) { b -= PW; ++a; }
      if (a >= PH) { a -= PH; ++n1; }
    }
    // All loads of the batch are waited for HERE, once, in straight-line code: the rows below are consumed inside branches, and
    // after a branch join the compiler no longer knows which loads have landed.  It then protects every later re-use of one of
    // these registers with "s_waitcnt vmcnt(0)": in the fused data-gradient that wait sat behind every dy_out store (one HBM
    // round trip per store), in the caller's tap loop in front of the first MFMA of every tap (defeating the slab prefetch).
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      asm volatile("" : "+v"(v[j]));
      if (BWD) asm volatile("" : "+v"(yv[BWD ? j : 0]));
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int R = base + RP * j;
      if (R < nrows) {
        if (!((okmask >> j) & 1u)) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        else if (bnp) {
          if (BWD) {
            // (explicit fused multiply-adds: the same roundings in every kernel that rebuilds dy — as whole-vector operations, which
            // hipcc issues as v_pk_fma_f32, two elements per instruction slot: every instruction next to the MFMAs costs matrix time)
            const f32x4 z4 = __builtin_elementwise_fma(yv[j], sc4, sh4), t4 = __builtin_elementwise_fma(c1, yv[j], c0);
            f32x4 dz4;
#pragma unroll
            for (int e = 0; e < 4; ++e) dz4[e] = z4[e] > 0.f ? v[j][e] : 0.f;
            v[j] = __builtin_elementwise_fma(sc4, dz4, -t4);
            if (f.dy_out && (unsigned)(R - core_lo) < (unsigned)core_n) *(f32x4*)(f.dy_out + (size_t)offs[j]) = v[j];
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float z = v[j][e] * sc4[e] + sh4[e]; v[j][e] = z > 0.f ? z : 0.f; }
          }
        }
        const int sl = SWZ ? (slot ^ (R & 15)) : slot;
        *(f32x4*)(lds + R * 64 + sl * 4) = v[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The row table of a forward tile.  stage_rows walks (image, row, column) per staged row and thread: with the bounds tests, the
// pixel offset and the 64-bit address that is ~30 vector-ALU instructions per row (two of them quarter-rate 64-bit multiply-adds),
// 16 rows per thread and tile — a sixth of everything conv64_fwd_kernel issues next to its MFMAs, each costing matrix time
// (DESIGN.md 5.3).  Here every thread decomposes ONE row of the tile's range [qstart, qstart + nrows) into a table in LDS, once per
// tile:   entry = pixel index of the row's class-(0,0) source pixel << 4 | bit k: source class k = (cy << 1) | cx is inside the image
// (0: no class is), and a staging is then, per row: one quarter of a ds_read_b128, a bit-field extract, an add-shift, two ANDs and the
// address add.  The four stagings of a stride-2 gather tile share the table.
// Layout: entry of row R at (R & 15) * tpa + (R >> 4): the rows of thread t (R = (t >> 4) + 16 j) are consecutive words.
// tpa = passes over the tile's rows rounded up to the batch (entries past nrows are 0: such a row reads pixel 0 and is dropped).
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int rowtab_passes(int nrows) { return ((nrows + 15) / 16 + SRLZ_BATCH_FWD - 1) / SRLZ_BATCH_FWD * SRLZ_BATCH_FWD; }

__device__ __forceinline__ void rowtab_build(unsigned* __restrict__ tab, int tpa, const ConvProg& P, int qstart, int nrows) {
  for (int R = threadIdx.x; R < 16 * tpa; R += blockDim.x) {
    unsigned e = 0;
    if (R < nrows) e = src_entry<true>(P, qstart + R, P.ss);
    tab[(R & 15) * tpa + (R >> 4)] = e;
  }
}

// Rows of source class `cls` -> LDS (swizzled), through the table.  lrec != NULL: relu(batchnorm(.)) on the way in (scale, shift in LDS).
// cshift / coff: the tensor has 2^cshift channels per pixel and channels [coff, coff + 64) are staged (convN_fwd_kernel; the 64-channel
// kernels pass the defaults, which fold to the constants they had)
template <int BATCH>
__device__ __forceinline__ void stage_rows_tab(float* __restrict__ lds, const float* __restrict__ src,
                                               const unsigned* __restrict__ tab, int tpa, int cls, int W, int nrows,
                                               const float* __restrict__ lrec, int cshift = 6, int coff = 0) {
  const int t = threadIdx.x;
  const int slot = t & 15, r = t >> 4;
  const unsigned delta = (unsigned)((cls >> 1) * W + (cls & 1));
  const float* __restrict__ base = src + coff + slot * 4;
  f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
  if (lrec) { sc4 = *(const f32x4*)(lrec + slot * 4); sh4 = *(const f32x4*)(lrec + 64 + slot * 4); }
  for (int j0 = 0; j0 < tpa; j0 += BATCH) {
    f32x4 v[BATCH];
    unsigned okmask = 0;
#pragma unroll
    for (int jj = 0; jj < BATCH; jj += 4) {  // (four entries at a time: all sixteen up front cost 12 registers the pooled-block kernel lacks)
      const uint4 q = *(const uint4*)(tab + r * tpa + j0 + jj);
      const unsigned e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = jj + i;
        // branch-free (see stage_rows): m = all ones where the row's pixel of this class exists; any other row reads pixel 0
        const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)e[i], (unsigned)cls, 1u);
        const unsigned off = (((e[i] >> 4) + delta) << cshift) & m;  // floats (a group's tensor has < 2^32: checked by the host)
        v[j] = *(const f32x4*)(base + off);
        okmask |= m & (1u << j);
      }
    }
    // all loads of the batch are waited for here, once, in straight-line code (see stage_rows)
#pragma unroll
    for (int j = 0; j < BATCH; ++j) asm volatile("" : "+v"(v[j]));
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int R = r + 16 * (j0 + j);
      if (R < nrows) {
        if (!((okmask >> j) & 1u)) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        else if (lrec) {
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) { const float z = v[j][e2] * sc4[e2] + sh4[e2]; v[j][e2] = z > 0.f ? z : 0.f; }
        }
        *(f32x4*)(lds + R * 64 + ((slot ^ (R & 15)) << 2)) = v[j];
      }
    }
  }
}

// ---- What the route predicates of every family ask about a program (host) ----
// A stride-2 gather program as the pipelined kernels expect it: four source classes in tap groups {4, 2, 2, 1} (taps 0-3, 4-5, 6-7, 8),
// one destination class (conv3's forward, a ConvTranspose's data gradient); never under an ablation switch.
inline bool taps_grouped_4221(const conv64::Prog& P) {
  bool grouped = P.s2 && P.ss == 2 && !P.dbg;
  for (int t = 0; t < NTAPS; ++t) grouped = grouped && P.tsrc[t] == P.tsrc[t < 4 ? 0 : t < 6 ? 4 : t < 8 ? 6 : 8] && P.tdst[t] == 0;
  return grouped;
}

// The 32-bit limits (all per BatchNorm group: P.N images).
// byte offsets into buffer resources over one group's src / dst, with room below the DROP offset of a lane that must not store
inline bool fits_32bit_buffer_bytes(const conv64::Prog& P) {
  return P.src_gstride * 4 < (1LL << 32) - 65536 && P.dst_gstride * 4 < (1LL << 32) - 65536;
}
// float offsets of the stagings and row tables into one group's src / dst
inline bool fits_32bit_src_floats(const conv64::Prog& P) { return (long long)P.N * P.Hs * P.Ws * 64 < (1LL << 32); }
inline bool fits_32bit_dst_floats(const conv64::Prog& P) { return (long long)P.N * P.Hd * P.Wd * 64 < (1LL << 32); }
// the destination word of a forward tile (rowinfo): pixel index << 2 | two bits, negative = outside
inline bool fits_32bit_dst_rowinfo(const conv64::Prog& P) { return (long long)P.N * P.Hd * P.Wd < (1LL << 29); }
// fastdiv takes dividends below 2^31: the last grid position + the one-image shift + how far a kernel stages past it
inline bool fits_31bit_grid(const conv64::Prog& P, int reach) { return (long long)P.total_q + P.PHW + reach < (1LL << 31); }

// host view of the fused BatchNorm-backward operand (include/srlz.h: srlz_bn_bwd_operand)
inline int make_bwd_fuse(OpFuse* f, const srlz_bn_bwd_operand* o, const char* who) {
  *f = SRLZ_NO_FUSE;
  if (!o) return 0;
  SRLZ_REQUIRE(o->y && o->bnp && o->sums && o->count > 0, SRLZ_ERR_NULL, "%s: incomplete srlz_bn_bwd_operand", who);
  f->bnp = o->bnp; f->y = o->y; f->sums = o->sums; f->training = o->training;
  f->inv_count = 1.0f / (float)(double)o->count;
  f->dy_out = o->dy_out;
  return 0;
}

}  // namespace
