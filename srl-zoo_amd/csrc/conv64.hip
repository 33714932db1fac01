// conv64.hip — 3x3, 64->64 channel convolutions and transposed convolutions (stride 1 / 2) as fp32-MFMA implicit GEMM.
//
// Replaces (forward + autograd backward) nn.Conv2d / nn.ConvTranspose2d of /root/reference/models/models.py:54,59
// (conv3x3 s1/s2) and :66,70,74,78 (ConvTranspose2d(64,64,3,stride=2) x4).
//
// One formulation covers every case ("virtual-grid program"):
//   * a virtual grid of PH x PW positions per image, flattened to q = (n*PH + a)*PW + b;
//   * source class c = (cy,cx):  S_c(q) = src[n, a*ss+cy, b*ss+cx, :]  (64 floats) if in bounds, else 0;
//   * dest   class d = (dy,dx):  D_d(q) -> dst[n, a*ds+dy, b*ds+dx, :] if in bounds, else discarded;
//   * D_d(q) = sum over taps t of  S_{c_t}(q + off_t) . W[w_t]   (W[w] is a 64x64 slab of the 3x3 kernel).
// PH/PW carry one spare (zero) row/column so that a flat offset never wraps onto real data (see build_program).
//   conv s1         : 1 src class, 1 dst class, 9 taps          (conv2 fwd, conv2 dgrad)
//   conv s2 (gather): 4 src classes (input parity), 1 dst class  (conv3 fwd, ConvT dgrad)
//   convT s2 (scatter): 1 src class, 4 dst classes (output parity, 4/2/2/1 taps) (ConvT fwd, conv3 dgrad)
// GEMM view per tile: M = 128 grid positions, N = 64 output channels, K = 64 input channels per tap.
//
// Kernel structure (fwd): 256 threads = 4 waves, wave w owns rows [32w,32w+32) x 64 columns = two 32x32
// v_mfma_f32_32x32x2_f32 accumulators.  The source rows the tile touches (128 + halo) are staged ONCE in LDS and
// re-used by all taps; the weight slab of the current tap (16 KB) is staged per tap.  Both operands are read with
// ds_read_b128: lanes 0-31 take k = 8c..8c+3 and lanes 32-63 k = 8c+4..8c+7 of a chunk (MFMA k-order is free as
// long as A and B agree), so one 16-byte read feeds four MFMAs.  Rows are 256 B; the 16-byte slot index is XORed
// with (row & 15) so a 16-lane ds_read_b128 group (consecutive rows, same k) covers all 64 banks.
// LDS: (128+116)*256 + 16384 + 1024 + 512 + 1024 = 81408 B for conv2 (source rows, slab, the tile's row table, one word per output
// position, fused-operand coefficients) -> 2 workgroups per CU (81920 B each), which is what hides the staging.
// Epilogue: accumulators leave through a wave-private 4 KB transposition buffer (the wave's own quarter of the idle slab), so
// that every global store is 16 bytes per lane (flush16).  See DESIGN.md 5.2 for what the generated ISA taught about this file.
#include "conv64_tile.h"
#include <stdlib.h>

// GATHER: out[o] = sum_k in[o*s - p + k];  SCATTER: out[o] = sum_{k: (o+p-k)%s==0} in[(o+p-k)/s]
static int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

// Build the program.  gather != 0: conv-like (dst is the low-res / same-res side); else convT-like.
int conv64::build_program(Prog* P, int gather, int stride, int pad, int N, int Hs, int Ws, int Hd, int Wd, int G) {
  if (stride != 1 && stride != 2) return -1;
  if (G < 1 || N % G != 0) return -1;
  N /= G;  // the virtual grid covers ONE group; a tile / chunk never straddles two groups (see conv64_fwd_kernel)
  P->N = N; P->Hs = Hs; P->Ws = Ws; P->Hd = Hd; P->Wd = Wd;
  P->G = G;
  P->src_gstride = (long long)N * Hs * Ws * 64;
  P->dst_gstride = (long long)N * Hd * Wd * 64;
  int kcls[3], kd[3];  // identical for both axes (square kernel, same stride/pad)
  if (gather) {
    P->ss = stride; P->ds = 1;
    for (int k = 0; k < 3; ++k) {
      int t = k - pad;
      int c = ((t % stride) + stride) % stride;
      kcls[k] = c; kd[k] = (t - c) / stride;
    }
  } else {
    P->ss = 1; P->ds = stride;
    // for dest class py: k valid iff (py + pad - k) % stride == 0; exactly one py per k
    for (int k = 0; k < 3; ++k) {
      int py = (((k - pad) % stride) + stride) % stride;
      kcls[k] = py; kd[k] = floordiv(py + pad - k, stride);
      if ((py + pad - k) != kd[k] * stride) return -1;
    }
  }
  // grid extents per axis
  auto extent = [&](int Hsrc, int Hdst) {
    int mx = 0, mn = 0;
    for (int k = 0; k < 3; ++k) { if (kd[k] > mx) mx = kd[k]; if (kd[k] < mn) mn = kd[k]; }
    int n_out = (Hdst + P->ds - 1) / P->ds;
    int n_src = (Hsrc + P->ss - 1) / P->ss;
    int ph = n_out + mx; if (n_src > ph) ph = n_src;
    if (mn < 0) {
      // the last row must read as zero for every source class (it is what offset -1 wraps onto)
      bool nonzero = false;
      for (int c = 0; c < P->ss; ++c) if (P->ss * (ph - 1) + c < Hsrc) nonzero = true;
      if (nonzero) ph += 1;
      if (mn < -1) return -1;
    }
    return ph;
  };
  P->PH = extent(Hs, Hd);
  P->PW = extent(Ws, Wd);
  if (P->PH <= 0 || P->PW <= 0) return -1;
  P->PHW = P->PH * P->PW;
  if (P->PW < 2) return -1;
  fastdiv_init((unsigned)P->PHW, &P->mPHW, &P->sPHW);
  fastdiv_init((unsigned)P->PW, &P->mPW, &P->sPW);
  long long tq = (long long)N * P->PHW;
  if (tq > 0x7fffff00LL) return -1;
  P->total_q = (int)tq;
  P->tpg = (P->total_q + TM - 1) / TM;
  // taps, grouped by class, groups in descending size (4,2,2,1 for stride 2)
  int nclass = stride * stride;
  int order[4] = {0, 1, 2, 3}, cnt[4] = {0, 0, 0, 0};
  for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx) cnt[kcls[ky] * stride + kcls[kx]]++;
  for (int i = 0; i < nclass; ++i) for (int j = i + 1; j < nclass; ++j)
    if (cnt[order[j]] > cnt[order[i]]) { int t = order[i]; order[i] = order[j]; order[j] = t; }
  if (nclass == 4 && cnt[order[1]] == cnt[order[2]]) {
    // Of the two 2-tap classes the one whose taps reach LESS far ahead comes first (round 6).  conv64_bwd_fused_kernel keeps the
    // classes of a tile in two alternating LDS buffers (classes 0 / 2 in one, 1 / 3 in the other): with the {0, +1} class second
    // and the 1-tap class fourth the second buffer needs TM + 1 rows instead of TM + PW, which is what makes room for a second
    // weight slab (one barrier per tap instead of two).  Every kernel reads the order from the program: results differ from the
    // other order by the summation order of the taps only.
    int reach[4] = {0, 0, 0, 0};
    for (int c = 0; c < 4; ++c)
      for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx)
        if (kcls[ky] * stride + kcls[kx] == c) { const int o = kd[ky] * P->PW + kd[kx]; if (o > reach[c]) reach[c] = o; }
    if (reach[order[2]] < reach[order[1]]) { int t = order[1]; order[1] = order[2]; order[2] = t; }
  }
  int nt = 0;
  P->min_off = 0; int max_off = 0;
  for (int g = 0; g < nclass; ++g) {
    int cy = order[g] / stride, cx = order[g] % stride;
    for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx) {
      if (kcls[ky] != cy || kcls[kx] != cx) continue;
      int cls2 = cy * 2 + cx;  // class encoding used by the kernels: (cy<<1)|cx
      P->tsrc[nt] = gather ? cls2 : 0;
      P->tdst[nt] = gather ? 0 : cls2;
      P->toff[nt] = kd[ky] * P->PW + kd[kx];
      P->tw[nt] = ky * 3 + kx;
      if (P->toff[nt] < P->min_off) P->min_off = P->toff[nt];
      if (P->toff[nt] > max_off) max_off = P->toff[nt];
      nt++;
    }
  }
  if (nt != NTAPS) return -1;
  for (int t = 0; t < NTAPS; ++t) {
    if (P->toff[t] < -32768 || P->toff[t] > 32767) return -1;
    P->tp[t] = (P->toff[t] & 0xffff) | (P->tw[t] << 16) | (P->tsrc[t] << 20) | (P->tdst[t] << 22);
  }
  P->tp[NTAPS] = P->tp[NTAPS + 1] = 0;
  P->span = max_off - P->min_off;
  P->s2 = (stride == 2);
  { const char* e = getenv("SRLZ_ABLATE"); P->dbg = e ? atoi(e) : 0; }
  if (P->s2 && !(cnt[order[0]] == 4 && cnt[order[1]] == 2 && cnt[order[2]] == 2 && cnt[order[3]] == 1)) return -1;
  return 0;
}

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Forward / data-gradient kernel.  NW = waves per workgroup: 4 (wave = 32 rows x 64 columns, two accumulators) or
// 8 (wave = 32 rows x 32 columns, one accumulator; twice the waves per SIMD to hide barriers, LDS and staging latency).
// ---------------------------------------------------------------------------------------------------------------
// BWD = true is the data-gradient launch whose operand is rebuilt from (dA, y) by the fused BatchNorm+ReLU backward (and
// optionally stored): a separate instantiation, so the plain kernel keeps its register budget and shows up under its own
// name in rocprof.
// PSUM: 0 = statistics of a forward launch; 1 / 2 = the pooled-block epilogue (PoolSum) of a data gradient with ONE destination class
// (its pooled values are requested before the first tap and travel under the whole tile) / with several (requested inside every
// flush: the small stride-2 layer).
// (The body is shared by two kernel symbols: conv64_fwd_kernel<NW, BWD> — PSUM = 0, what rocprof has listed since round 1 — and
// conv64_dgrad_poolsum_kernel<PSUM>.)
template <int NW, bool BWD, int PSUM>
__device__ __forceinline__ void conv64_fwd_body(const float* __restrict__ src, const float* __restrict__ wpack,
                                                const float* __restrict__ bias, float* __restrict__ dst,
                                                float* __restrict__ stats_partial, const ConvProg& P, int ntiles,
                                                const OpFuse& src_fuse_all, const PoolSum& ps) {
  static_assert(NW == 4, "8 waves of 32 x 32 measured within +-3 % in rounds 1-3 and are not kept");
  static_assert(PSUM == 0 || !BWD, "the pooled-block epilogue exists for the plain kernel");
  constexpr int NT = NW * 64;      // threads
  constexpr int NACC = 8 / NW;     // 32-column tiles per wave
  // rows (of 16 lanes) a thread requests per HBM round trip of the source staging: a stride-1 tile (244 rows = 15.25 passes) or a
  // gather class (185 rows = 11.6 passes) in ONE batch instead of two
  constexpr int BATCH_BWD = SRLZ_BATCH_BWD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* As = (float*)smem;                 // (TM + span) x 64, swizzled
  float* Bs = As + (TM + P.span) * 64;      // 64 x 64 weight slab of the current tap, pre-swizzled in global
  const int tpa = rowtab_passes(TM + P.span);
  unsigned* rowtab = (unsigned*)(Bs + 4096);  // [16][tpa]: the source-side row table (rowtab_build)
  int* rowinfo = (int*)(rowtab + 16 * tpa);   // [TM]: the destination side of a grid position — pixel index of its class-(0,0) output
                                              // << 2 | bit 0: the row below exists | bit 1: the column to the right exists; -1 = outside

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wrow = wave & 3, wcol = wave >> 2;  // row group (32 rows), first column tile
  const int h = lane >> 5, l31 = lane & 31;
  // BatchNorm groups (P.G > 1: `obs || next_obs` of one training step batched along n): tiles [g*tpg, (g+1)*tpg) cover group g's
  // own virtual grid, so a tile never mixes two groups — its statistics partial belongs to one group, its fused operand
  // uses one group's BatchNorm record — and the launch is exactly the union of the G per-group launches.
  const int tile = xcd_remap(blockIdx.x, ntiles);
  const int grp = (P.G > 1) ? tile / P.tpg : 0;
  const int q0 = (tile - grp * P.tpg) * TM;
  src += grp * P.src_gstride;
  dst += grp * P.dst_gstride;
  const OpFuse src_fuse = fuse_for_group(src_fuse_all, grp, grp * P.src_gstride);

  if (tid < TM) {
    const int q = q0 + tid;
    int ri = -1;
    if (q < P.total_q) {
      const GridPix g = grid_pix<false>(P, q, P.ds);
      if (g.y < P.Hd && g.x < P.Wd) ri = (((g.n * P.Hd + g.y) * P.Wd + g.x) << 2) | (g.y + 1 < P.Hd ? 1 : 0) | (g.x + 1 < P.Wd ? 2 : 0);
    }
    rowinfo[tid] = ri;
  }
  if constexpr (!BWD) rowtab_build(rowtab, tpa, P, q0 + P.min_off, TM + P.span);
  // coefficients of a fused operand, once per workgroup (visible after the first tap's barrier, which precedes the first staging)
  float* frec = (float*)(rowinfo + TM);  // [4][64]: scale, shift, c0, c1
  if (src_fuse.bnp && tid >= NT - 64) {
    const int c = tid - (NT - 64);
    const float sc = src_fuse.bnp[128 + c], sh = src_fuse.bnp[192 + c];
    float c0 = 0.f, c1 = 0.f;
    if (BWD && src_fuse.training) {
      c1 = sc * src_fuse.bnp[64 + c] * src_fuse.sums[64 + c] * src_fuse.inv_count;
      c0 = sc * src_fuse.sums[c] * src_fuse.inv_count - c1 * src_fuse.bnp[c];
    }
    frec[c] = sc; frec[64 + c] = sh; frec[128 + c] = c0; frec[192 + c] = c1;
  }
  const float* lrec = src_fuse.bnp ? frec : nullptr;

  f32x16 acc[NACC];
  float bcol[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) bcol[j] = bias ? bias[(wcol * NACC + j) * 32 + l31] : 0.f;

  int cur_src = -1, cur_dst = -1;
  bool pz_new = false;  // (PSUM == 2) a destination class opened at this tap: its pooled values are still to be requested

  // PSUM: the pooled value z = relu(gamma * xhat + beta), so where it is positive xhat = (z - beta) / gamma = z * pA + pB with
  // pA = invstd / scale, pB = -(shift / scale + mean) * invstd — one fused multiply-add per element, for this lane's four channels of
  // the flush layout (4 * (lane & 15) ..); channels with scale == 0 (pz_zero, pthr = +inf) are summed by the cold loop of the flush
  f32x4 pA = {0.f, 0.f, 0.f, 0.f}, pB = pA, pthr = pA;
  unsigned pz_zero = 0;
  const float* __restrict__ ppool = nullptr;
  if constexpr (PSUM) {
    const float* __restrict__ rec = ps.bnp + grp * 256 + (lane & 15) * 4;
    const f32x4 mean = *(const f32x4*)rec;
    const f32x4 pinv = *(const f32x4*)(rec + 64), psh = *(const f32x4*)(rec + 192);
    const f32x4 psc = *(const f32x4*)(rec + 128);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // |scale| tiny against |shift| (exactly 0 included): z - shift cancels — xhat = (z - shift) / scale ... would carry an error of
      // ~ eps * |shift| / |scale| — so such a channel takes the cold loop, which computes xhat from the convolution output itself
      const bool zero = fabsf(psc[e]) <= 1e-3f * fabsf(psh[e]) || psc[e] == 0.f;
      pz_zero |= (zero ? 1u : 0u) << e;
      pthr[e] = zero ? __builtin_inff() : 0.f;
      const float isc = zero ? 0.f : 1.f / psc[e];
      pA[e] = pinv[e] * isc;
      pB[e] = -(psh[e] * isc + mean[e]) * pinv[e];
    }
    ppool = ps.pooled + grp * P.dst_gstride;
  }

  // NW == 4: the accumulators leave through a 4 KB wave-private transposition buffer (this wave's part of the idle weight slab),
  // 16 tile rows at a time, so that every global store is a 16-byte one — lane (g = lane >> 4, slot = lane & 15) stores channels
  // [4*slot, 4*slot+4) of rows g, g+4, g+8, g+12 — instead of 32 dword-per-lane stores per flush (the dword path sustains ~5 B per
  // cycle and CU, which bounds the scatter programs: a ConvTranspose forward tile writes 128 KB).  The BatchNorm partials are taken
  // in the same layout (s4 / q4).  Rows 4..7 and 12..15 of the buffer hold their two 32-channel halves swapped, so that the lanes
  // h = 0 / 1 of one ds_write_b32 (rows 4 apart, same column) hit different banks.
  f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 pz[PSUM ? 8 : 1];  // PSUM: the pooled values of this lane's eight rows of a flush (rows 16*(hk >> 2) + (lane >> 4) + 4*(hk & 3))
  auto pz_request = [&](int d) {  // branch-free, clamped: a row outside the tensor reads pixel 0 and is never used
    const int need = d >> 1 | (d & 1) << 1;  // destination class (dy, dx): the rowinfo bits it needs
    const unsigned ddelta = (unsigned)((d >> 1) * P.Wd + (d & 1));
#pragma unroll
    for (int hk = 0; hk < 8; ++hk) {  // (the flush works the row's position out again: one LDS word and four instructions, against
      // nine registers for the whole tile in a kernel that has none to spare)
      const int row = wrow * 32 + 16 * (hk >> 2) + (lane >> 4) + 4 * (hk & 3);
      const int ri = rowinfo[row];
      const bool ok = ri >= 0 && (ri & need) == need;
      const unsigned pix = ok ? (unsigned)(ri >> 2) + ddelta : 0u;
      pz[PSUM ? hk : 0] = *(const f32x4*)(ppool + (size_t)pix * 64 + (lane & 15) * 4);
    }
  };
  auto flush16 = [&](int d) {
    if constexpr (PSUM == 0) {  // (the ablation switches belong to the plain kernel)
      if (P.dbg & 2) {
        if (acc[0][0] + acc[NACC - 1][5] == 123.456f) dst[tid] = acc[0][1];
        return;
      }
    }
    const int need = d >> 1 | (d & 1) << 1;
    const unsigned ddelta = (unsigned)((d >> 1) * P.Wd + (d & 1));
    float* S = Bs + wave * 1024;
    const int eg = lane >> 4, eslot = lane & 15;
    // The pooled values were requested before the first tap of this destination class (PSUM == 1: the tile's only one) and have
    // travelled under its MFMAs; they are waited for once, in straight-line code, before the first conditional store
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int rowl = (rr & 3) + 8 * (rr >> 2) + 4 * h;
        const int swz = (rowl & 4) << 3;  // 32 for rows 4..7, 12..15
#pragma unroll
        for (int j = 0; j < NACC; ++j) S[rowl * 64 + ((32 * j + l31) ^ swz)] = acc[j][8 * half + rr] + bcol[j];
      }
      // (wave-private: the compiler's lgkmcnt wait orders the writes above before the reads below)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rowl = eg + 4 * k;
        const int row = wrow * 32 + 16 * half + rowl;
        const f32x4 v = *(const f32x4*)(S + rowl * 64 + ((eslot ^ ((rowl & 4) << 1)) << 2));
        if constexpr (PSUM) {
          if (half == 0 && k == 0) {
#pragma unroll
            for (int hk = 0; hk < 8; ++hk) asm volatile("" : "+v"(pz[hk]));
          }
        }
        const int ri = rowinfo[row];
        const bool inside = ri >= 0 && (ri & need) == need;
        const size_t pixel = (unsigned)(ri >> 2) + ddelta;
        if (inside) {
          *(f32x4*)(dst + pixel * 64 + eslot * 4) = v;
          if constexpr (PSUM) {
            const f32x4 z = pz[half * 4 + k];
            f32x4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = __builtin_fmaf(z[e], pA[e], pB[e]);
            // (pthr = 0, or +inf for a channel whose scale is 0: those are summed by the cold loop behind the stores — a load inside THIS
            // loop's branches would put a full vmcnt wait behind every store)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float dz = z[e] > pthr[e] ? v[e] : 0.f;
              s4[e] += dz; q4[e] += dz * xh[e];
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { s4[e] += v[e]; q4[e] += v[e] * v[e]; }
          }
        }
      }
    }
    if constexpr (PSUM != 0) {
      if (pz_zero) {
        // BatchNorm scale (almost) 0 in one of this lane's channels — exactly 0: relu(bn(.)) is the constant max(shift, 0), every
        // window's first position is the argmax — xhat cannot be recovered from the pooled value: it is taken from the convolution
        // output under the recorded argmax, and the ReLU decision is the forward's own expression on that output.  Rare and slow on
        // purpose: d(pooled) is read back from where this lane has just stored it.
        const float* __restrict__ rec = ps.bnp + grp * 256 + eslot * 4;  // (the cold loop re-reads what it needs of the record)
        const f32x4 mean = *(const f32x4*)rec, pinv = *(const f32x4*)(rec + 64), psc = *(const f32x4*)(rec + 128),
                    psh = *(const f32x4*)(rec + 192);
#pragma unroll 1
        for (int hk = 0; hk < 8; ++hk) {
          const int ri = rowinfo[wrow * 32 + 16 * (hk >> 2) + eg + 4 * (hk & 3)];
          if (!(ri >= 0 && (ri & need) == need)) continue;
          const size_t pixel = (unsigned)(ri >> 2) + ddelta;  // (n * Hd + y) * Wd + x of the output this lane stored
          const int n = (int)pixel / (P.Hd * P.Wd);
          const int y = ((int)pixel - n * P.Hd * P.Wd) / P.Wd, x = (int)pixel - (n * P.Hd + y) * P.Wd;
          const uint32_t packed = *(const uint32_t*)(ps.argmax + (size_t)grp * P.dst_gstride + pixel * 64 + eslot * 4);
          const f32x4 v = *(const f32x4*)(dst + pixel * 64 + eslot * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if ((pz_zero >> e) & 1u) {
              const int a = (packed >> (8 * e)) & 0xff;
              const int iy = y * 2 - ps.pad + a / 3, ix = x * 2 - ps.pad + a % 3;
              const float vy = ps.y[grp * ps.y_gstride + ((size_t)(n * ps.H + iy) * ps.W + ix) * 64 + eslot * 4 + e];
              const float dz = vy * psc[e] + psh[e] > 0.f ? v[e] : 0.f;
              s4[e] += dz; q4[e] += dz * ((vy - mean[e]) * pinv[e]);
            }
        }
      }
    }
  };

  // The weight slab of tap t+1 is fetched into registers while tap t's MFMAs run, and written to LDS between the two
  // barriers of the next iteration: the L2 latency of the slab never sits between barriers.
  // Wave w moves the contiguous part [w, w+1) * 16 KB / NW of the slab (and nobody else's): between the barrier that ends a tap and
  // its own slab write a wave may therefore use that part of Bs as private scratch (flush16).
  constexpr int BV = 1024 / NT;  // 16-byte vectors of the 16 KB slab per thread
  const int bslot = wave * (BV * 64) + lane;
  f32x4 breg[BV];
  {
    const f32x4* wsrc = (const f32x4*)(wpack + (size_t)P.tw[0] * 4096);
#pragma unroll
    for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot + i * 64];
  }
  // The per-tap program words travel two taps ahead of their use (w0 = this tap, w1 = the next one, whose slab is requested
  // right after this tap's second barrier): fetched at their point of use, each costs a scalar-memory round trip in front of the
  // slab requests / the first LDS reads of every tap.
  int w0 = P.tp[0], w1 = P.tp[1];
  if constexpr (PSUM == 1) {  // the tile's one flush is known now: its pooled values travel under the whole tile
    __syncthreads();          // (rowinfo)
    pz_request(P.tdst[0]);
  }
  // Three taps per trip of the loop (the plain kernels; hipcc chose this by itself while the body was larger): 20 KB of code instead of
  // 50 KB unrolled nine times — the instruction cache is 64 KB for two CUs.  (Everything tap-dependent comes from the program words.)
  constexpr int TAP_UNROLL = BWD ? NTAPS : 3;
#pragma unroll TAP_UNROLL
  for (int ti = 0; ti < NTAPS; ++ti) {
    const int w2 = P.tp[ti + 2];
    const int tsrc = (w0 >> 20) & 3, tdst = (w0 >> 22) & 3;
    __syncthreads();  // all waves are done with the previous tap's Bs (and with As if it is about to be replaced)
    if (tdst != cur_dst) {
      if (cur_dst >= 0) flush16(cur_dst);
#pragma unroll
      for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      if constexpr (PSUM == 2) pz_new = true;
      cur_dst = tdst;
    }
    if (tsrc != cur_src) {
      if (!(P.dbg & 1)) {
        if (BWD)
          stage_rows<true, (NW == 4 ? BATCH_BWD : 2), NT, true>(As, src, P.Hs, P.Ws, P.ss, tsrc, P.PW, P.PH, P.total_q,
                                                        q0 + P.min_off, TM + P.span, src_fuse, -P.min_off, TM, 64, 0, lrec);
        else
          stage_rows_tab<BATCH_FWD>(As, src, rowtab, tpa, tsrc, P.Ws, TM + P.span, lrec);
      }
      cur_src = tsrc;
    }
    {
      f32x4* wdst = (f32x4*)Bs;
#pragma unroll
      for (int i = 0; i < BV; ++i) wdst[bslot + i * 64] = breg[i];
    }
    if constexpr (PSUM == 2) {
      // Several destination classes: the pooled values of the class that opens at this tap, for the flush that will close it.
      // Requested inside that flush they were one exposed HBM round trip per class and tile; requested here — BEHIND the slab write,
      // whose wait for the slab registers would otherwise wait for these younger loads too — they travel under the class's MFMAs.
      if (pz_new) { pz_request(cur_dst); pz_new = false; }
    }
    __syncthreads();
    if (BWD ? ti + 1 < NTAPS : true) {  // (never a run-time condition: behind the join of a branch with loads in it hipcc waits for
      // everything at the next re-use of their registers — in the flush that was one full wait per store.  The plain kernels, whose
      // loop is not unrolled nine times, therefore request a slab behind the last tap as well: word NTAPS of the program is 0 = slab 0)
      const f32x4* wsrc = (const f32x4*)(wpack + (size_t)((w1 >> 16) & 15) * 4096);
#pragma unroll
      for (int i = 0; i < BV; ++i) breg[i] = wsrc[bslot + i * 64];
    }
    __builtin_amdgcn_sched_barrier(0);  // the slab requests go out HERE, ahead of the tap's MFMAs (the scheduler sinks them otherwise)
    const int R = wrow * 32 + l31 + (int)(short)(w0 & 0xffff) - P.min_off;
    // offset of this lane's first 16-byte slot of row R; slot (2kc + h) ^ (R & 15) of the swizzled row is that offset XOR
    // (kc << 5) bytes — R*256 has no bits below 8, 2kc + h = 2kc ^ h — so each k-chunk costs ONE v_xor with a literal
    int abase = (R * 64 + ((h ^ (R & 15)) << 2)) * 4;  // in BYTES (the XOR then is the whole address computation)
    asm volatile("" : "+v"(abase));                     // one opaque value: the compiler otherwise re-splits it into its parts
    const float* brow = Bs + (wcol * NACC * 32 + l31) * 64;  // column tile j is 32 rows (2048 floats) further
    const int bkey = lane & 15;
    f32x4 a = *(const f32x4*)((const char*)As + abase);
    f32x4 b[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) b[j] = *(const f32x4*)(brow + j * 2048 + ((h ^ bkey) << 2));
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) {
      f32x4 an = a, bn[NACC];
#pragma unroll
      for (int j = 0; j < NACC; ++j) bn[j] = b[j];
      if (kc < 7) {
        const int slot = (kc + 1) * 2 + h;
        an = *(const f32x4*)((const char*)As + (abase ^ ((kc + 1) << 5)));
#pragma unroll
        for (int j = 0; j < NACC; ++j) bn[j] = *(const f32x4*)(brow + j * 2048 + ((slot ^ bkey) << 2));
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ahead of this chunk's MFMAs (hipcc sinks them otherwise)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[j][r], acc[j], 0, 0, 0);
      a = an;
#pragma unroll
      for (int j = 0; j < NACC; ++j) b[j] = bn[j];
    }
    w0 = w1; w1 = w2;
  }
  __syncthreads();  // every wave is done with the last tap's slab: Bs becomes scratch
  flush16(cur_dst);

  if (stats_partial && !(P.dbg & 2)) {
    // the 4 row groups g of a wave hold the same columns; then the 4 row groups of waves are combined through LDS
    __syncthreads();
    float* red = Bs;  // [4 row groups][128]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s4[e] += __shfl_xor(s4[e], 16, 64); s4[e] += __shfl_xor(s4[e], 32, 64);
      q4[e] += __shfl_xor(q4[e], 16, 64); q4[e] += __shfl_xor(q4[e], 32, 64);
    }
    if (lane < 16) {
      *(f32x4*)(red + wrow * 128 + lane * 4) = s4;
      *(f32x4*)(red + wrow * 128 + 64 + lane * 4) = q4;
    }
    __syncthreads();
    if (tid < 128) {
      const float v = red[tid] + red[128 + tid] + red[256 + tid] + red[384 + tid];
      stats_partial[(size_t)tile * 128 + tid] = v;  // [0,64): sum, [64,128): sum of squares
    }
  }
}

template <int NW, bool BWD = false>
__global__ __launch_bounds__(NW * 64, NW / 2) void conv64_fwd_kernel(const float* __restrict__ src,
                                                                    const float* __restrict__ wpack,
                                                                    const float* __restrict__ bias,
                                                                    float* __restrict__ dst,
                                                                    float* __restrict__ stats_partial,
                                                                    const ConvProg P, int ntiles, const OpFuse src_fuse_all) {
  conv64_fwd_body<NW, BWD, 0>(src, wpack, bias, dst, stats_partial, P, ntiles, src_fuse_all, SRLZ_NO_POOLSUM);
}

// The data gradient of a convolution whose input was a pooled map, with the pooled block's BatchNorm-backward sums in its epilogue
// (PoolSum; PSUM = 1: one destination class, 2: several).
template <int PSUM>
__global__ __launch_bounds__(256, 2) void conv64_dgrad_poolsum_kernel(const float* __restrict__ src,
                                                                     const float* __restrict__ wpack,
                                                                     float* __restrict__ dst,
                                                                     float* __restrict__ bn_bwd_partial, const ConvProg P,
                                                                     int ntiles, const PoolSum ps) {
  conv64_fwd_body<4, false, PSUM>(src, wpack, nullptr, dst, bn_bwd_partial, P, ntiles, SRLZ_NO_FUSE, ps);
}

// w_ref -> packed [tap][n_out][slot ^ (n_out&15)][4]; fwd: (n=co,k=ci), bwd: (n=ci,k=co)
__global__ void conv64_pack_kernel(const float* __restrict__ w_ref, float* __restrict__ pf, float* __restrict__ pb,
                                   int transposed) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= NTAPS * 4096) return;
  const int tap = id >> 12, n = (id >> 6) & 63, k = id & 63;
  const int o = (tap * 64 + n) * 64 + ((((k >> 2) ^ (n & 15)) << 2) | (k & 3));
  // reference element [A][B][tap]: conv A=co,B=ci ; convT A=ci,B=co
  const int fwd_idx = transposed ? ((k * 64 + n) * 9 + tap) : ((n * 64 + k) * 9 + tap);
  const int bwd_idx = transposed ? ((n * 64 + k) * 9 + tap) : ((k * 64 + n) * 9 + tap);
  if (pf) pf[o] = w_ref[fwd_idx];
  if (pb) pb[o] = w_ref[bwd_idx];
}

static int check_desc(const srlz_conv64_desc* d) {
  SRLZ_REQUIRE(d != nullptr, SRLZ_ERR_NULL, "conv64: null descriptor");
  SRLZ_REQUIRE(d->ksize == 3 && (d->stride == 1 || d->stride == 2) && d->n > 0, SRLZ_ERR_BAD_DESC,
               "conv64: only 3x3 stride 1/2 supported (k=%d s=%d)", d->ksize, d->stride);
  SRLZ_REQUIRE(d->groups >= 0 && (d->groups <= 1 || d->n % d->groups == 0), SRLZ_ERR_BAD_DESC,
               "conv64: n = %d is not a multiple of groups = %d", d->n, d->groups);
  int eho, ewo;
  if (!d->transposed) {
    eho = (d->hi + 2 * d->pad - 3) / d->stride + 1;
    ewo = (d->wi + 2 * d->pad - 3) / d->stride + 1;
  } else {
    eho = (d->hi - 1) * d->stride - 2 * d->pad + 3;
    ewo = (d->wi - 1) * d->stride - 2 * d->pad + 3;
  }
  SRLZ_REQUIRE(eho == d->ho && ewo == d->wo, SRLZ_ERR_BAD_DESC, "conv64: output size %dx%d inconsistent (expected %dx%d)",
               d->ho, d->wo, eho, ewo);
  return 0;
}

static size_t fwd_lds_bytes(const ConvProg& P) {  // source rows, slab, row table, rowinfo, fused-operand coefficients
  return (size_t)(TM + P.span) * 256 + 16384 + (size_t)64 * rowtab_passes(TM + P.span) + TM * 4 + 256 * 4;
}

static int launch_fwd(const float* src, const float* wpack, const float* bias, float* dst, float* stats,
                      const ConvProg& P, hipStream_t st, const OpFuse src_fuse = SRLZ_NO_FUSE, const PoolSum* psum = nullptr,
                      bool forward = false) {
  const int ntiles = P.G * P.tpg;
  const size_t lds = fwd_lds_bytes(P);
  SRLZ_REQUIRE(lds <= 160 * 1024, SRLZ_ERR_BAD_DESC, "conv64: tile needs %zu bytes of LDS", lds);
  // the row table keeps pixel indices in 28 bits and the staging 32-bit float offsets; the fast divisions take dividends below 2^31
  SRLZ_REQUIRE(fits_32bit_src_floats(P) && fits_32bit_dst_rowinfo(P) && fits_31bit_grid(P, TM + P.span), SRLZ_ERR_BAD_DESC, "conv64: a group of %d images of %d x %d -> %d x %d is beyond the tile tables' 32-bit offsets", P.N, P.Hs,
               P.Ws, P.Hd, P.Wd);
  if (psum) {  // data gradient whose epilogue takes the pooled block's BatchNorm-backward sums (its own instantiation)
    SRLZ_REQUIRE(!src_fuse.y && !src_fuse.bnp && stats && !bias, SRLZ_ERR_BAD_DESC, "conv64: the pooled-block epilogue takes a plain operand");
    bool one_class = true;
    for (int t = 1; t < NTAPS; ++t) one_class = one_class && P.tdst[t] == P.tdst[0];
    if (one_class) {
      SRLZ_MAX_LDS(conv64_dgrad_poolsum_kernel<1>, lds);
      SRLZ_LAUNCH(conv64_dgrad_poolsum_kernel<1>, dim3(ntiles), dim3(256), lds, st, src, wpack, dst, stats, P, ntiles, *psum);
    } else {
      SRLZ_MAX_LDS(conv64_dgrad_poolsum_kernel<2>, lds);
      SRLZ_LAUNCH(conv64_dgrad_poolsum_kernel<2>, dim3(ntiles), dim3(256), lds, st, src, wpack, dst, stats, P, ntiles, *psum);
    }
    return 0;
  }
  // 4 waves (32x64 per wave); 8 waves of 32x32 were measured within +-3 % (the kernel is bound by the power-limited matrix
  // rate, not by latency hiding) and are not instantiated any more
#define SRLZ_FWD_LAUNCH(NWV, BWDV)                                                                                          \
  do {                                                                                                                     \
    SRLZ_MAX_LDS((conv64_fwd_kernel<NWV, BWDV>), lds);                                                                      \
    SRLZ_LAUNCH((conv64_fwd_kernel<NWV, BWDV>), dim3(ntiles), dim3(NWV * 64), lds, st, src, wpack, bias, dst, stats,        \
                P, ntiles, src_fuse);                                                                                      \
  } while (0)
  if (src_fuse.y) {
    SRLZ_REQUIRE(fits_32bit_src_floats(P), SRLZ_ERR_BAD_DESC,
                 "conv64: a group's operand has %lld floats (the fused staging keeps 32-bit row offsets)", (long long)P.N * P.Hs * P.Ws * 64);
    // (a fused BatchNorm-backward operand that must also be STORED for a separate weight-gradient launch: the shapes
    // conv64_bwd_fused_kernel does not take — fewer than 8 tiles, a low-resolution grid wider than 63)
    SRLZ_FWD_LAUNCH(4, true);
  } else {
    // plain stride-2 gather programs with many tiles (conv3 forward at training batch sizes): the software-pipelined persistent
    // kernel (gather_pipe_ok: a per-group criterion, so that one BatchNorm group alone and the batched pair take the same kernel)
    if (!src_fuse.bnp && !bias && conv64::gather_pipe_ok(P)) return conv64::launch_gather_pipe(src, wpack, dst, stats, P, st);
    // a stride-2 ConvTranspose's forward with many tiles: the pipelined persistent kernel of the scatter programs, bit-identical to
    // conv64_fwd_kernel<4, false> in y and in the statistics (scatter_pipe_ok: per group as well)
    if (forward && conv64::scatter_pipe_ok(P)) return conv64::launch_scatter_pipe(src, wpack, bias, dst, stats, src_fuse.bnp, P, st);
    SRLZ_FWD_LAUNCH(4, false);
  }
#undef SRLZ_FWD_LAUNCH
  return 0;
}

}  // namespace

// What every entry point that takes a descriptor begins with: check_desc, then the descriptor's forward or data-gradient program
int conv64::with_program(const srlz_conv64_desc* d, int backward_data, Prog* P) {
  if (int rc = check_desc(d)) return rc;
  const int G = d->groups > 1 ? d->groups : 1;
  const int rc = backward_data ? build_program(P, d->transposed, d->stride, d->pad, d->n, d->ho, d->wo, d->hi, d->wi, G)
                               : build_program(P, !d->transposed, d->stride, d->pad, d->n, d->hi, d->wi, d->ho, d->wo, G);
  SRLZ_REQUIRE(rc == 0, SRLZ_ERR_BAD_DESC, "conv64: cannot build a grid program for this descriptor");
  return 0;
}

extern "C" size_t srlz_conv64_packed_floats(void) { return (size_t)NTAPS * 4096; }

extern "C" int srlz_conv64_pack_weights(const float* w_ref, float* wpack_fwd, float* wpack_bwd,
                                        const srlz_conv64_desc* d, srlz_stream_t stream) {
  if (int rc = check_desc(d)) return rc;
  SRLZ_REQUIRE(w_ref, SRLZ_ERR_NULL, "conv64_pack: null weights");
  SRLZ_LAUNCH(conv64_pack_kernel, dim3((NTAPS * 4096 + 255) / 256), dim3(256), 0, as_stream(stream), w_ref, wpack_fwd, wpack_bwd,
              d->transposed);
  return 0;
}

extern "C" int srlz_conv64_fwd_tiles(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 0, &P)) return -1;
  return P.G * P.tpg;
}

extern "C" int srlz_conv64_fwd(const float* x, const float* wpack_fwd, const float* bias, float* y,
                               float* stats_partial, const float* x_bnp, const srlz_conv64_desc* d,
                               srlz_stream_t stream) {
  ConvProg P;
  if (int rc = conv64::with_program(d, 0, &P)) return rc;
  SRLZ_REQUIRE(x && wpack_fwd && y, SRLZ_ERR_NULL, "conv64_fwd: null pointer");
  return launch_fwd(x, wpack_fwd, bias, y, stats_partial, P, as_stream(stream), OpFuse{x_bnp, nullptr, nullptr, 0.f, 0, nullptr}, nullptr,
                    true);
}

extern "C" int srlz_conv64_bwd_data(const float* dy, const float* wpack_bwd, float* dx, const srlz_bn_bwd_operand* dy_bn,
                                    const srlz_conv64_desc* d, srlz_stream_t stream) {
  ConvProg P;
  if (int rc = conv64::with_program(d, 1, &P)) return rc;
  SRLZ_REQUIRE(dy && wpack_bwd && dx, SRLZ_ERR_NULL, "conv64_bwd_data: null pointer");
  OpFuse gf;
  if (int rc = make_bwd_fuse(&gf, dy_bn, "conv64_bwd_data")) return rc;
  return launch_fwd(dy, wpack_bwd, nullptr, dx, nullptr, P, as_stream(stream), gf);
}

extern "C" int srlz_conv64_bwd_data_tiles(const srlz_conv64_desc* d) {
  ConvProg P;
  if (conv64::with_program(d, 1, &P)) return -1;
  return P.G * P.tpg;
}

extern "C" int srlz_conv64_bwd_data_pool_sums(const float* dy, const float* wpack_bwd, float* dx, const float* pooled,
                                              const float* pool_bnp, const float* pool_y, const uint8_t* pool_argmax,
                                              const srlz_pool_desc* pd, float* bn_bwd_partial, const srlz_conv64_desc* d,
                                              srlz_stream_t stream) {
  ConvProg P;
  if (int rc = conv64::with_program(d, 1, &P)) return rc;
  SRLZ_REQUIRE(dy && wpack_bwd && dx && pooled && pool_bnp && pool_y && pool_argmax && pd && bn_bwd_partial, SRLZ_ERR_NULL,
               "conv64_bwd_data_pool_sums: null pointer");
  // dx (this layer's input gradient) is the gradient of the pooled map pd describes: same images, same spatial size, NHWC
  SRLZ_REQUIRE(pd->n == d->n && pd->hp == d->hi && pd->wp == d->wi && !pd->out_nchw &&
               (pd->groups > 1 ? pd->groups : 1) == (d->groups > 1 ? d->groups : 1), SRLZ_ERR_BAD_DESC,
               "conv64_bwd_data_pool_sums: the pooled map [%d,%d,%d] is not this layer's input [%d,%d,%d]", pd->n, pd->hp, pd->wp, d->n,
               d->hi, d->wi);
  const int G = d->groups > 1 ? d->groups : 1;
  PoolSum ps = {pooled, pool_bnp, pool_y, pool_argmax, (long long)(pd->n / G) * pd->h * pd->w * 64, pd->h, pd->w, pd->pool_pad};
  return launch_fwd(dy, wpack_bwd, nullptr, dx, bn_bwd_partial, P, as_stream(stream), SRLZ_NO_FUSE, &ps);
}

// Debug/test hook (host only, no GPU needed): dump the grid program so tests can interpret it on the CPU.
// out[0..]: N,PH,PW,ss,Hs,Ws,ds,Hd,Wd,min_off,span,s2, then 9 x {src,dst,off,w}.  Returns number of ints or <0.
extern "C" int srlz_conv64_debug_program(const srlz_conv64_desc* d, int backward_data, int* out, int cap) {
  ConvProg P;
  if (int rc = conv64::with_program(d, backward_data, &P)) return rc;
  if (cap < 12 + 4 * NTAPS) return SRLZ_ERR_WORKSPACE;
  int i = 0;
  out[i++] = P.N; out[i++] = P.PH; out[i++] = P.PW; out[i++] = P.ss; out[i++] = P.Hs; out[i++] = P.Ws;
  out[i++] = P.ds; out[i++] = P.Hd; out[i++] = P.Wd; out[i++] = P.min_off; out[i++] = P.span; out[i++] = P.s2;
  for (int t = 0; t < NTAPS; ++t) { out[i++] = P.tsrc[t]; out[i++] = P.tdst[t]; out[i++] = P.toff[t]; out[i++] = P.tw[t]; }
  return i;
}
