/*
 * srlz.h — C ABI of libsrlz_hip.so: the MI355X (gfx950) kernels behind srl-zoo's image-representation
 * training hot path.
 *
 * The reference (araffin/srl-zoo, /root/reference) has NO native code: every op below is reached there through
 * PyTorch (torch.nn / autograd / torch.optim).  Each entry point therefore cites the reference call site whose
 * arithmetic it replaces (file:line into /root/reference).  The Python binding a maintainer adds is a ctypes stub
 * (see INTEGRATION.md); this build's own is srl-zoo_amd/srlz/_cabi.py.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless the name ends in _host.
 *   - all floating point data is fp32 (only srlz_knn_f64, the evaluation search, srlz_gtc_rows_f64, the ground-truth correlation, and srlz_pca_*, the PCA baseline, take fp64; srlz_reward_probe_* return their loss sums in fp64); activations are NHWC ([N][H][W][C], C fastest) unless stated NCHW.
 *     The reference's tensors are NCHW ([B,C,D1,D2]; D1/D2 are the image's W/H because the loader transposes,
 *     preprocessing/data_loader.py:255); the NCHW<->NHWC change happens INSIDE conv1 (reads NCHW) and the last
 *     ConvTranspose (writes NCHW), so callers only ever hand over / receive reference-layout images.
 *   - parameters cross the ABI in the reference's state_dict layouts (Conv2d [Cout,Cin,kh,kw],
 *     ConvTranspose2d [Cin,Cout,kh,kw], Linear [out,in]); *_pack_* entry points build the kernels' private copies.
 *   - the caller owns all memory (weights, activations, workspaces); nothing is allocated, freed or retained.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises.
 *   - return 0 on success, a negative srlz_status otherwise; srlz_last_error() gives the text (thread-local).
 */
#ifndef SRLZ_H
#define SRLZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* srlz_stream_t; /* hipStream_t */

enum srlz_status {
  SRLZ_OK = 0,
  SRLZ_ERR_BAD_DESC = -1,   /* unsupported shape / inconsistent descriptor */
  SRLZ_ERR_WORKSPACE = -2,  /* workspace too small */
  SRLZ_ERR_HIP = -3,        /* a HIP runtime call failed (text in srlz_last_error) */
  SRLZ_ERR_NULL = -4        /* required pointer is NULL */
};

/* ABI version: bumped whenever an existing entry point changes its signature or the meaning / size of a buffer it fills, so that a
 * binding built against an older header fails at load time instead of passing a pointer where a float is expected (a binding
 * compares srlz_version() with the SRLZ_ABI_VERSION it was written for; srl-zoo_amd/srlz/_cabi.py does).
 * 101 (round 4): srlz_convT_out_bwd_fused carries three gain arguments (added in round 3 without a bump); its partial records and
 *                workspace follow the strip geometry of csrc/convt_out.hip; srlz_convT_out_fwd_loss_workgroups counts those strips'
 *                workgroups. */
#define SRLZ_ABI_VERSION 104
int srlz_version(void);
const char* srlz_last_error(void);
/* Number of CUs of the current device (used by callers to size persistent grids / workspaces). */
int srlz_device_cus(void);

/* ------------------------------------------------------------------------------------------------------------
 * 64 -> 64 channel convolutions (3x3, stride 1 or 2): fp32 MFMA implicit GEMM.
 * Replaces nn.Conv2d / nn.ConvTranspose2d forward + autograd backward for
 *   conv3x3 s1 p1      models/models.py:54,217-226      conv3x3 s2 p1   models/models.py:59
 *   ConvTranspose2d(64,64,3,stride=2) x4               models/models.py:66,70,74,78
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  int n;          /* images */
  int hi, wi;     /* forward-input spatial size  (NHWC, 64 channels) */
  int ho, wo;     /* forward-output spatial size (NHWC, 64 channels) */
  int ksize;      /* 3 */
  int stride;     /* 1 or 2 */
  int pad;        /* conv: zero padding; convT: `padding` argument */
  int transposed; /* 0 = nn.Conv2d, 1 = nn.ConvTranspose2d */
  int groups;     /* BatchNorm groups batched along n (0 / 1 = one): images [g*n/groups, (g+1)*n/groups) are group g, i.e. the
                     launch is the union of `groups` independent model calls — `obs || next_obs` of one training step,
                     models/learner.py:392-393.  Every BatchNorm record argument (x_bnp, bnp, sums) then holds `groups`
                     consecutive records, statistics partials come group after group (tiles never straddle two groups),
                     weight gradients are summed over all groups. */
} srlz_conv64_desc;

/* floats needed for one packed weight copy (9 taps x 64 x 64) */
size_t srlz_conv64_packed_floats(void);
/* w_ref (reference layout) -> wpack_fwd (forward / weight-grad operand) and wpack_bwd (data-grad operand). */
int srlz_conv64_pack_weights(const float* w_ref, float* wpack_fwd, float* wpack_bwd,
                             const srlz_conv64_desc* d, srlz_stream_t stream);
/* number of per-tile BatchNorm partial records forward() writes (each record = 128 floats: sum[64], sumsq[64]) */
int srlz_conv64_fwd_tiles(const srlz_conv64_desc* d);
/* y = conv(x) (+bias).  bias may be NULL.  stats_partial may be NULL; otherwise receives
 * srlz_conv64_fwd_tiles(d) x 128 floats of per-tile sum / sum-of-squares per channel over y (BatchNorm input).
 * x_bnp (may be NULL): x is the RAW output of the previous convolution and the layer input is relu(batchnorm(x)) with
 * this 4x64 record (srlz_bn_finalize / srlz_bn_eval_params) — nn.BatchNorm2d + nn.ReLU of models/models.py:67-80 fused
 * into the operand load, so the activated tensor is never written to memory. */
int srlz_conv64_fwd(const float* x, const float* wpack_fwd, const float* bias, float* y, float* stats_partial,
                    const float* x_bnp, const srlz_conv64_desc* d, srlz_stream_t stream);
/* Fused BatchNorm + ReLU BACKWARD operand.  Wherever a `dy` argument is followed by a `const srlz_bn_bwd_operand* dy_bn`,
 * a non-NULL record means: the convolution whose gradient is being taken was followed by BatchNorm2d + ReLU
 * (models/models.py:67-80), `dy` actually holds dA = d(loss)/d(relu(bn(y))), and the kernel rebuilds
 *   d(loss)/dy = scale * ( dA*[bn(y)>0] - sums[c]/count - xhat*sums[64+c]/count )      (training; eval: scale*dA*[..])
 * while loading its operand, so d(loss)/dy is never written to memory.  y = the raw convolution output (same shape as
 * dA), bnp = its 4x64 BatchNorm record, sums = output of srlz_bn_relu_bwd_sums, count = N*H*W of y.
 * dy_out (srlz_conv64_bwd_data only, may be NULL): the rebuilt d(loss)/dy is also stored there, every element exactly
 * once, as a by-product of the operand staging — the weight-gradient kernel then reads it as a plain dy. */
typedef struct {
  const float* y;
  const float* bnp;
  const float* sums;
  long long count;   /* N*H*W of y PER GROUP */
  int training;
  float* dy_out;
} srlz_bn_bwd_operand; /* with srlz_conv64_desc.groups > 1: bnp / sums hold one record per group */
/* dx = d(loss)/d(x) from dy (dy_bn may be NULL: dy is then the plain gradient). */
int srlz_conv64_bwd_data(const float* dy, const float* wpack_bwd, float* dx, const srlz_bn_bwd_operand* dy_bn,
                         const srlz_conv64_desc* d, srlz_stream_t stream);
/* The same data gradient for a layer whose INPUT was a pooled map — conv3x3 after BatchNorm2d + ReLU + MaxPool2d(3, 2)
 * (models/models.py:50-54, 55-59) — with the BatchNorm-backward sums of that pooled block taken in the epilogue: dx is d(loss)/d(pooled),
 * and the tile that writes it also reads `pooled` (same shape) and leaves, per tile,  bn_bwd_partial[tile][0..64) = sum dz,
 * [64..128) = sum dz * xhat  with dz = dx where pooled > 0 (the gradient of max-pool + ReLU lives at the argmax, where the pooled value
 * is relu(bn(y)): xhat follows from it; pool_y / pool_argmax are read only for channels whose BatchNorm scale is exactly 0).
 * srlz_bn_bwd_finalize_partials turns the srlz_conv64_bwd_data_tiles(d) records into sums / dgamma / dbeta: the separate pass of
 * srlz_bn_relu_pool_bwd_sums over (d pooled, pooled, argmax) disappears.  pd describes the pooling that produced `pooled`. */
struct srlz_pool_desc_s;
int srlz_conv64_bwd_data_tiles(const srlz_conv64_desc* d);
int srlz_conv64_bwd_data_pool_sums(const float* dy, const float* wpack_bwd, float* dx, const float* pooled, const float* pool_bnp,
                                   const float* pool_y, const uint8_t* pool_argmax, const struct srlz_pool_desc_s* pd,
                                   float* bn_bwd_partial, const srlz_conv64_desc* d, srlz_stream_t stream);
/* The WHOLE backward of a decoder block's ConvTranspose2d(64, 64, 3, stride 2) + BatchNorm2d + ReLU (models/models.py:70-80, as
 * autograd runs it for loss.backward(), models/learner.py:489) in ONE launch: srlz_conv64_bwd_data(dy, dy_bn) and
 * srlz_conv64_bwd_weight(x, dy_out, x_bnp) on a single staging of the rebuilt d(loss)/dy, which therefore never touches memory
 * (dy_bn->dy_out must be NULL).  x = the RAW input tensor of the layer, x_bnp its BatchNorm record(s) (the layer's input is
 * relu(batchnorm(x)); required), dy / dy_bn as in srlz_conv64_bwd_data (dy_bn required).  dx is bit-identical to
 * srlz_conv64_bwd_data's; dw_ref / dbias are deterministic (per-workgroup partials in `ws`, fixed-order fp64 second stage).
 * Only where srlz_conv64_bwd_fused_supported(d) != 0 (stride-2 transposed layers with at least 8 tiles; groups <= 2). */
int srlz_conv64_bwd_fused_supported(const srlz_conv64_desc* d);
/* != 0: srlz_conv64_fwd (backward_data = 0) / srlz_conv64_bwd_data (1) of this layer with a plain operand and no bias run as
 * conv64_gather_pipe_kernel — the software-pipelined persistent kernel of the stride-2 gather programs (conv3's forward,
 * /root/reference/models/models.py:59, and the first ConvTranspose's data gradient) — rather than conv64_fwd_kernel: what a profile
 * will list the launch under. */
int srlz_conv64_gather_pipe_supported(const srlz_conv64_desc* d, int backward_data);
/* != 0: srlz_conv64_fwd of this layer (backward_data = 0; a data gradient never does) — with or without bias, plain operand or x_bnp —
 * runs as conv64_scatter_pipe_kernel, the software-pipelined persistent kernel of the stride-2 scatter programs (the forward of
 * ConvTranspose2d(64, 64, 3, stride 2), reference models/models.py:66-78), rather than conv64_fwd_kernel.  y and stats_partial
 * are bit-identical between the two.  Host only: no launch. */
int srlz_conv64_scatter_pipe_supported(const srlz_conv64_desc* d, int backward_data);
size_t srlz_conv64_bwd_fused_workspace(const srlz_conv64_desc* d);
/* x_bn_bwd_partial (may be NULL; round 6): dx of this call is dA of the BatchNorm + ReLU that produced the layer's input from x —
 * the previous decoder block's (models/models.py:67-77) — and the tile that writes it holds relu(bn(x)) of the same positions, so the
 * launch also leaves that layer's two BatchNorm-backward sums,  sum dA*[bn(x)>0]  and  sum dA*[bn(x)>0]*xhat,  as
 * srlz_conv64_bwd_fused_bn_rows(d) partial records of 128 floats ([groups][rows / groups][128]) for srlz_bn_bwd_finalize_partials:
 * srlz_bn_relu_bwd_sums' separate pass over (x, dx) disappears.  (Channels whose BatchNorm scale is (almost) 0 are summed from x
 * itself by a companion launch inside this call — normally a ~4 us no-op.) */
int srlz_conv64_bwd_fused_bn_rows(const srlz_conv64_desc* d);
/* Host only: the persistent workgroups of srlz_conv64_bwd_fused (one per CU, a multiple of 8), which walk the
 * srlz_conv64_bwd_data_tiles(d) tiles; its workspace holds one weight-gradient partial per workgroup. */
int srlz_conv64_bwd_fused_workgroups(const srlz_conv64_desc* d);
int srlz_conv64_bwd_fused(const float* x, const float* x_bnp, const float* dy, const srlz_bn_bwd_operand* dy_bn,
                          const float* wpack_bwd, float* dx, float* dw_ref, float* dbias /* may be NULL */,
                          float* x_bn_bwd_partial /* may be NULL */, void* ws, size_t ws_bytes, const srlz_conv64_desc* d,
                          srlz_stream_t stream);
/* ---- conv3x3 stride 1 pad 1 (conv2 of the encoder, models/models.py:54) as Winograd F(2x2, 3x3) on the fp32 matrix cores (round 6;
 * csrc/wino.hip): 16 multiplications per (ci, co) and 2x2 output patch instead of 36 — what cuDNN, the reference's backend, runs for
 * this layer.  Products and accumulation stay fp32; outputs differ from the direct fp32 chain by a few 1e-7 of the output scale and do
 * not depend on how images are batched or grouped.  srlz_conv64_wino_supported: non-transposed, stride 1, pad 1, even sizes.
 * upack_* = srlz_conv64_wino_packed_floats() floats each (G g G^T in the kernel's layout; fwd for srlz_conv64_wino_fwd, bwd for
 * srlz_conv64_wino_bwd_data*; either may be NULL).  stats_partial: srlz_conv64_wino_tiles(d) records of 128 floats, group after group. */
int srlz_conv64_wino_supported(const srlz_conv64_desc* d);
size_t srlz_conv64_wino_packed_floats(void);
int srlz_conv64_wino_pack_weights(const float* w_ref, float* upack_fwd, float* upack_bwd, srlz_stream_t stream);
int srlz_conv64_wino_tiles(const srlz_conv64_desc* d);
int srlz_conv64_wino_fwd(const float* x, const float* upack_fwd, const float* bias /* may be NULL */, float* y,
                         float* stats_partial /* may be NULL */, const float* x_bnp /* may be NULL: as srlz_conv64_fwd's — x is the raw
                         output of the previous convolution, the layer's input relu(batchnorm(x)) with these records */,
                         const srlz_conv64_desc* d, srlz_stream_t stream);
/* dx = d(loss)/dx from dy, same kernel with upack_bwd.  The _pool_sums form is srlz_conv64_bwd_data_pool_sums' (above): dx is the gradient
 * of the pooled map `pd` describes and the launch also leaves the pooled block's two BatchNorm-backward sums as
 * srlz_conv64_wino_bwd_data_rows(d) records of 128 floats (group after group; a group's last 64 records come from a companion launch
 * for channels whose BatchNorm scale is (almost) 0 — normally zeros) for srlz_bn_bwd_finalize_partials. */
int srlz_conv64_wino_bwd_data(const float* dy, const float* upack_bwd, float* dx, const srlz_conv64_desc* d, srlz_stream_t stream);
int srlz_conv64_wino_bwd_data_rows(const srlz_conv64_desc* d);
int srlz_conv64_wino_bwd_data_pool_sums(const float* dy, const float* upack_bwd, float* dx, const float* pooled, const float* pool_bnp,
                                        const float* pool_y, const uint8_t* pool_argmax, const struct srlz_pool_desc_s* pd,
                                        float* bn_bwd_partial, const srlz_conv64_desc* d, srlz_stream_t stream);
/* dw_ref (reference layout [co][ci][3][3]) = d(loss)/d(w) of the same layer by the transposed Winograd algorithm: per transform-domain
 * component one [co] x [ci] contraction over all 2x2 patches of (A dY A^T) and (B^T x B), G^T . G in the (fixed-order, fp64) second
 * stage.  Layers without a bias (conv3x3 of the reference has none); ws: srlz_conv64_wino_bwd_weight_workspace(d) bytes. */
size_t srlz_conv64_wino_bwd_weight_workspace(const srlz_conv64_desc* d);
int srlz_conv64_wino_bwd_weight(const float* x, const float* dy, float* dw_ref, void* ws, size_t ws_bytes, const srlz_conv64_desc* d,
                                srlz_stream_t stream);
/* workspace (bytes) for bwd_weight */
size_t srlz_conv64_bwd_weight_workspace(const srlz_conv64_desc* d);
/* dw_ref (reference layout) = d(loss)/d(w); dbias[64] = sum of dy over n,h,w (may be NULL).
 * Deterministic: split-K partials in `ws`, fixed-order second-stage reduction (learner.py:62 asks cuDNN for the same). */
int srlz_conv64_bwd_weight(const float* x, const float* dy, float* dw_ref, float* dbias, const float* x_bnp /* as above */,
                           const srlz_bn_bwd_operand* dy_bn /* may be NULL */,
                           void* ws, size_t ws_bytes, const srlz_conv64_desc* d, srlz_stream_t stream);
/* Host only (no launch): what srlz_conv64_bwd_weight would run for this layer with (has_x_bnp) / without a fused x_bnp and with
 * (has_dy_bn) / without a gradient rebuilt from (dA, y).  out[0] = the kernel: 0 conv64_wgrad_ring_s2_kernel, 1 conv64_wgrad_ring_kernel,
 * 2 conv64_wgrad_gather_kernel, 3 conv64_wgrad_kernel (chunk at a time); out[1] = workgroups launched (<= the workspace's);
 * out[2] = chunks per workgroup — 0 and 1: every workgroup of a BatchNorm group takes that many consecutive chunks, the group's last
 * one what is left; 2 and 3: the most any workgroup takes, striding over all chunks by out[1]; out[3] = grid positions per chunk. */
int srlz_conv64_bwd_weight_plan(const srlz_conv64_desc* d, int has_x_bnp, int has_dy_bn, int out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * convN — FORWARD-ONLY 3x3 (pad 1, stride 1/2) and 1x1 (stride 2) convolutions without bias for Cin, Cout multiples of 64:
 * the frozen ResNet-18 trunk behind EmbeddingNet (models/triplet.py:6-39; torchvision 0.2.1 resnet18: BasicBlock conv3x3
 * layers and the 1x1 downsample convolutions).  Same fp32-MFMA implicit GEMM as the 64->64 family; no gradient exists
 * because the reference freezes the trunk (triplet.py:17-19).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  int n, hi, wi, ho, wo; /* NHWC activations: x [n,hi,wi,cin] -> y [n,ho,wo,cout] */
  int cin, cout;         /* multiples of 64; cin a power of two from 64 to 512 (every entry point refuses anything else) */
  int ksize, stride, pad; /* (3, 1|2, 1) or (1, 2, 0) */
  int groups;            /* BatchNorm groups batched along n (0 / 1 = one), as in srlz_conv64_desc: the launch is the union of
                            `groups` independent trunk calls — the anchor / positive / negative views of obs and next_obs of one
                            time-contrastive step, models/learner.py:383-391.  stats_partial is then
                            [cout/64][groups][tiles / groups][128], x_bnp [groups][cin/64][256] */
} srlz_convn_desc;
size_t srlz_convn_packed_floats(const srlz_convn_desc* d);
/* w_ref [cout,cin,k,k] (torch layout) -> the kernel's packed copy (srlz_convn_packed_floats floats) */
int srlz_convn_pack_weights(const float* w_ref, float* wpack, const srlz_convn_desc* d, srlz_stream_t stream);
/* per-tile BatchNorm partial records per block of 64 output channels (stats_partial is [cout/64][tiles][128]) */
int srlz_convn_fwd_tiles(const srlz_convn_desc* d);
/* y = conv(x); x_bnp (may be NULL): the input is relu(batchnorm(x)) with one 256-float record per block of 64 input channels */
int srlz_convn_fwd(const float* x, const float* wpack, float* y, float* stats_partial, const float* x_bnp,
                   const srlz_convn_desc* d, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * "Skinny" convolutions: one side has C in {3,6,9} image channels stored NCHW, the other 64 channels NHWC.
 *   kind 0: nn.Conv2d(C,64,k=7,s=2,p=3,bias=False)       models/models.py:49   (encoder conv1)
 *   kind 1: nn.ConvTranspose2d(64,C,k=4,s=2)             models/models.py:82   (decoder's last layer)
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  int n;       /* images */
  int c;       /* image channels: 3, 6 or 9 */
  int himg, wimg; /* image-side spatial size (224 x 224) */
  int hf, wf;  /* 64-channel feature-map spatial size (112x112 for kind 0, 111x111 for kind 1) */
  int kind;    /* 0 = conv1 7x7 s2 p3 ; 1 = convT 4x4 s2 p0 */
  int groups;  /* BatchNorm groups along n (0 / 1 = one), as in srlz_conv64_desc */
} srlz_skinny_desc;

int srlz_skinny_tiles(const srlz_skinny_desc* d); /* BN partial records written by conv1 forward */
/* Host only: the persistent workgroups that walk those tiles in srlz_conv1_fwd(_u8) and srlz_conv1_bwd_weight(_fused(_u8)). */
int srlz_conv1_workgroups(const srlz_skinny_desc* d);
/* Host only: 1 when srlz_conv1_fwd(_u8) and srlz_conv1_bwd_weight_fused(_u8) stage their image windows through a buffer resource
 * (32-bit offsets from a scalar base, out-of-image elements dropped by the hardware's range check), 0 when they keep the
 * generic-pointer staging: C = 3 and kind 0 only, the image tensor — judged as floats — below 2^32 bytes (with the few rows the first
 * window starts in front of it), one image plane below 2^24 bytes and one image's feature map below 2^32 bytes.  The results are the
 * same bits either way (srlz_debug_conv1_*_generic run the generic staging regardless). */
int srlz_conv1_buffer_staging_supported(const srlz_skinny_desc* d);
/* kind 0 forward: x_nchw [N,C,H,W] -> y_nhwc [N,hf,wf,64]; w_ref [64,C,7,7]. stats_partial as in srlz_conv64_fwd. */
int srlz_conv1_fwd(const float* x_nchw, const float* w_ref, float* y_nhwc, float* stats_partial,
                   const srlz_skinny_desc* d, srlz_stream_t stream);
/* The same layer on frames that are still the loader's BYTES: x_u8 [N,C,himg,wimg] uint8, planar — the reference's tensor layout
 * (preprocessing/data_loader.py:255: transpose(0,3,2,1) of the [B,H,W,C] image batch) taken BEFORE preprocessInput — and
 * norm_lut = the 3 x 256 table of srlz_normalize_lut.  ((v/255) - mean[c]) / std[c] (preprocessing/utils.py:20-32) is applied
 * while the window lands in LDS: identical bits to srlz_conv1_fwd on the normalised float tensor, a quarter of the input bytes,
 * and no normalisation pass in the step.  Same for the fused weight gradient and the fused reconstruction loss below. */
int srlz_conv1_fwd_u8(const uint8_t* x_u8, const float* norm_lut, const float* w_ref, float* y_nhwc, float* stats_partial,
                      const srlz_skinny_desc* d, srlz_stream_t stream);
size_t srlz_skinny_bwd_weight_workspace(const srlz_skinny_desc* d);
/* kind 0 data gradient: dx_nchw [N,C,himg,wimg] = d(loss)/d(image) from dy_nhwc [N,hf,wf,64].  The training path never
 * needs it (conv1 is the first layer); it exists for the perceptual loss (losses/losses.py:217-236), whose frozen
 * denoiser encodes a DECODED image that carries a gradient (models/learner.py:404-412). */
int srlz_conv1_bwd_data(const float* dy_nhwc, const float* w_ref, float* dx_nchw, const srlz_skinny_desc* d,
                        srlz_stream_t stream);
/* kind 0 weight gradient: dw_ref [64,C,7,7] from x_nchw and dy_nhwc. */
int srlz_conv1_bwd_weight(const float* x_nchw, const float* dy_nhwc, float* dw_ref, void* ws, size_t ws_bytes,
                          const srlz_skinny_desc* d, srlz_stream_t stream);
/* kind 0 weight gradient with the BatchNorm + ReLU + MaxPool backward of the FOLLOWING block fused into the operand load:
 * dy = d(loss)/d(conv1 output) is never materialised (it has no other consumer: conv1 needs no data gradient).
 * y_nhwc / bnp / argmax as in srlz_bn_relu_pool_fwd, dpooled = gradient of the pooled map (NHWC),
 * sums = output of srlz_bn_relu_pool_bwd_sums; pd describes that pooling layer. */
int srlz_conv1_bwd_weight_fused(const float* x_nchw, const float* y_nhwc, const float* bnp, const uint8_t* argmax,
                                const float* dpooled, const float* sums, int training, float* dw_ref, void* ws,
                                size_t ws_bytes, const srlz_skinny_desc* d, const struct srlz_pool_desc_s* pd,
                                srlz_stream_t stream);
int srlz_conv1_bwd_weight_fused_u8(const uint8_t* x_u8, const float* norm_lut, const float* y_nhwc, const float* bnp,
                                   const uint8_t* argmax, const float* dpooled, const float* sums, int training, float* dw_ref,
                                   void* ws, size_t ws_bytes, const srlz_skinny_desc* d, const struct srlz_pool_desc_s* pd,
                                   srlz_stream_t stream);
/* kind 1 forward: x_nhwc [N,hf,wf,64] -> y_nchw [N,C,H,W] = convT(x) + bias; w_ref [64,C,4,4]. */
int srlz_convT_out_fwd(const float* x_nhwc, const float* w_ref, const float* bias, float* y_nchw,
                       const float* x_bnp /* may be NULL, see srlz_conv64_fwd */, const srlz_skinny_desc* d,
                       srlz_stream_t stream);
/* kind 1 data gradient: dx_nhwc [N,hf,wf,64] from dy_nchw.
 * x_raw / x_bnp / bn_bwd_partial (all three or none): the layer input was relu(batchnorm(x_raw)) (models/models.py:79-81),
 * so dx is dA of that BatchNorm+ReLU; the epilogue then also reads x_raw and writes, per 16x16 tile, the partial
 * BatchNorm-backward sums  bn_bwd_partial[tile][0..64) = sum dA*[bn(x)>0],  [64..128) = sum dA*[bn(x)>0]*xhat
 * (srlz_skinny_tiles(d) rows) for srlz_bn_bwd_finalize_partials — no separate pass over (dA, x_raw). */
int srlz_convT_out_bwd_data(const float* dy_nchw, const float* w_ref, float* dx_nhwc, const float* x_raw,
                            const float* x_bnp, float* bn_bwd_partial, const srlz_skinny_desc* d, srlz_stream_t stream);
/* kind 1 weight gradient: dw_ref [64,C,4,4], dbias [C]. */
int srlz_convT_out_bwd_weight(const float* x_nhwc, const float* dy_nchw, float* dw_ref, float* dbias,
                              const float* x_bnp, void* ws, size_t ws_bytes, const srlz_skinny_desc* d,
                              srlz_stream_t stream);

/* kind 1 data gradient + BatchNorm-backward partials + weight gradient + bias gradient in ONE pass over dy and x_raw (C == 3 or 6,
 * the layer input was relu(batchnorm(x_raw)): the autograd backward of nn.ConvTranspose2d(64, C, 4, stride=2), models/models.py:82,
 * as srlz_convT_out_bwd_data(x_raw, x_bnp, bn_bwd_partial) followed by srlz_convT_out_bwd_weight(x_bnp) would compute it, with
 * x_raw (1.6 GB at 512 images) and dy crossing HBM once instead of twice.  Round 4: output-stationary, one wave per strip of 16
 * feature columns x R rows (csrc/convt_out.hip); bn_bwd_partial has srlz_convT_out_bwd_fused_tiles(d) rows of 128 floats (one per
 * strip, image-major: the records of BatchNorm group g are rows [g, g+1) * tiles / groups); ws >=
 * srlz_convT_out_bwd_fused_workspace(d) bytes.  srlz_convT_out_bwd_fused_supported: 1 for C in {3, 6}, else 0 (use the two calls). */
int srlz_convT_out_bwd_fused_supported(const srlz_skinny_desc* d);
int srlz_convT_out_bwd_fused_tiles(const srlz_skinny_desc* d);
size_t srlz_convT_out_bwd_fused_workspace(const srlz_skinny_desc* d);
/* dy_gain_dev != NULL: `dy_nchw` holds the reconstruction ERROR dec - obs left behind by srlz_convT_out_fwd_loss, and the loss
 * gradient d(loss)/d(dec) = ((dy_gain_dev[0] / dy_gain_div) * dy_gain_coef) * (dec - obs) is formed while it is staged
 * (dy_gain_dev = the upstream gradient of the loss scalar on the device; div = numel per frame for the mean form, 1 for the sum
 * form; coef = 2) — the rounding order autograd uses for sum((dec-obs)^2)/numel.  NULL: dy_nchw is the gradient itself. */
int srlz_convT_out_bwd_fused(const float* dy_nchw, const float* w_ref, float* dx_nhwc, const float* x_raw, const float* x_bnp,
                             float* bn_bwd_partial, float* dw_ref, float* dbias /* may be NULL */, void* ws, size_t ws_bytes,
                             const float* dy_gain_dev, float dy_gain_div, float dy_gain_coef,
                             const srlz_skinny_desc* d, srlz_stream_t stream);

/* The last ConvTranspose forward WITH the reconstruction / generation loss of the step taken in its epilogue (SURVEY.md 8a' K11 /
 * K12; replaces reconstructionLoss / autoEncoderLoss, /root/reference/losses/losses.py:172-196, and generationLoss, :199-214,
 * on the training path — there `obs` is read twice and `decoded` three times, here `decoded` never leaves the chip):
 * the batch is the two frames of a step (images [0, n/2) = obs, [n/2, n) = next_obs; d->groups = BatchNorm groups as usual);
 * err_nchw = dec - target (what the backward needs), dec_nchw = the reconstruction itself (optional, NULL on the training path),
 * loss_partial[2][srlz_convT_out_fwd_loss_workgroups(d)] = per-frame, per-workgroup sums of squared errors (fp64), to be
 * combined by srlz_pair_loss_finalize.  The gradient is err times a scalar: see srlz_convT_out_bwd_fused / srlz_scale_by_scalar. */
int srlz_convT_out_fwd_loss_workgroups(const srlz_skinny_desc* d);
/* Host only: out[0] = jobs (strips of 16 columns), out[1] = persistent workgroups of 4 waves that share them, for srlz_convT_out_fwd /
 * srlz_convT_out_fwd_loss (backward = 0) or srlz_convT_out_bwd_fused (backward = 1). */
int srlz_convT_out_os_plan(const srlz_skinny_desc* d, int backward, int out[2]);
int srlz_convT_out_fwd_loss(const float* x_nhwc, const float* w_ref, const float* bias, const float* target_nchw, float* err_nchw,
                            float* dec_nchw, const float* x_bnp, double* loss_partial, const srlz_skinny_desc* d,
                            srlz_stream_t stream);
/* target_u8: the observations as uint8 [N,C,himg,wimg] + the normalisation table (see srlz_conv1_fwd_u8) */
int srlz_convT_out_fwd_loss_u8(const float* x_nhwc, const float* w_ref, const float* bias, const uint8_t* target_u8,
                               const float* norm_lut, float* err_nchw, float* dec_nchw, const float* x_bnp, double* loss_partial,
                               const srlz_skinny_desc* d, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * BatchNorm2d(64) (+ ReLU (+ MaxPool 3x3 s2)) — nn.BatchNorm2d / nn.ReLU / nn.MaxPool2d,
 * models/models.py:50-52,55-57,60-62 (encoder) and 67-68,71-72,75-76,79-80 (decoder).
 * bnp is a 4x64 float record {mean, invstd, scale = gamma*invstd, shift = beta - mean*scale}.
 * ------------------------------------------------------------------------------------------------------------ */
/* Training-mode statistics from the convolution's per-tile partials: fills bnp and applies `repeat` momentum
 * updates of running_mean / running_var (momentum, unbiased variance — torch defaults eps 1e-5, momentum 0.1).
 * batch_stat[2][64] (may be NULL) receives {mean, unbiased var} so the update can be replayed (VAE getStates quirk,
 * models/learner.py:402).  ws: srlz_bn_bwd_workspace(0) bytes of scratch (two-stage fp64 reduction of the partials).
 * groups > 1: `groups` independent BatchNorm calls batched along n (the conv descriptors' `groups`): stats_partial holds
 * n_partials / groups records per group, group after group; count is PER GROUP; bnp receives `groups` records of 256
 * floats, batch_stat `groups` x 128; the running statistics take the groups' momentum updates in order (obs, then
 * next_obs, models/learner.py:392-393).  Per group the arithmetic is exactly that of a single-group call. */
int srlz_bn_finalize(const float* stats_partial, int n_partials, int groups, long long count, const float* gamma,
                     const float* beta, float eps, float momentum, int repeat, float* running_mean,
                     float* running_var, long long* num_batches_tracked /* int64 counter += groups; may be NULL */,
                     float* bnp, float* batch_stat, void* ws, size_t ws_bytes, srlz_stream_t stream);
/* A C-channel BatchNorm (C = 64 * chunks) of the frozen ResNet-18 trunk as `chunks` independent 64-channel layers:
 * stats_partial is srlz_convn_fwd's [chunks][tiles][128]; gamma / beta / running_* hold C floats; bnp receives `chunks`
 * records of 256 floats (training-mode forward of nn.BatchNorm2d: batch statistics + one momentum update; the trunk's
 * parameters are frozen but the reference leaves it in train() mode, models/learner.py:365 — so its statistics do move).
 * groups > 1 (ABI 103): `groups` independent BatchNorm calls batched along n — stats_partial is
 * [chunks][groups][tiles / groups][128] (`tiles` counts all groups), count is PER GROUP, bnp receives [groups][chunks][256]
 * (a group's records contiguous), the running statistics take the groups' momentum updates in order and the counter += groups:
 * bit for bit what `groups` separate calls leave.  ws >= srlz_bn_finalize_chunks_workspace(chunks, groups) bytes. */
size_t srlz_bn_finalize_chunks_workspace(int chunks, int groups);
int srlz_bn_finalize_chunks(const float* stats_partial, int tiles, int chunks, int groups, long long count, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                            long long* num_batches_tracked /* += groups; may be NULL */, float* bnp, void* ws, size_t ws_bytes,
                            srlz_stream_t stream);
int srlz_bn_eval_params_chunks(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float eps, int chunks, float* bnp, srlz_stream_t stream);
/* out = relu(bn(a) + (b_bnp ? bn(b) : b)) over pixels x 64*chunks — BasicBlock's `out = relu(bn2(out) + identity)`;
 * groups > 1: records [groups][chunks][256], group g = pixels [g, g+1) * pixels / groups */
int srlz_bn_add_relu(const float* a, const float* a_bnp, const float* b, const float* b_bnp, float* out, long long pixels,
                     int chunks, int groups, srlz_stream_t stream);
/* out[n,c] = mean over hw of x[n,hw,c] — resnet18.avgpool */
int srlz_avgpool_nhwc(const float* x, float* out, int n, int hw, int c, srlz_stream_t stream);
/* Eval-mode bnp from running statistics. */
int srlz_bn_eval_params(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, float* bnp, srlz_stream_t stream);
/* running = (1-m)*running + m*batch_stat, once (replay of a previous call's statistics). */
int srlz_bn_replay(const float* batch_stat, float momentum, float* running_mean, float* running_var,
                   srlz_stream_t stream);
/* The same for up to SRLZ_BN_REPLAY_MAX different layers in ONE launch, each with its nn.BatchNorm2d.num_batches_tracked (+= 1; may be
 * NULL): the learner's getStates(obs) after forward(obs) in train mode (models/learner.py:402 with models.py:131-139) re-runs the three
 * encoder BatchNorms of a frame on the same batch.  `items` is a HOST array. */
#define SRLZ_BN_REPLAY_MAX 8
typedef struct {
  const float* batch_stat;  /* [128]: batch mean, unbiased batch variance (srlz_bn_finalize's batch_stat record of the group) */
  float* running_mean;
  float* running_var;
  long long* num_batches_tracked;
} srlz_bn_replay_item;
int srlz_bn_replay_many(const srlz_bn_replay_item* items, int n, float momentum, srlz_stream_t stream);

typedef struct srlz_pool_desc_s {
  int n, h, w;      /* input  [N,h,w,64] */
  int hp, wp;       /* pooled [N,hp,wp,64] */
  int pool_pad;     /* 0 or 1 (kernel 3, stride 2) */
  int out_nchw;     /* 1: write the pooled map as [N,64,hp,wp] (feeds Linear(2304,S), autoencoders.py:107-108) */
  int groups;       /* BatchNorm groups along n (0 / 1 = one), as in srlz_conv64_desc: bnp / sums hold one record per group */
} srlz_pool_desc;

/* pooled = maxpool3x3s2(relu(y*scale+shift)); argmax (uint8 per output, window index 0..8) may be NULL (eval). */
int srlz_bn_relu_pool_fwd(const float* y, const float* bnp, float* pooled, uint8_t* argmax,
                          const srlz_pool_desc* d, srlz_stream_t stream);
size_t srlz_bn_bwd_workspace(long long elems);
/* First half of the backward below: sums[128] = {sum dz[64], sum dz*xhat[64]} (= dbeta, dgamma). */
int srlz_bn_relu_pool_bwd_sums(const float* y, const float* bnp, const uint8_t* argmax, const float* dpooled,
                               const float* pooled, float* sums, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                               const srlz_pool_desc* d, srlz_stream_t stream);
/* dy (same shape as y) and dgamma[64], dbeta[64] from dpooled.  training != 0: batch-statistics backward;
 * training == 0: running-statistics backward (validation minibatches, models/learner.py:362-364,489). */
int srlz_bn_relu_pool_bwd(const float* y, const float* bnp, const uint8_t* argmax, const float* dpooled,
                          const float* pooled /* forward output, may be NULL (slower) */, float* dy, float* dgamma,
                          float* dbeta, int training, void* ws, size_t ws_bytes, const srlz_pool_desc* d,
                          srlz_stream_t stream);
/* Stage 2 alone: dy from sums that are already known (srlz_bn_relu_pool_bwd_sums, or srlz_bn_bwd_finalize_partials over the records of
 * srlz_conv64_bwd_data_pool_sums). */
int srlz_bn_relu_pool_bwd_apply(const float* y, const float* bnp, const uint8_t* argmax, const float* dpooled, const float* sums,
                                float* dy, int training, const srlz_pool_desc* d, srlz_stream_t stream);
/* a = relu(y*scale+shift) over `pixels` x 64 */
int srlz_bn_relu_fwd(const float* y, const float* bnp, float* a, long long pixels, srlz_stream_t stream);
/* Second stage for the per-tile partials of a data-gradient epilogue (srlz_convT_out_bwd_data, srlz_conv64_bwd_data):
 * partial[n_partials][128] -> sums[128], dgamma[64], dbeta[64]; fp64 across tiles, fixed order. */
int srlz_bn_bwd_finalize_partials(const float* partial, int n_partials, int groups, float* sums, float* dgamma, float* dbeta,
                                  void* ws, size_t ws_bytes, srlz_stream_t stream);
/* First half of srlz_bn_relu_bwd: sums[128] = {sum dz[64], sum dz*xhat[64]} (= dbeta, dgamma), for srlz_bn_bwd_operand. */
/* (groups > 1: bnp / sums hold one record per group, `pixels` counts all groups; dgamma / dbeta are the groups' totals) */
int srlz_bn_relu_bwd_sums(const float* y, const float* bnp, const float* da, float* sums, float* dgamma, float* dbeta,
                          void* ws, size_t ws_bytes, long long pixels, int groups, srlz_stream_t stream);
int srlz_bn_relu_bwd(const float* y, const float* bnp, const float* da, float* dy, float* dgamma, float* dbeta,
                     int training, void* ws, size_t ws_bytes, long long pixels, int groups, srlz_stream_t stream);
/* [N,C,H,W] <-> [N,H,W,C] for the two 6x6x64 seams around the FC layers (autoencoders.py:107-108,116-117). */
int srlz_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, srlz_stream_t stream);
int srlz_nhwc_to_nchw(const float* src, float* dst, int n, int c, int h, int w, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Dense layers of the mlp / linear models (csrc/dense.hip): the nn.Linear whose input or output is the flattened image,
 * K = input_dim = C * W * H (preprocess.py getInputDim), M = images of the call, n = the small side (1..256).
 * x / target come as fp32 [M][K] or as the loader's planar uint8 frames [M][C][W][H] with the srlz_normalize_lut table
 * (plane = W * H; the two routes agree bit for bit).  W in torch [out, in] layout.  No float atomics: deterministic.
 * ------------------------------------------------------------------------------------------------------------ */
/* 1 when M, n, K, plane fit the kernels (n <= 256, K = 3 or 6 planes, every offset below 2^31), else 0 with the reason in
 * srlz_last_error().  Every dense launcher checks it. */
int srlz_dense_supported(int M, int n, int K, int plane);
/* y[M,n] = act(x . W[n,K]^T + b), act 0 none / 1 ReLU / 2 tanh — nn.Linear(input_dim, h) of autoencoders.py:15,51,
 * vae.py:17 (+ ReLU, vae.py:35), priors.py:89 (+ ReLU), priors.py:116.  x or x_u8 (+ lut) is non-NULL.  Split over K,
 * partials in ws (srlz_dense_in_workspace bytes) summed in a fixed order. */
size_t srlz_dense_in_workspace(int M, int n, int K);
int srlz_dense_in_fwd(const float* x, const uint8_t* x_u8, const float* norm_lut, const float* w, const float* b, float* y, int M,
                      int n, int K, int plane, int act, void* ws, size_t ws_bytes, srlz_stream_t stream);
/* dW[n,K] = dy^T . x, db[n] = sum_m dy (db may be NULL) — the weight gradient of the layers above (no data gradient: the
 * images need none). */
int srlz_dense_in_wgrad(const float* dy, const float* x, const uint8_t* x_u8, const float* norm_lut, float* dw, float* db, int M,
                        int n, int K, int plane, srlz_stream_t stream);
/* out[M,K] = z[M,n] . W[K,n]^T + b — nn.Linear(h, input_dim) of autoencoders.py:19,59, vae.py:29 (the decoded frames). */
int srlz_dense_out_fwd(const float* z, const float* w, const float* b, float* out, int M, int n, int K, int plane,
                       srlz_stream_t stream);
/* The same layer with the reconstruction / generation loss (losses.py:172-214) in the epilogue instead of the frames:
 * partial[2][workgroups] fp64 sums of (out - target)^2 over rows < half (frame 0) and rows >= half (frame 1), for
 * srlz_pair_loss_finalize. */
int srlz_dense_out_fwd_loss_workgroups(int M, int K);
int srlz_dense_out_fwd_loss(const float* z, const float* w, const float* b, const float* target, const uint8_t* target_u8,
                            const float* norm_lut, double* partial, int M, int n, int K, int plane, int half, srlz_stream_t stream);
/* Backward of that loss: dOut = ((gain[0] / div) * 2) * (z W^T + b - target) recomputed, then dw[K,n] = dOut^T . z,
 * db[K] = column sums of dOut and (dz non-NULL) dz[M,n] = dOut . W.  ws: srlz_dense_out_bwd_workspace bytes. */
size_t srlz_dense_out_bwd_workspace(int M, int n, int K);
int srlz_dense_out_bwd(const float* z, const float* w, const float* b, const float* target, const uint8_t* target_u8,
                       const float* norm_lut, const float* gain, float div, float* dz, float* dw, float* db, int M, int n, int K,
                       int plane, void* ws, size_t ws_bytes, srlz_stream_t stream);
/* The same gradients from a given dOut [M,K] (the materialised route: any loss of the decoded frames).  ws: at least
 * srlz_dense_in_workspace(M, n, K) bytes. */
int srlz_dense_out_bwd_from(const float* dout, const float* z, const float* w, float* dz, float* dw, float* db, int M, int n, int K,
                            int plane, void* ws, size_t ws_bytes, srlz_stream_t stream);
/* nn.Tanh of the dense auto-encoder (autoencoders.py:52-62): y = tanh(x); dx = (1 - y^2) * dy. */
int srlz_tanh_fwd(const float* x, float* y, int n, srlz_stream_t stream);
int srlz_tanh_bwd(const float* y, const float* dy, float* dx, int n, srlz_stream_t stream);
/* out = a + b — GaussianNoiseVariant's x + noise (custom_layers.py:49-50). */
int srlz_add_f32(const float* a, const float* b, float* out, int n, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Linear layers — nn.Linear: autoencoders.py:94-100, vae.py:52-57, forward_inverse.py:16,48-55.
 * y[M,N] = x[M,K] . w[N,K]^T + b[N]   (w in torch [out,in] layout), optional ReLU on y.
 * ------------------------------------------------------------------------------------------------------------ */
/* ws (may be NULL): srlz_linear_workspace bytes; lets skinny GEMMs split their reduction over more workgroups
 * (deterministic two-stage sum). */
size_t srlz_linear_workspace(int M, int N, int K);
int srlz_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int relu,
                    void* ws, size_t ws_bytes, srlz_stream_t stream);
/* dx[M,K] = dy[M,N] . w[N,K] */
/* The forward model's residual (forward_inverse.py:27-37: next_state = state + Linear([state ; onehot(action)])) in the GEMM's
 * epilogue: y = (x . w^T + b) + res with res [M, N] — two separately rounded fp32 adds, as the reference rounds them — and its data
 * gradient restricted to the first Kout input columns (the state part of the concatenation) with the residual branch's gradient
 * added: dx[M, Kout] = (dy . w)[:, :Kout] + res, res [M, Kout] (res = dy for the residual above: N == Kout). */
int srlz_linear_fwd_res(const float* x, const float* w, const float* b, const float* res, float* y, int M, int N, int K, int relu,
                        void* ws, size_t ws_bytes, srlz_stream_t stream);
int srlz_linear_bwd_data_res(const float* dy, const float* w, const float* res, float* dx, int M, int N, int K, int Kout, void* ws,
                             size_t ws_bytes, srlz_stream_t stream);
int srlz_linear_bwd_data(const float* dy, const float* w, float* dx, int M, int N, int K, void* ws, size_t ws_bytes,
                         srlz_stream_t stream);
/* dw[N,K] = dy^T . x ; db[N] = column sums of dy (may be NULL) */
int srlz_linear_bwd_weight(const float* dy, const float* x, float* dw, float* db, int M, int N, int K,
                           void* ws, size_t ws_bytes, srlz_stream_t stream);
/* dy *= (y > 0)  — backward of the fused ReLU */
int srlz_relu_bwd_inplace(const float* y, float* dy, long long n, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Losses — losses/losses.py.  `out` scalars are device floats; partial sums are reduced in fp64 in a fixed order.
 * ------------------------------------------------------------------------------------------------------------ */
size_t srlz_reduce_workspace(long long n);
/* out[0] = sum((a-b)^2)            reconstructionLoss 172-181 (caller divides by numel) / F.mse_loss(sum) 210-211 */
int srlz_sqdiff_sum(const float* a, const float* b, long long n, float* out, void* ws, size_t ws_bytes,
                    srlz_stream_t stream);
/* The same for `groups` consecutive slices of n_per_group elements (the two frames of a step batched along n): out[g] is
 * group g's sum, each exactly as a single call on that slice would compute it. */
int srlz_sqdiff_sum_groups(const float* a, const float* b, long long n_per_group, int groups, float* out, void* ws,
                           size_t ws_bytes, srlz_stream_t stream);
/* da[i] = coef_dev[0] * coef * (a[i]-b[i])   (gradient of the above w.r.t. a; coef_dev may be NULL = 1) */
int srlz_sqdiff_grad(const float* a, const float* b, const float* coef_dev, float coef, float* da, long long n,
                     srlz_stream_t stream);
/* grouped form: slice g is scaled by (coef_dev[g * coef_stride] / div) * coef   (coef_stride 0: one shared upstream scalar) */
int srlz_sqdiff_grad_groups(const float* a, const float* b, const float* coef_dev, int coef_stride, float div, float coef,
                            float* da, long long n_per_group, int groups, srlz_stream_t stream);
/* The loss of a batched pair a = [a0 ; a1], b = [b0 ; b1] in one go: sums[g] = sum((a_g - b_g)^2) and
 * comb[0] = sums[0]/n + sums[1]/n (mean != 0: autoEncoderLoss, losses.py:184-196) or sums[0] + sums[1] (generationLoss,
 * losses.py:199-214), rounded like the reference's separate fp32 operations. */
/* Second stage of a pair loss whose fp64 partials [2][nb] another kernel wrote (srlz_convT_out_fwd_loss): sums[g] and
 * comb = sums[0]/n + sums[1]/n (mean) or sums[0] + sums[1], rounded exactly like srlz_sqdiff_pair_loss.
 * (/root/reference/losses/losses.py:181,196 / :210-214) */
int srlz_pair_loss_finalize(const double* partial, int nb, long long n_per_group, int mean, float* sums, float* comb,
                            srlz_stream_t stream);
/* out = ((gain_dev[0] / div) * coef) * x (in place allowed): the gradient of a fused pair loss materialised from the stored
 * error for consumers that cannot apply the factor themselves (autograd of F.mse_loss, /root/reference/losses/losses.py:210). */
int srlz_scale_by_scalar(const float* x, const float* gain_dev, float div, float coef, float* out, long long n,
                         srlz_stream_t stream);
int srlz_sqdiff_pair_loss(const float* a, const float* b, long long n_per_group, int mean, float* sums, float* comb,
                          void* ws, size_t ws_bytes, srlz_stream_t stream);
/* out = [a ; b] (n_each floats each) — joins the halves of a batched pair (th.cat of learner.py's obs / next_obs) */
int srlz_join2(const float* a, const float* b, float* out, long long n_each, srlz_stream_t stream);

/* LossManager.computeTotalLoss (losses/losses.py:55-56): total = sum_i w_i * l_i over n <= SRLZ_MAX_LOSS_TERMS device scalars, in
 * Python's left-to-right fp32 order with separately rounded products.  `scalars` and `weights` are HOST arrays (of device pointers /
 * of floats).  tail != NULL: also tail[0] = total, tail[1 + i] = l_i (the step's scalars in the gradient bucket's tail,
 * models/learner.py:485,501-522).  _bwd: g[i] = dout * w_i. */
#define SRLZ_MAX_LOSS_TERMS 15
int srlz_weighted_total(const float* const* scalars, const float* weights, int n, float* total, float* tail,
                        srlz_stream_t stream);
int srlz_weighted_total_bwd(const float* dout, const float* weights, int n, float* g, srlz_stream_t stream);
/* out[0] = -0.5*sum(1 + logvar - mu^2 - exp(logvar))      kullbackLeiblerLoss 239-256 */
/* out[0] = fp32(sum((a-b)^2)) / div      reconstructionLoss 172-181 (div = numel): the fp32 division behind the sum's rounding */
int srlz_sqdiff_mean(const float* a, const float* b, long long n, float div, float* out, void* ws, size_t ws_bytes,
                     srlz_stream_t stream);
int srlz_kl_sum(const float* mu, const float* logvar, long long n, float* out, void* ws, size_t ws_bytes,
                srlz_stream_t stream);
/* dmu += g*mu ; dlogvar += g*0.5*(exp(logvar)-1)   with g = coef_dev[0]*coef */
int srlz_kl_grad(const float* mu, const float* logvar, const float* coef_dev, float coef, float* dmu,
                 float* dlogvar, long long n, srlz_stream_t stream);
/* z = eps*exp(0.5*logvar) + mu        BaseModelVAE.reparameterize models/models.py:147-165 (eps drawn by the host) */
int srlz_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z, long long n,
                     srlz_stream_t stream);
/* dmu = dz ; dlogvar = dz*eps*0.5*exp(0.5*logvar) */
int srlz_reparam_bwd(const float* dz, const float* logvar, const float* eps, float* dmu, float* dlogvar,
                     long long n, srlz_stream_t stream);
/* out[0] = mean_b( logsumexp(logits[b,:]) - logits[b,target[b]] )   nn.CrossEntropyLoss, inverseModelLoss 117-129
 * dlogits (may be NULL) = (softmax - onehot)/B */
int srlz_cross_entropy(const float* logits, const int64_t* target, int B, int A, float* out, float* dlogits,
                       srlz_stream_t stream);
/* nn.PReLU() with one slope — EmbeddingNet.fc[0], models/triplet.py:24 */
int srlz_prelu_fwd(const float* x, const float* slope, float* y, long long n, srlz_stream_t stream);
int srlz_prelu_bwd(const float* x, const float* slope, const float* dy, float* dx, float* dslope, long long n,
                   srlz_stream_t stream);
/* tripletLoss losses/losses.py:360-376: out[0] = mean_b relu(|s-p|^2 - |s-n|^2 + alpha); hinge[B] = active rows (for bwd) */
int srlz_triplet_fwd(const float* s, const float* p, const float* n, int B, int S, float alpha, float* out, float* hinge,
                     srlz_stream_t stream);
int srlz_triplet_bwd(const float* s, const float* p, const float* n, const float* hinge, const float* g, int B, int S,
                     float* ds, float* dp, float* dn, srlz_stream_t stream);
/* cat[b,:] = [s[b,:S], onehot(a[b])]          forwardModel forward_inverse.py:21-31 + encodeOneHot models.py:229-237 */
/* th.cat((state, next_state), dim=1) of the inverse / reward heads (forward_inverse.py:62,78-95) and the split of its gradient
 * (a or b may be NULL: that half is not wanted); out / in: [rows, ca + cb], a: [rows, ca], b: [rows, cb]. */
int srlz_cat_cols(const float* a, const float* b, float* out, int rows, int ca, int cb, srlz_stream_t stream);
int srlz_split_cols(const float* in, float* a, float* b, int rows, int ca, int cb, srlz_stream_t stream);
/* out = ((t0 + t1) + t2) + t3 over nterms (1..4) tensors of n floats, left to right in fp32: the gradient of a tensor with several
 * consumers (states feed the decoder, the forward / inverse / reward heads and the forward loss: models/learner.py:392-449) summed
 * by ONE launch in a fixed order instead of one accumulation kernel per extra consumer.  terms: HOST array of device pointers. */
int srlz_sum_terms(const float* const* terms, int nterms, float* out, long long n, srlz_stream_t stream);
int srlz_concat_onehot(const float* s, const int64_t* a, float* cat, int B, int S, int A, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input pipeline tail: decoded uint8 frames [N,H,W,C] (RGB per 3-group) -> normalised fp32 [N,C,W,H]
 * = preprocessInput(x, "image_net") (preprocessing/utils.py:20-32) + the loader's transpose(0,3,2,1)
 * (preprocessing/data_loader.py:255), bit-identical to the host arithmetic.  Lets the loader ship uint8 over PCIe.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_normalize_u8(const uint8_t* img_nhwc, float* out_ncwh, int n, int h, int w, int c, srlz_stream_t stream);
/* norm_lut[c][v] (3 x 256 floats) = ((v / 255) - mean[c]) / std[c] for v = 0..255 and the image_net mean / std of channel c —
 * preprocessInput (preprocessing/utils.py:20-32) tabulated with its three fp32 roundings; the operand of the *_u8 entry points. */
int srlz_normalize_lut(float* norm_lut, srlz_stream_t stream);
/* Frames already in the reference's tensor layout but still uint8 ([N,C,*] planar, `plane` bytes per channel plane) -> the float
 * tensor, through the table (for consumers that have no *_u8 form; bit-identical to srlz_normalize_u8 of the NHWC frames). */
int srlz_normalize_u8_planar(const uint8_t* x_u8, const float* norm_lut, float* out, int n, int c, long long plane,
                             srlz_stream_t stream);
/* The dataset resident in HBM (round 4): the loader process of /root/reference/preprocessing/data_loader.py:195-256
 * decodes every frame of every epoch again; here a decoded frame is kept ([frames][C][W][H] uint8, 150 KB each: 100 k frames = 15 GB
 * of the 288) and later epochs move frames BY INDEX.  Whole frames of frame_bytes (a multiple of 16) bytes:
 *   dst[dst_index ? dst_index[i] + dst_shift : i] = src[src_index ? src_index[i] + src_shift : i],  i < n  (index arrays: int64, device)
 * gather (next_obs = store[minibatch + 1]: src_shift = 1), scatter (store <- a freshly decoded minibatch), plain copy. */
int srlz_copy_frames_u8(const uint8_t* src, const long long* src_index, long long src_shift, uint8_t* dst,
                        const long long* dst_index, long long dst_shift, int n, long long frame_bytes, srlz_stream_t stream);
/* The same between frames of different pitch, for a byte range inside the frame:
 *   dst[df][dst_offset .. dst_offset + copy_bytes) = src[sf][src_offset .. src_offset + copy_bytes),  frames src_frame_bytes / dst_frame_bytes apart.
 * The time-contrastive triplets of /root/reference/preprocessing/data_loader.py:219-243 are [view 1 ; view 2 ; view 1 of ANOTHER time step
 * of the same record] = 9 channels; the store keeps the two views of every time step (6 channels), so a triplet minibatch is two
 * gathers by index — the frame's own two views, and the negative's first — and no pixel of it is decoded again (round 5). */
int srlz_copy_frames_u8_strided(const uint8_t* src, const long long* src_index, long long src_shift, long long src_frame_bytes,
                                long long src_offset_bytes, uint8_t* dst, const long long* dst_index, long long dst_shift,
                                long long dst_frame_bytes, long long dst_offset_bytes, int n, long long copy_bytes, srlz_stream_t stream);
/* The DAE loader's occluded copies (preprocessing/data_loader.py:100-111) made on the device from resident frames: out [n,C,W,H] fp32 =
 * the normalised frame store[index[i] + shift] with the rectangle rects[i][view] = (h1, h2, w1, w2) set to 0, one rectangle per
 * camera view (group of 3 channels); the rectangles are drawn by the loader process with the reference's np.random calls. */
int srlz_occlude_frames_u8(const uint8_t* store, const long long* index, long long shift, const int* rects, const float* norm_lut,
                           float* out, int n, int c, int w, int h, srlz_stream_t stream);

/* SRLModulesSplit.detachSplit (models/modules.py:191-236): the state rebuilt from zero blocks and ONE kept slice is a
 * column mask: y[r][c] = x[r][c] for lo <= c < hi, else 0.  Its backward is the same call on the gradient. */
int srlz_mask_columns(const float* x, float* y, int rows, int cols, int lo, int hi, srlz_stream_t stream);

/* l1Loss / l2Loss (losses/losses.py:132-155) over the list of regularised parameters (LossManager.reg_params,
 * losses.py:30-31).  ptrs[nseg] / lens[nseg]: DEVICE arrays with the device address and element count of each tensor.
 * mode 0: norms[i] = sum |p_i|,  out = scale * sum_i norms[i]           (l1: scale = 1)
 * mode 1: norms[i] = ||p_i||_2,  out = scale * sum_i norms[i]           (l2: scale = 1/nseg)
 * fp64 accumulation, one workgroup per tensor, fixed order. */
int srlz_param_norms(const float* const* ptrs, const long long* lens, int nseg, int mode, float scale, float* norms,
                     float* out, srlz_stream_t stream);
/* gradient of the above into gptrs[i] (same shapes): coef * sign(p) (mode 0) or coef * p / norms[i] (mode 1),
 * coef = coef_dev[0] * scale (coef_dev may be NULL = 1). */
int srlz_param_norms_grad(const float* const* ptrs, float* const* gptrs, const long long* lens, int nseg, int mode,
                          const float* norms, const float* coef_dev, float scale, srlz_stream_t stream);

/* Gradient delivery.  The weight-gradient kernels write each parameter's k-th contribution of a backward pass into
 * stage k (stages = nstage copies of the flat bucket, each n floats); this call folds them into the bucket,
 * grad[i] = ((grad[i] + stage0[i]) + stage1[i]) ..., and clears the stages.  One launch replaces autograd's per-parameter,
 * per-contribution `grad += new` kernels (AccumulateGrad behind loss.backward(), models/learner.py:487-489). */
int srlz_fold_grads(float* grad, float* stages, long long n, int nstage, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The reward-prior and episode-prior losses (csrc/priors.hip).  fp32 tensors, row-major; every reduction in a fixed order, no
 * float atomics.
 * ------------------------------------------------------------------------------------------------------------ */
/* rewardPriorLoss losses/losses.py:290-304 with correlationMatrix losses/utils.py:120-134 (call: models/learner.py:470-474):
 * out[0] = 1 - mean_j |clamp(corr[S, j], -1, 1)| of X = cat([states, rewards], 1)^T, states [B, S], rewards [B] (raw float
 * rewards), B >= 2.  fwd leaves the reward statistics and per column (mean, inv stddev, corr, cov) in ws
 * (srlz_reward_prior_workspace(S) bytes); bwd reads them: dstates [B, S] = g[0] * d out / d states. */
size_t srlz_reward_prior_workspace(int S);
int srlz_reward_prior_fwd(const float* states, const float* rewards, int B, int S, float* out, double* ws, size_t ws_bytes,
                          srlz_stream_t stream);
int srlz_reward_prior_bwd(const float* states, const float* rewards, const double* ws, size_t ws_bytes, const float* g, int B, int S,
                          float* dstates, srlz_stream_t stream);
/* episodePriorLoss losses/losses.py:307-359 with Discriminator / ReverseLayerF models/priors.py:129-175 (learner.py:476-479):
 * out[0] = BCELoss(sum)(Discriminator(cat(s_i, s_{others[i]})), same_i), states [B, S], others int32 [B] in [0, B), same [B]
 * (0 / 1), w1 [64, 2S], b1 [64], w2 [64, 64], b2 [64], w3 [1, 64], b3 [1].  An index outside [0, B) is never read through: it pairs
 * its row with itself, consistently in fwd and bwd (srlz.ops.EpisodePriorFn rejects such indices when it is handed host indices).  fwd keeps the hidden activations and p in ws
 * (srlz_episode_prior_workspace(B, S) bytes); ticket: one device int, zero before the first call, left zero by every call (the
 * workgroup that finishes last adds the row terms).  bwd (two launches): dstates = -(d loss / d states) (the reversed gradient,
 * lambda = 1) and the six parameter gradients (overwritten), all for upstream g[0]. */
size_t srlz_episode_prior_workspace(int B, int S);
int srlz_episode_prior_fwd(const float* states, const int* others, const float* same, int B, int S, const float* w1, const float* b1,
                           const float* w2, const float* b2, const float* w3, const float* b3, float* out, void* ws, size_t ws_bytes,
                           unsigned* ticket, srlz_stream_t stream);
int srlz_episode_prior_bwd(const float* states, const int* others, const float* same, const float* g, int B, int S, const float* w1,
                           const float* w2, const float* w3, void* ws, size_t ws_bytes, float* dstates, float* dw1, float* db1,
                           float* dw2, float* db2, float* dw3, float* db3, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Adam over one flat parameter buffer — th.optim.Adam(params, lr) models/learner.py:199,495 (torch defaults).
 * step is 1-based; grad_scale multiplies g first (1/world_size after the RCCL sum).  The hyper-parameters are doubles, as
 * torch holds them: lr / (1 - beta1^step), sqrt(1 - beta2^step) and (1 - beta) are evaluated in double and rounded once.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_adam_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2,
                   double eps, int step, float grad_scale, srlz_stream_t stream);
/* The same update with the step count kept ON THE DEVICE (step_dev[0] is incremented first; bc_dev = 2 floats of scratch):
 * the form a captured hipGraph can replay, since a kernel argument frozen at capture time cannot advance. */
int srlz_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2,
                       double eps, int* step_dev, float* bc_dev, float grad_scale, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Data-parallel exchange over RCCL (xGMI): one process per GPU, ONE in-place sum all-reduce of the flat fp32 bucket per
 * training step (gradients + scalar tail).  New — the reference is single-device (models/learner.py:65,187); the call
 * sits between loss.backward() (learner.py:489) and optimizer.step() (learner.py:495).
 * Rank 0 calls srlz_comm_unique_id() and shares the srlz_comm_unique_id_bytes() bytes with every rank (any host
 * rendezvous); every rank then calls srlz_comm_init() once with its HIP device current.  RCCL is dlopen'ed on first use
 * (the copy already loaded into the process is reused).  id buffers are HOST memory.
 * ------------------------------------------------------------------------------------------------------------ */
size_t srlz_comm_unique_id_bytes(void);
int srlz_comm_unique_id(void* id_out_host);
int srlz_comm_init(const void* id_host, int rank, int world);
int srlz_comm_world(void); /* 0 before srlz_comm_init */
int srlz_comm_allreduce_f32(float* buf, long long n, srlz_stream_t stream);
int srlz_comm_destroy(void);

/* ------------------------------------------------------------------------------------------------------------
 * The supervised baseline (csrc/supervised.hip).  fp32 tensors, row-major; fixed summation order, no atomics.
 * ------------------------------------------------------------------------------------------------------------ */
/* nn.MSELoss() of the predicted against the ground-truth states and its gradient in ONE launch (reference
 * srl_baselines/supervised.py:85,103-104: criterion(pred_states, target_states.detach()); loss.backward()):
 * loss[0] = fp32(sum((pred - target)^2) / (B * S)), the sum in fp64 in a fixed order and rounded once;
 * dpred_unit [B, S] = 2 (pred - target) / (B * S), i.e. d loss / d pred for an incoming gradient of 1 (the backward is
 * srlz_scale_by_scalar of it by the incoming scalar).  No gradient to the target.  Any B >= 1, S >= 1 with B * S <= 2^20; beyond
 * that SRLZ_ERR_BAD_DESC.  Buffers 16-byte aligned. */
int srlz_mse_target_fwd(const float* pred, const float* target, int B, int S, float* loss, float* dpred_unit, srlz_stream_t stream);
/* F.dropout(x, p, training=True) with the caller's mask (reference models/supervised.py:26): y = x * mask / keep with
 * keep = 1 - p in (0, 1] and mask [rows, cols] uint8 (0 = dropped, anything else = kept), the fp32 operations in that order.
 * bwd: dx = dy * mask / keep.  Any rows >= 1, cols >= 1; in place allowed.  Eval mode calls neither. */
int srlz_dropout_fwd(const float* x, const unsigned char* mask, float keep, float* y, int rows, int cols, srlz_stream_t stream);
int srlz_dropout_bwd(const float* dy, const unsigned char* mask, float keep, float* dx, int rows, int cols, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation: exact k nearest neighbours in fp64 (csrc/knn.hip).  Replaces
 *   NearestNeighbors(n_neighbors=k + 1, algorithm='ball_tree').fit(states).kneighbors(states)      evaluation/knn_images.py:83-84
 * fp64 tensors (with srlz_pca_* the only ones of this ABI): the states of states_rewards.npz are float32 and convert exactly, --ground-truth searches the
 * dataset's float64 states unrounded.
 *   dist2(q, x) = sum_d (q_d - x_d)^2 in fp64, ONE chain acc = fma(q_d - x_d, q_d - x_d, acc) over d = 0 .. D-1 (the differences
 *   form, never |q|^2 + |x|^2 - 2 q.x); the chain of a pair is the same whatever the tiling, so neither the value nor the order
 *   depends on launch geometry, on Q or on how the database is split.
 *   Row r of idx / dist2 [Q, K]: the K rows of db [N, D] with the smallest key (dist2, index) for queries[r], compared
 *   lexicographically, ascending — equal distances go to the lower index.  queries [Q, D] may alias db; nothing is special-cased (a
 *   query that is a database row finds itself at distance 0).  No float atomics, every merge has one order: repeated calls are
 *   bit-identical.  Inputs must be finite (a NaN distance never enters a list).
 * 1 <= K <= 32, K <= N, D >= 1 (no upper limit on D: the dimensions pass through the chip 64 at a time), Q >= 1, N * D and Q * K
 * below 2^31; anything else is SRLZ_ERR_BAD_DESC, a null pointer SRLZ_ERR_NULL, ws_bytes < srlz_knn_workspace(N, Q, D, K)
 * SRLZ_ERR_WORKSPACE — all before any launch.  srlz_knn_workspace returns 0 for a shape the launcher rejects.
 * ------------------------------------------------------------------------------------------------------------ */
size_t srlz_knn_workspace(int N, int Q, int D, int K);
int srlz_knn_f64(const double* db /*[N,D]*/, int N, const double* queries /*[Q,D]*/, int Q, int D, int K, int* idx /*[Q,K]*/,
                 double* dist2 /*[Q,K]*/, void* ws, size_t ws_bytes, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation: ground-truth correlation (GTC) in fp64 (csrc/gtc.hip).  Replaces
 *   corr = np.corrcoef(x=x + eps, y=states_rewards['states'] + eps, rowvar=0)                plotting/representation_plot.py:283
 * of which the reference reads rows 0 .. G-1 only (:296-300: the diagonal entry zeroed, max(abs(row)) per ground-truth dimension).
 * gt [N, G] and states [N, S] are fp64 (float32 states convert exactly); column k of the virtual matrix [gt | states] is gt[:, k]
 * for k < G and states[:, k - G] behind it — the concatenation is never written.
 *   Two passes: mean_k = sum_r col_k[r] / N, then var_k = sum_r (col_k[r] - mean_k)^2 / (N - 1) for all G + S columns and
 *   cov_{g,k} = sum_r (gt_g[r] - mean_g)(col_k[r] - mean_k) / (N - 1) for g < G — never sum x^2 - (sum x)^2 / N.
 *   corr[g][k] = cov_{g,k} / sqrt(var_g) / sqrt(var_k) (two divisions, as numpy), then clipped to [-1, 1].  A zero-variance column
 *   gives 0 / 0 = NaN in its entries exactly where numpy does (NaN survives the clip); nothing is raised for it.
 *   colstats [2, G + S]: row 0 the means, row 1 the variances (ddof 1).
 *   Rows are cut into chunks whose size is a function of (N, G, S) alone; each chunk's partial sums go to ws and are added in chunk
 *   order.  No float atomics, every sum has one order: repeated calls are bit-identical, whatever number of workgroups ran at once.
 * N >= 2, 1 <= G <= 16, S >= 1, N * (G + S) below 2^31; anything else is SRLZ_ERR_BAD_DESC, a null pointer SRLZ_ERR_NULL,
 * ws_bytes < srlz_gtc_workspace(N, G, S) SRLZ_ERR_WORKSPACE — all before any launch.  srlz_gtc_workspace returns 0 for a shape the
 * launcher rejects.
 * ------------------------------------------------------------------------------------------------------------ */
size_t srlz_gtc_workspace(int N, int G, int S);
int srlz_gtc_rows_f64(const double* gt /*[N,G]*/, const double* states /*[N,S]*/, int N, int G, int S, double* corr /*[G,G+S]*/,
                      double* colstats /*[2,G+S]: mean, variance (ddof 1)*/, void* ws, size_t ws_bytes, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation: the reward-prediction probe (csrc/reward_probe.hip).  Replaces the minibatch loop of
 *   outputs = model.rewardModel(inputs, next_inputs); _, preds = th.max(outputs, dim=1); loss = criterion(outputs, labels);
 *   loss.backward(); optimizer.step(); running_loss += ...; corrects[...] += ...          evaluation/predict_reward.py:106-141
 * with the classifier Linear(2S,4)-ReLU-Linear(4,4)-ReLU-Linear(4,2) on th.cat((state, next_state), dim=1)
 *                                                                                         models/forward_inverse.py:78-95
 * by ONE launch per training phase (srlz_reward_probe_fit) and ONE per validation phase (srlz_reward_probe_eval).
 *   states [N, S] fp32 and labels [N] int32 (class 1 where the label is 1, class 0 otherwise) stay on the device for the whole run.
 *   idx [n, B] int32 on the device, idx_host the SAME table on the host: every entry is checked there against [0, N - 2] before
 *   anything is launched (SRLZ_ERR_BAD_DESC).  Row b of minibatch s is the 2S floats at states + idx[s][b] * S, i.e. the rows i and
 *   i + 1 — the concatenation is never written.
 *   params / m / v: 4 * 2S + 34 floats each in state_dict order (reward_net.0.weight [4, 2S], 0.bias, 2.weight [4, 4], 2.bias,
 *   4.weight [2, 4], 4.bias).
 *   running_loss [1] fp64 and counts [5] int64 (correct, correct of class 0, of class 1, rows of class 0, of class 1) are ADDED TO:
 *   the caller zeroes them where a phase begins.  Argmax ties go to class 0, as th.max does.
 * fit: n_steps consecutive Adam steps (torch's defaults are the caller's to pass; no weight decay, no amsgrad; the arithmetic of
 *   srlz_adam_step) by one workgroup that keeps params, m and v in LDS from the first step to the last.  Step s uses the bias
 *   corrections of t = t0 + s + 1 (t0: the Adam steps already taken).  Forward in fp32, cross-entropy as the mean over B in
 *   log-sum-exp form, every sum over rows in one order that depends on (S, B) alone (rows are processed in chunks of
 *   srlz_reward_probe_chunk_rows(S)), running_loss += (sum of the row losses / B) * B per step in fp64.  step_loss (may be NULL)
 *   receives the n_steps mean losses in fp64.  No float atomics; n_steps in one call and n_steps calls of one step leave the same
 *   bits in params, m, v, running_loss and counts.  S must lie in [1, 512] (SRLZ_ERR_BAD_DESC): four copies of the parameters and
 *   a row chunk have to fit in LDS.
 * eval: the same forward over n_batches * B independent rows by many workgroups, the row loss in fp64; per-workgroup sums go to
 *   ws (srlz_reward_probe_eval_workspace(n_batches, B) bytes) and are added in workgroup order by the workgroup that finishes
 *   last (`ticket`: one zeroed unsigned the kernel leaves zeroed, as in srlz_episode_prior_fwd).  params are only read.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_reward_probe_chunk_rows(int S); /* rows of a chunk; 0 for an S the launchers reject */
int srlz_reward_probe_fit(const float* states /*[N,S]*/, const int* labels /*[N]*/, int N, int S, const int* idx /*[n_steps,B]*/,
                          const int* idx_host /*[n_steps,B]*/, int n_steps, int B, float* params, float* m, float* v, int t0, double lr,
                          double beta1, double beta2, double eps, double* running_loss /*[1]*/, long long* counts /*[5]*/,
                          double* step_loss /*[n_steps] or NULL*/, srlz_stream_t stream);
size_t srlz_reward_probe_eval_workspace(int n_batches, int B);
int srlz_reward_probe_eval(const float* states /*[N,S]*/, const int* labels /*[N]*/, int N, int S, const int* idx /*[n_batches,B]*/,
                           const int* idx_host /*[n_batches,B]*/, int n_batches, int B, const float* params, double* running_loss /*[1]*/,
                           long long* counts /*[5]*/, void* ws, size_t ws_bytes, unsigned* ticket, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation: decoded tensors into pictures (csrc/latent.hip).  Replaces, per shown image,
 *   img = detachToNumpy(net_out)[0].T; img = deNormalize(img, mode="image_net"); return img[:, :, ::-1]
 *                                                                                         evaluation/enjoy_latent.py:36-39
 * with deNormalize = x[..., c] *= std[c]; x[..., c] += mean[c]; np.clip(x, 0, 1)           preprocessing/utils.py:54-66
 * dec [N, 3, W, H] is the decoder's output in the reference's tensor layout (W-major planes).
 *   srlz_decoded_to_bgr: img [N, H, W, 3] fp32 with img[i][y][x][2 - c] = clip(fadd(fmul(dec[i][c][x][y], std[c]), mean[c]), 0, 1),
 *   std = (0.229, 0.224, 0.225) and mean = (0.485, 0.456, 0.406) as fp32.  The product and the sum are rounded separately (no fma):
 *   the result has the bits of the numpy expression.  A NaN stays a NaN, as in np.clip.
 *   srlz_decoded_to_sheet_u8: the same pictures as bytes, (uint8) rintf(fmul(v, 255)) with v the value above (round half to even:
 *   np.rint(v * np.float32(255)).astype(np.uint8); a NaN gives 0), tiled into ONE sheet [sheet_h, sheet_w, 3]: picture i at tile
 *   (i / cols, i % cols) of a grid of rows = ceil(n / cols) by cols tiles, `gap` pixels of `fill` between the tiles and around the
 *   grid, the empty tiles of the last row `fill` too.  rgb != 0 keeps the channel order R, G, B, rgb == 0 writes B, G, R.  Every
 *   byte of the sheet is written exactly once.  sheet_h = rows * h + (rows + 1) * gap and sheet_w = cols * w + (cols + 1) * gap.
 * Both are transposes staged through LDS (reads and writes coalesced), any w and h.  n, w, h, cols >= 1, gap >= 0, 0 <= fill <= 255,
 * n * 3 * w * h and the sheet's byte count below 2^31, sheet_h and sheet_w as above; anything else is SRLZ_ERR_BAD_DESC, a null
 * pointer SRLZ_ERR_NULL — all before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_decoded_to_bgr(const float* dec /*[N,3,W,H]*/, int n, int w, int h, float* img /*[N,H,W,3]*/, srlz_stream_t stream);
int srlz_decoded_to_sheet_u8(const float* dec /*[N,3,W,H]*/, int n, int w, int h, int cols, int gap, int fill, int rgb,
                             unsigned char* sheet /*[sheet_h,sheet_w,3]*/, int sheet_h, int sheet_w, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * PCA baseline: sklearn's IncrementalPCA in fp64 through a Gram matrix (csrc/pca.hip).  Replaces, per minibatch,
 *   ipca.partial_fit(toNumpyMatrix(obs_var))      srl_baselines/pca.py:107-108   (one LAPACK SVD of a (k + bs + 1) x D matrix)
 *   ipca.transform(toNumpyMatrix(obs_var))        srl_baselines/pca.py:117-118
 * State, all fp64 on the device: running mean [D] and var [D], basis [k, D] = singular_values_[:, None] * components_.
 * Frames come in one of two forms, EXACTLY ONE of x_u8 / x_f32 non-null: x_u8 = the loader's planar bytes [m, C, plane] with
 * norm_lut = the srlz_normalize_lut table (channel c reads row c % 3; C = D / plane in {3, 6, 9}), or x_f32 [m, D].
 * The matrix A sklearn decomposes (sklearn 1.7 decomposition/_incremental_pca.py:343-360, partial_fit: "Whitening" ... np.vstack) is never
 * written: first minibatch (first != 0) A = X - bmean, m rows; later A = [ basis ; X - bmean ; corr ], r = k + m + 1 rows.
 * Every sum has one order and there are no float atomics: repeated calls are bit-identical.
 * Rejected before any launch (SRLZ_ERR_BAD_DESC, text in srlz_last_error): m < 1, k < 1, k > D, k > m on the first minibatch, more
 * than 65535 output tiles of 16 x 16; a missing pointer is SRLZ_ERR_NULL, a short workspace SRLZ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------------------------ */
/* Bytes of partials for the Gram matrix of a `rows`-row A (srlz_pca_gram) / for srlz_pca_transform; 0 for a rejected shape. */
size_t srlz_pca_workspace(int rows, int D);
size_t srlz_pca_transform_workspace(int M, int k, int D);
/* sklearn.utils.extmath._incremental_mean_and_var (utils/extmath.py:1064-1187, called at _incremental_pca.py:335) per column, and what partial_fit derives from it:
 * mean / var [D] are updated in place from n_seen samples to n_seen + m (n_seen == 0: their contents are not read);
 * bmean [D] = the batch mean (np.mean(X, axis=0)); corr [D] = sqrt(n_seen / (n_seen + m) * m) * (mean_old - bmean), the
 * mean_correction row (zeros on the first minibatch). */
int srlz_pca_stats(const uint8_t* x_u8, const float* x_f32, const float* norm_lut, int plane, int m, int D, long long n_seen,
                   double* mean, double* var, double* bmean, double* corr, srlz_stream_t stream);
/* G [r, r] = A Aᵀ, exactly symmetric — what replaces linalg.svd(X, full_matrices=False) of partial_fit (_incremental_pca.py:362): the eigenpairs (w, u) of G
 * give S = sqrt(w) and S_i V_i = u_iᵀ A.  v_mfma_f64_16x16x4_f64 over the lower triangle of 16 x 16 tiles, D split over
 * workgroups, partials in ws summed in chunk order.  ws_bytes >= srlz_pca_workspace(r, D). */
int srlz_pca_gram(const double* basis /*[k,D]*/, int k, int first, const uint8_t* x_u8, const float* x_f32, const float* norm_lut,
                  int plane, int m, const double* bmean /*[D]*/, const double* corr /*[D]*/, int D, double* G /*[r,r]*/, void* ws,
                  size_t ws_bytes, srlz_stream_t stream);
/* out [k, D] = W [k, r] A (W = the k leading eigenvectors as rows): the new basis S·V.  out must not be the basis being read. */
int srlz_pca_project(const double* W /*[k,r]*/, const double* basis /*[k,D]*/, int k, int first, const uint8_t* x_u8,
                     const float* x_f32, const float* norm_lut, int plane, int m, const double* bmean, const double* corr, int D,
                     double* out /*[k,D]*/, srlz_stream_t stream);
/* IncrementalPCA.transform (sklearn decomposition/_base.py:116-145: (X - mean_) @ components_.T): states [M, k] fp32 =
 * (X - mean) (basis / S)ᵀ accumulated in fp64; a component with S_i <= 0 gives zeros.  ws_bytes >= srlz_pca_transform_workspace. */
int srlz_pca_transform(const uint8_t* x_u8, const float* x_f32, const float* norm_lut, int plane, int M, const double* mean /*[D]*/,
                       const double* basis /*[k,D]*/, const double* S /*[k]*/, int k, int D, float* states /*[M,k]*/, void* ws,
                       size_t ws_bytes, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deployment encoder (csrc/infer.hip): camera frames to states in four launches.  Replaces, per call of
 *   model.getStates(obs) in eval mode                                  models/models.py:25-30, 131-139; autoencoders.py:107-108
 * the three encoder blocks  Conv2d, BatchNorm2d, ReLU, MaxPool2d(3, 2)  models/models.py:47-63
 * each as ONE launch,  pooled = maxpool3x3s2(relu(conv(x) * scale + shift)),  scale / shift = the record srlz_bn_eval_params
 * produces (floats [128,192) and [192,256)), applied with the arithmetic of srlz_bn_relu_pool_fwd.  The raw convolution output is
 * never written.  The state head is the existing srlz_linear_fwd on the last block's [N,64,hp,wp] output.
 *   kind SRLZ_INFER_IN    7x7 stride 2 pad 3, c_in in {3, 6} -> 64   models/models.py:49-52   x: uint8 frames through norm_lut
 *   kind SRLZ_INFER_MID   3x3 stride 1 pad 1, 64 -> 64               models/models.py:54-57   x: fp32 NHWC
 *   kind SRLZ_INFER_LAST  3x3 stride 2 pad 1, 64 -> 64               models/models.py:59-62   x: fp32 NHWC
 * hi / wi are the two spatial sizes of the tensor the convolution sees (the reference's [B,C,D1,D2]: D1 = hi).  The byte input of
 * kind IN is addressed by ELEMENT strides: element (n, c, y, x) is byte n*stride_n + c*stride_c + y*stride_y + x*stride_x, and
 * channel c reads row c % 3 of the srlz_normalize_lut table (preprocessing/utils.py:20-32), as srlz_conv1_fwd_u8 does.  The reference's
 * planar [N,C,W,H] tensor (strides C*hi*wi, hi*wi, wi, 1) and a camera's [N,H,W,C] frames (hi = W, wi = H; strides H*W*C, 1, C, W*C:
 * the spatial swap of preprocessing/data_loader.py:255 as a stride choice) are the same kernel, no layout pass, identical bits.
 * A 64-channel input is contiguous NHWC and its strides say so (hi*wi*64, 1, wi*64, 64).
 * Output: pooled [N,hp,wp,64], or with out_nchw [N,64,hp,wp] (flat c*hp*wp + h*wp + w: what Linear(2304, S) reads), where
 * hc = (hi + 2 pad - k) / stride + 1 and hp = (hc + 2 pool_pad - 3) / 2 + 1, the same for the widths.  Any map size, rectangular
 * included.  No float atomics; every output's sum has one order that depends on neither n nor the tile boundaries: two runs are
 * bit-identical and row i of a batch has the bits of that frame run alone.
 * Rejected before any launch with SRLZ_ERR_BAD_DESC (srlz_infer_block_supported says so first): an unknown kind, c_in outside the
 * table, a map whose convolution or pooled output would be empty, pool_pad / out_nchw outside {0, 1}, strides that make two elements
 * share an address (kind IN) or that are not the contiguous NHWC ones (MID, LAST), more than 2^31 - 1 tiles.
 * ------------------------------------------------------------------------------------------------------------ */
#define SRLZ_INFER_IN 0
#define SRLZ_INFER_MID 1
#define SRLZ_INFER_LAST 2
typedef struct {
  int n;          /* frames */
  int c_in;       /* 3 or 6 (IN), 64 (MID, LAST) */
  int hi, wi;     /* input map */
  int kind;       /* SRLZ_INFER_* */
  int pool_pad;   /* 0 or 1: models/models.py:52 (1), 57, 62 (0) */
  int out_nchw;   /* 1: [N,64,hp,wp] (autoencoders.py:107-108: x.view(x.size(0), -1) of the NCHW map) */
  long long stride_n, stride_c, stride_y, stride_x; /* input element strides */
} srlz_infer_block_desc;
int srlz_infer_block_supported(const srlz_infer_block_desc* d);
/* Sizes of the convolution output (never stored) and of the pooled map; any of the four pointers may be NULL.  Host only. */
int srlz_infer_block_out_dims(const srlz_infer_block_desc* d, int* hc, int* wc, int* hp, int* wp);
/* Edge of the square tile of POOLED outputs one workgroup owns (host only; tests size their multi-tile cases by it). */
int srlz_infer_tile(void);
/* The kernels' private copy of a Conv2d weight [64, c_in, k, k] (nn.Conv2d, models/models.py:49, 54, 59): floats it takes (0 for a
 * kind / c_in outside the table) and the packing launch. */
long long srlz_infer_packed_floats(int kind, int c_in);
int srlz_infer_pack_weights(const float* w_ref, float* wpack, int kind, int c_in, srlz_stream_t stream);
int srlz_infer_block(const void* x, const float* norm_lut /* kind IN only */, const float* wpack, const float* bnp, float* out,
                     const srlz_infer_block_desc* d, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deployment decoder (csrc/infer_dec.hip): states to camera frames in six launches.  Replaces, per call of
 *   srl_model.decode(state) in eval mode + deNormalize        evaluation/enjoy_latent.py:21-39; autoencoders.py:111-118; vae.py:68-75
 * the decoder stack  ConvTranspose2d, BatchNorm2d, ReLU (x4), ConvTranspose2d      models/models.py:65-83
 * each layer as ONE launch.  decoder_fc is the existing srlz_linear_fwd, whose [N,2304] output viewed [N,64,6,6] kind FIRST reads.
 *   kind SRLZ_INFER_DEC_FIRST  3x3 stride 2, 64 -> 64, out = 2 in + 1   models/models.py:67-69   x: fp32 [N,64,hi,wi]
 *   kind SRLZ_INFER_DEC_MID    3x3 stride 2, 64 -> 64, out = 2 in + 1   models/models.py:71-81   x: fp32 NHWC
 *   kind SRLZ_INFER_DEC_OUT    4x4 stride 2, 64 -> c_out in {3, 6}, out = 2 in + 2   models/models.py:83   x: fp32 NHWC
 * FIRST / MID (srlz_infer_dec_block):  out = relu((convT(x) + bias) * scale + shift), fp32 NHWC [N,2hi+1,2wi+1,64]; scale / shift =
 * the record of srlz_bn_eval_params (floats [128,192) and [192,256)), applied with the expression of srlz_infer_block behind the bias.
 * The raw ConvTranspose output is never written.
 * OUT (srlz_infer_dec_out): out_u8 = 0 writes the reference's decode tensor, fp32 [N,c_out,ho,wo]; out_u8 = 1 writes the picture as
 * BYTES addressed by four element strides, element (n, c, y, x) of that tensor at byte n*out_stride_n + c*out_stride_c +
 * y*out_stride_y + x*out_stride_x:
 *   v = clip(fadd(fmul(d, std[c % 3]), mean[c % 3]), 0, 1), byte = (uint8) rintf(fmul(v, 255)), NaN -> 0      preprocessing/utils.py:54-66
 * (the arithmetic of srlz_decoded_to_sheet_u8).  The reference's planar [N,C,W,H] (strides C*ho*wo, ho*wo, wo, 1) and a camera's
 * [N,H,W,C] frames (ho = W, wo = H; strides H*W*C, 1, C, W*C: byte (n,y,x,c) of a frame is decoded[n][c][x][y]) are the same kernel;
 * bgr = 1 stores channel c of each camera (group of three) at 2 - c % 3.  The out strides are ignored for fp32 output.
 * The input strides state the layout the kernel reads and must be the contiguous ones: [N,64,hi,wi] (64*hi*wi, hi*wi, wi, 1) for
 * FIRST, NHWC (hi*wi*64, 1, wi*64, 64) for MID and OUT.  Weights: nn.ConvTranspose2d's [64, c_out, k, k].
 * No atomics; every output's sum has one order that depends on neither n nor the tile boundaries: two runs are bit-identical, row i
 * of a batch has the bits of state i decoded alone, and the bytes are exactly the expression above on the fp32 output.
 * Rejected before any launch with SRLZ_ERR_BAD_DESC (srlz_infer_dec_supported says so first): an unknown kind, c_in != 64, c_out
 * outside 64 / {3, 6}, an empty map, input strides other than the contiguous ones, output byte strides under which two elements share
 * an address, out_u8 on a block kind, more than 2^31 - 1 tiles or a frame beyond 32-bit byte offsets.
 * ------------------------------------------------------------------------------------------------------------ */
#define SRLZ_INFER_DEC_FIRST 0
#define SRLZ_INFER_DEC_MID 1
#define SRLZ_INFER_DEC_OUT 2
typedef struct {
  int n;          /* states */
  int c_in;       /* 64 */
  int c_out;      /* 64 (FIRST, MID), 3 or 6 (OUT) */
  int hi, wi;     /* input map */
  int kind;       /* SRLZ_INFER_DEC_* */
  int out_u8;     /* OUT only: 1 = bytes by the out strides, 0 = fp32 [N,c_out,ho,wo] */
  int bgr;        /* bytes only: 1 = reverse the three channels of each camera */
  long long in_stride_n, in_stride_c, in_stride_y, in_stride_x;     /* input element strides (checked) */
  long long out_stride_n, out_stride_c, out_stride_y, out_stride_x; /* byte output element strides */
} srlz_infer_dec_desc;
int srlz_infer_dec_supported(const srlz_infer_dec_desc* d);
/* Size of the output map: 2 hi + 1 (FIRST, MID), 2 hi + 2 (OUT), the same for the widths; either pointer may be NULL.  Host only. */
int srlz_infer_dec_out_dims(const srlz_infer_dec_desc* d, int* ho, int* wo);
/* Edge of the square tile of CELLS one workgroup of that kind owns (a cell = one input position and the 2 x 2 outputs under it; the
 * cell grid of an hi x wi map is (hi + 1) x (wi + 1)); 0 for an unknown kind.  Host only; tests size their multi-tile cases by it. */
int srlz_infer_dec_tile(int kind);
/* The kernels' private copy of a ConvTranspose2d weight [64, c_out, k, k]: floats it takes (0 outside the table), the packing launch. */
long long srlz_infer_dec_packed_floats(int kind, int c_out);
int srlz_infer_dec_pack_weights(const float* w_ref, float* wpack, int kind, int c_out, srlz_stream_t stream);
int srlz_infer_dec_block(const float* x, const float* wpack, const float* bias /*[64]*/, const float* bnp, float* out,
                         const srlz_infer_dec_desc* d, srlz_stream_t stream);
int srlz_infer_dec_out(const float* x, const float* wpack, const float* bias /*[c_out]*/, void* out, const srlz_infer_dec_desc* d,
                       srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deployment dynamics (csrc/rollout.hip): states and plans to final states and returns in ONE launch.  Replaces, per step of a
 * controller that scores candidate action sequences on the learned state,
 *   forwardModel: state + forward_net(cat(state, onehot(action)))          models/forward_inverse.py:21-31
 *   rewardModel:  reward_net(cat(state, next_state)), Linear-ReLU-Linear-ReLU-Linear   models/forward_inverse.py:78-95
 * (six launches of the training kernels a step).  R = N * K independent rows (environment n, candidate plan k), T sequential steps;
 * per row, s_0 = states[n], a_t = plans[n][k][t]:
 *   d_t     = fl(fl(Wf[:, :S] . s_t + Wf[:, S + a_t]) + bf)       the one-hot selects a column, it is never materialised
 *   s_{t+1} = fl(s_t + d_t)                                        the residual add rounded separately, as srlz_linear_fwd_res does
 *   l_t     = W3 . relu(W2 . relu(W1 . [s_t ; s_{t+1}] + b1) + b2) + b3
 *   ret    += fl(g_t * softmax(l_t)[1]);  g_0 = 1, g_{t+1} = fl(g_t * gamma);  softmax(l)[1] = 1 / (1 + exp(l[0] - l[1]))
 * states fp32 [N,S]; plans int32 [N,K,T] (plan_env_stride = K * T) or one [K,T] shared by every environment (plan_env_stride = 0,
 * nothing is copied); the weights in the reference's own layouts, read in place at every call: forward_net.weight wf [S,S+A], bias bf
 * [S], reward_net.0/2/4 w1 [H,2S], b1 [H], w2 [H,H], b2 [H], w3 [2,H], b3 [2].  The six reward-head pointers are all given or all
 * NULL; NULL means no reward work, and then returns and reward_logits must be NULL too (and H, n_rewards are not looked at).
 * Outputs, each optional (NULL) except the first: final_states [N,K,S] = s_T; returns [N,K]; trajectory [N,K,T,S], entry t = s_{t+1};
 * reward_logits [N,K,T,2].
 * fp32 throughout, the contractions over S on v_mfma_f32_32x32x2_f32; a tile of 32 rows stays in LDS from step 0 to step T-1.  No
 * atomics, and every sum's order depends on (S, A, H) alone: two runs are bit-identical; a call of T steps leaves the bits of T calls
 * of one step each fed the previous call's final_states (trajectory, reward_logits); a row's outputs do not depend on the other rows
 * of the call or on its place in it; shared plans give the bits of the same plans tiled.
 * An action outside [0, A) is never read through: from that step on the row's states, logits and return are NaN; its earlier steps
 * and every other row are untouched.
 * Limits (srlz_rollout_supported; the state tile, the partial blocks of layer 1 and the small operands take 115 KB of the 160 KB of
 * LDS at the limits, the forward model's accumulators 32 registers a wave): 1 <= S <= 512, 1 <= A <= 65536, 1 <= H <= 32,
 * n_rewards == 2.  Outside them, N, K or T < 1, N * K above 2^31 - 33, a plan stride other than 0 or K * T, a partly given reward
 * head or reward outputs without one: SRLZ_ERR_BAD_DESC before any launch, nothing written; a missing required pointer SRLZ_ERR_NULL.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_rollout_supported(int S, int A, int H, int n_rewards);
/* Rows one workgroup owns (host only; tests size their multi-tile cases by it). */
int srlz_rollout_tile(void);
int srlz_rollout(const float* states, const int* plans, long long plan_env_stride, const float* wf, const float* bf,
                 const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                 float* final_states, float* returns, float* trajectory, float* reward_logits, int N, int K, int T, int S, int A,
                 int H, int n_rewards, float gamma, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deployment planner (csrc/plan.hip): a categorical cross-entropy method (CEM) over discrete action sequences on the dynamics above,
 * ONE launch per iteration, enqueued back to back on the caller's stream with no host synchronisation between them; no plan ever
 * exists on the host.  N environments, K plans each, horizon T, A actions, I = iterations, E = elites, integer sharpness Q, a 64-bit
 * seed.  Everything is integer arithmetic except the returns:
 *   table   cum[n][t][a] (uint32) = inclusive prefix sum over a of integer weights w[n][t][a] >= 0.  Iteration 0: w = 1 (init_weights
 *           NULL), or the caller's init_weights, uint32 [N,T,A] (init_env_stride = T * A) or one [T,A] for every environment (stride
 *           0); the caller guarantees a positive total below 2^32 in every (n, t) row.
 *   sample  the action of (iteration i, environment n, plan k, step t): u = word t & 3 of Philox4x32-10 with key (seed & 0xffffffff,
 *           seed >> 32) and counter (t >> 2, k, n, i); target = (uint64(u) * cum[n][t][A-1]) >> 32; the first a with
 *           cum[n][t][a] > target.  A sample depends on (seed, i, n, k, t) and its table row alone — not on N, K or the launch.
 *   score   each plan rolled exactly as srlz_rollout rolls it (the same text, csrc/rollout_tile.h): the return, discounted by gamma,
 *           has the bits srlz_rollout leaves for the same plan.  The reward head is required.
 *   select  key = the return, NaN read as -inf; order by key descending, then k ascending; the first E plans are the elites.
 *   best    iteration 0 stores its top plan and that plan's true return (NaN included); a later iteration replaces them only if its
 *           top key is strictly greater.
 *   refit   count[t][a] = elites with action a at step t; w[t][a] = 1 + Q * count[t][a]; cum = its prefix sum.  No momentum.
 * Outputs: best_plan int32 [N,T], best_return [N], cum uint32 [N,T,A] (the table after the last refit); with plans int32 [I,N,K,T]
 * and returns [I,N,K] (both or neither) the whole population is kept.
 * Workspace: srlz_plan_workspace(N, K, T, keep_population) bytes (0 for a refused shape), 16-byte aligned.  Its first N uint32 are the
 * environments' tickets: zeroed on the stream when the call starts, and zero again when its last launch has ended.
 * Per launch N * ceil(K / 32) workgroups; the workgroup that finishes an environment last (an integer ticket, no spinning, no grid
 * barrier) does select, best and refit for it.  Integer LDS atomics for the counts, no float atomics: two runs are bit-identical.
 * Limits (srlz_plan_supported): those of srlz_rollout_supported and A <= 256, 1 <= K <= 1024, 1 <= T <= 32.  Outside them, a missing
 * reward head, N < 1, E outside [1, K], I < 1, Q outside [0, 4096], an init stride other than 0 or T * A, half a population:
 * SRLZ_ERR_BAD_DESC before anything is enqueued, nothing written; a missing required pointer SRLZ_ERR_NULL, a short workspace
 * SRLZ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_plan_supported(int S, int A, int H, int n_rewards, int K, int T);
size_t srlz_plan_workspace(int N, int K, int T, int keep_population);
int srlz_plan_cem(const float* states, const float* wf, const float* bf, const float* w1, const float* b1, const float* w2,
                  const float* b2, const float* w3, const float* b3, const unsigned* init_weights, long long init_env_stride,
                  int* best_plan, float* best_return, unsigned* cum, int* plans, float* returns, void* ws, size_t ws_bytes, int N, int K,
                  int T, int S, int A, int H, int n_rewards, int iterations, int elites, int sharpness, float gamma,
                  unsigned long long seed, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Goal-distance scores (csrc/rollout_tile.h, instantiated in rollout.hip and plan.hip): "drive the learned state to the state of this
 * goal picture".  The rollout and the planner above with one more term per step, composed on the same reference lines —
 * forwardModel (models/forward_inverse.py:21-31) for the states, rewardModel (:78-95) for prob_t when a reward head is given.
 * Per row, a goal goal[n] (fp32 [S]), a weight w > 0 and a mode; at step t, once s_{t+1} is in the tile:
 *   d_t    = sum_j fl(s_{t+1}[j] - goal[j])^2                            fp32, the order below
 *   c_t    = d_t (goal_mode 0, running)  |  d_t if t == T-1 else 0 (goal_mode 1, final)
 *   term_t = reward head given ?  fl(prob_t - fl(w * c_t))  :  -fl(w * c_t)     prob_t = 1 / (1 + exp(l0 - l1)) as above
 *   ret    = fl(ret + fl(g_t * term_t));   g_0 = 1, g_{t+1} = fl(g_t * gamma)     (g advances with or without a reward head)
 * returns [N,K] holds ret: the score, and the planner's key under the rule above (NaN read as -inf).  goal_dist [N,K,T] (optional)
 * holds d_t of every step in both modes.
 * Order of d_t, a function of S alone: 16 partial sums, partial q over j = q, q + 16, q + 32, .. ascending, each
 * p = fma(e, e, p) from p = 0 with e = fl(s_{t+1}[j] - goal[j]); then d_t = ((p_0 + p_1) + p_2) + .. + p_15, each add rounded.  (A partial
 * whose q >= S is 0.)  No atomics: two runs are bit-identical, a row's outputs do not depend on the other rows, and trajectory,
 * final_states and reward_logits are the bits srlz_rollout leaves.  A row that met an action outside [0, A) has NaN d_t from that
 * step on (its states are NaN), and a NaN ret.
 * goal: fp32 [N,S] (goal_env_stride = S) or one [S] shared by every environment (goal_env_stride = 0, nothing is copied).
 * The six reward pointers are all given or all NULL; NULL: the score is the goal term alone, returns is still allowed,
 * reward_logits must be NULL.  The planner's sampling, tickets, select, best and refit are those of srlz_plan_cem; only the key's
 * source differs.  srlz_plan_goal_workspace equals srlz_plan_workspace.
 * Limits (srlz_rollout_goal_supported / srlz_plan_goal_supported; has_reward = 0: H and n_rewards are not looked at): those of
 * srlz_rollout_supported / srlz_plan_supported — the 16 x 33 partials add 2.1 KB of LDS: 117 KB (rollout) and 157.8 KB (planner at
 * S = 512, H = 32, T = 32, A = 256, K = 1024) of 160.  Outside them, a partly given head, goal_weight not finite or not > 0,
 * goal_mode other than 0 or 1, a goal stride other than 0 or S, and whatever the call without a goal refuses: SRLZ_ERR_BAD_DESC
 * before any launch, nothing written; a missing required pointer (goal among them) SRLZ_ERR_NULL.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_rollout_goal_supported(int S, int A, int H, int n_rewards, int has_reward);
int srlz_rollout_goal(const float* states, const int* plans, long long plan_env_stride, const float* wf, const float* bf,
                      const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                      float* final_states, float* returns, float* trajectory, float* reward_logits, int N, int K, int T, int S, int A,
                      int H, int n_rewards, float gamma, const float* goal, long long goal_env_stride, float goal_weight,
                      int goal_mode, float* goal_dist, srlz_stream_t stream);
int srlz_plan_goal_supported(int S, int A, int H, int n_rewards, int has_reward, int K, int T);
size_t srlz_plan_goal_workspace(int N, int K, int T, int keep_population);
int srlz_plan_cem_goal(const float* states, const float* wf, const float* bf, const float* w1, const float* b1, const float* w2,
                       const float* b2, const float* w3, const float* b3, const unsigned* init_weights, long long init_env_stride,
                       int* best_plan, float* best_return, unsigned* cum, int* plans, float* returns, void* ws, size_t ws_bytes, int N,
                       int K, int T, int S, int A, int H, int n_rewards, int iterations, int elites, int sharpness, float gamma,
                       unsigned long long seed, const float* goal, long long goal_env_stride, float goal_weight, int goal_mode,
                       srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deployment tree search (csrc/beam.hip): exact enumeration or a beam of width W over the discrete action sequences of the dynamics
 * above, ONE launch per level of the tree, enqueued back to back on the caller's stream with no host synchronisation between them;
 * no plan and no frontier ever exists on the host.  Composed on the same reference lines as srlz_rollout — forwardModel
 * (models/forward_inverse.py:21-31) for every expanded node's state, rewardModel (:78-95) for prob_t when a reward head is given.
 * N environments, horizon T, beam width W >= 1, A actions, gamma; optionally the goal of srlz_rollout_goal (goal == NULL: no goal).
 * Without a goal the reward head is required; with one it is optional.  Per environment, for levels t = 0 .. T-1:
 *   frontier  level t has F_t nodes; F_0 = 1: the environment's state, ret = 0, g_0 = 1.
 *   expand    every node f by every action a: child c = f * A + a, C_t = F_t * A children.  A child's state is one forward step of
 *             its parent's state with the bits of srlz_rollout's step; its ret continues its parent's ret with this step's term under
 *             the arithmetic of srlz_rollout (no goal: ret = ret + g_t * prob_t as srlz_rollout evaluates it) or srlz_rollout_goal
 *             (fl(w * c_t), fl(prob_t - .), fl(g_t * term_t), fl(ret + .), each rounded on its own; in mode final c_t = d_t at level
 *             T-1 alone, 0 before); g_{t+1} = fl(g_t * gamma).  The ret of every leaf is, bit for bit, what srlz_rollout (or
 *             srlz_rollout_goal with the same goal, weight and mode) returns for that leaf's T-step plan.
 *   select    (t < T-1)  C_t <= W: the next frontier is all children in child-index order, F_{t+1} = C_t.  Otherwise key = ret, NaN
 *             read as -inf (and -0 as +0); order by key descending, then c ascending; the first W children in that order are the
 *             next frontier, in that order, F_{t+1} = W.
 *   leaves    (t = T-1)  all L = F_{T-1} * A children, in child-index order.  best = the leaf with the greatest key, ties to the
 *             lowest c; best_return = its true ret (NaN included); best_plan = its actions, read back through the parents.
 * With W >= A^(T-1) nothing is ever pruned: the leaves are all A^T plans in lexicographic order (a_0 the most significant digit) and
 * best is the optimum under the model — the argmax srlz_rollout over the enumeration gives, at A + A^2 + .. + A^T forward steps in
 * place of T * A^T.
 * Outputs: best_plan int32 [N,T], best_return [N]; optional leaf_plans int32 [N,L,T] with leaf_returns [N,L] (both or neither),
 * L = srlz_beam_leaves(W, A, T) (0 outside the limits).
 * Workspace: srlz_beam_workspace(N, W, T, S, A) bytes (0 for a refused shape), 16-byte aligned: the environments' tickets (N uint32,
 * zeroed on the stream when the call starts and zero again when its last launch has ended), two return buffers [N,L], the
 * frontiers [T-1,N,W] and two child-state buffers [N,C_{T-2},S] used in turn — a selected child's state is read in place by the
 * next level, nothing is copied; the last level writes no states.
 * Per level N * ceil(C_t / 32) workgroups: a tile of 32 children never straddles two environments.  On a level that prunes, and on
 * the last, the workgroup that finishes an environment last (the integer ticket of srlz_plan_cem, no spinning, no grid barrier) sorts
 * 64-bit (key, c) words in LDS with integer compares alone, or takes their minimum.  No float atomics: two runs are bit-identical.
 * Limits (srlz_beam_supported; has_reward = 0: H and n_rewards are not looked at): those of srlz_rollout_supported /
 * srlz_rollout_goal_supported, and 1 <= T <= 32, W >= 1, W * A <= 8192.  Outside them, N < 1 or N * L above 2^31 - 33, a partly given
 * head, no head and no goal, half the leaves, or a goal argument srlz_rollout_goal would refuse: SRLZ_ERR_BAD_DESC before anything is
 * enqueued, nothing written; a missing required pointer SRLZ_ERR_NULL, a short workspace SRLZ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_beam_supported(int S, int A, int H, int n_rewards, int has_reward, int W, int T);
size_t srlz_beam_workspace(int N, int W, int T, int S, int A);
int srlz_beam_leaves(int W, int A, int T);
int srlz_beam_search(const float* states, const float* wf, const float* bf, const float* w1, const float* b1, const float* w2,
                     const float* b2, const float* w3, const float* b3, int* best_plan, float* best_return, int* leaf_plans,
                     float* leaf_returns, void* ws, size_t ws_bytes, int N, int W, int T, int S, int A, int H, int n_rewards,
                     float gamma, const float* goal, long long goal_env_stride, float goal_weight, int goal_mode,
                     srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The k-step error of the dynamics on a recorded sequence (csrc/horizon.hip; evaluation/predict_forward.py): the open-loop check of
 * forwardModel (models/forward_inverse.py:21-31) and, on the imagined pairs, rewardModel (:78-95).  Two launches.
 * srlz_horizon_rows.  A recorded sequence of N frames: states fp32 [N,S], actions int32 [N] (actions[i] leads from frame i to i + 1).
 * M rows; row r starts at frame starts[r] and has len[r] steps (int32 [M] both).  The caller's contract, not checked on the device:
 * 0 <= starts[r], 0 <= len[r] <= T and starts[r] + len[r] <= N - 1.  Row r is rolled as srlz_rollout rolls a row (the same text,
 * csrc/rollout_tile.h) from s_0 = states[starts[r]] with a_t = actions[starts[r] + t] for t < len[r]; at step t < len[r], with
 * x = states[starts[r] + t + 1], once s_{t+1} is in the tile:
 *   err[r,t]  = sum_j fl(s_{t+1}[j] - x[j])^2                    the imagined state against the recorded one
 *   base[r,t] = sum_j fl(states[starts[r]][j] - x[j])^2          "the state stays s_0" against the recorded one
 * both in the order of the goal distance above (16 partials, partial q an fma chain over j = q, q + 16, .. ascending, then
 * ((p_0 + p_1) + ..) + p_15), a function of S alone.  For t >= len[r], err and base are a quiet NaN and nothing of the sequence is
 * read; a row that met an action outside [0, A) inside its steps has NaN err (not base) from that step on.
 * Outputs err, base fp32 [M,T]; optional reward_logits [M,T,2] (needs the head) and trajectory [M,T,S], for t < len[r] the bits
 * srlz_rollout leaves for the same actions; their entries at t >= len[r] hold the row rolled on with action 0 and mean nothing.
 * The six reward pointers are all given or all NULL.  No atomics; a row's outputs do not depend on the other rows or on its place.
 * Limits (srlz_horizon_supported; has_reward = 0: H and n_rewards are not looked at): those of srlz_rollout_supported — the two
 * reductions' partials add 4.2 KB of LDS: 119 KB of 160 at S = 512, H = 32 — and 1 <= T <= 32, N >= 1, 1 <= M <= 2^31 - 33.
 * srlz_horizon_sums.  Per horizon t: count[t] (int64) = rows with len[r] > t; sum_err[t], sum_base[t] (fp64) over exactly those rows
 * (a NaN among them propagates); with reward_logits, labels (int32 [N], classes 0 / 1) and hits (int64 [T]) — all three or none —
 * hits[t] = those rows whose class (reward_logits[r,t,1] > reward_logits[r,t,0] ? 1 : 0: torch's argmax, a tie or a NaN is class 0)
 * equals labels[starts[r] + t], the reward stored at the transition's first frame.
 * Order of each fp64 sum, a function of (M, T) alone: partial k of 512 adds the values of its rows r = k, k + 512, k + 1024, .. in
 * ascending order from 0 (rows with len[r] <= t are skipped); then for h = 256, 128, .. 1: p[k] += p[k + h] for every k < h; the sum
 * is p[0].  No atomics: two runs are bit-identical.
 * Refused before any launch, nothing written: a partly given head (or half of logits / labels / hits), reward_logits without a
 * head, a shape outside the limits: SRLZ_ERR_BAD_DESC; a missing required pointer SRLZ_ERR_NULL.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_horizon_supported(int S, int A, int H, int n_rewards, int has_reward);
int srlz_horizon_rows(const float* states, const int* actions, const int* starts, const int* len, const float* wf, const float* bf,
                      const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float* err,
                      float* base, float* reward_logits, float* trajectory, int N, int M, int T, int S, int A, int H, int n_rewards,
                      srlz_stream_t stream);
int srlz_horizon_sums(const float* err, const float* base, const float* reward_logits, const int* labels, const int* starts,
                      const int* len, int M, int T, long long* count, double* sum_err, double* sum_base, long long* hits,
                      srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The forward head in closed form (csrc/dynfit.hip; srlz/dynfit.py, evaluation/predict_forward.py --fit): the normal equations of
 *   next_state = state + self.forward_net(th.cat((state, encodeOneHot(action, self.action_dim)), dim=1))
 *                                                                                         models/forward_inverse.py:16,30-31
 * under the MSE of losses/losses.py:forwardModelLoss, over M recorded transitions.  states fp32 [N,S], actions int32 [N]
 * (actions[i] leads from frame i to i + 1), starts int32 [M] on the device: transition m is the frame pair (i, i + 1), i = starts[m].
 * In fp64, with P = S + A + 1:
 *   z_i = [ (double)s_i[0..S) | onehot(a_i)[0..A) | 1 ]        y_i = (double)s_{i+1} - (double)s_i
 *   G [P,P] = sum_m z zᵀ          C [P,S] = sum_m z yᵀ
 * The conversions are exact and the subtraction is an fp64 one.  Neither [z | y] nor the one-hot block is ever in memory: a stage
 * of 32 transitions is built in LDS (coalesced loads of s_i and s_{i+1}) and its 16-wide column tiles feed
 * v_mfma_f64_16x16x4_f64, the MFMA's k index running over the transitions.  Only the lower triangle of G's 16 x 16 tiles and C are
 * computed.  An action outside [0, A) gives a zero one-hot block for its transition (the Python layer refuses it on the host).
 * Order of every sum, a function of (M, S, A) alone: the transitions are split into chunks of srlz_dynfit_chunk_rows(M, S, A)
 * consecutive entries of starts (a multiple of 32), one workgroup per chunk and group of 8 tiles; inside a chunk wave w of four
 * accumulates the quads of transitions w, w + 4, .. in ascending order, the four waves are added ((w0 + w1) + w2) + w3 and the
 * partial tile goes to ws; a second launch adds the partials in chunk order and writes G's upper triangle as a copy of the lower
 * one.  No atomics, plain vector stores: G is exactly symmetric, two calls leave identical bits, and every element of G and C is
 * written exactly once and nothing beyond them.
 * Limits (srlz_dynfit_supported): 1 <= S <= 512, the width of the dynamics kernels' state tile (srlz_rollout_supported), and
 * 1 <= A <= 64.  They bound the system at P <= 577 — 1887 output tiles, one launch's grid — which the host solves in fp64 in well
 * under a second, and they leave 8 chunks within the workspace cap at the largest shape.
 * Workspace: tiles * chunks * 2048 bytes, with at most 256 chunks and at most 16384 partial tiles: never more than 32 MiB, whatever
 * M.  srlz_dynfit_chunk_rows and srlz_dynfit_workspace are functions of the shapes alone and return 0 for a shape the launcher
 * rejects (M < 1 or an unsupported (S, A)).
 * starts_host is the SAME table on the host: every entry is checked there against [0, N - 2] before anything is launched, as
 * srlz_reward_probe_fit checks its table (the device copy is clamped to that range, so it never forms an address outside states).
 * Refused before any launch, nothing written: an unsupported (S, A), N < 2, M < 1, N * S >= 2^31, a start outside [0, N - 2]:
 * SRLZ_ERR_BAD_DESC; a missing pointer SRLZ_ERR_NULL; ws_bytes < srlz_dynfit_workspace(M, S, A) SRLZ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_dynfit_supported(int S, int A);
int srlz_dynfit_chunk_rows(int M, int S, int A);
size_t srlz_dynfit_workspace(int M, int S, int A);
int srlz_dynfit_gram(const float* states /*[N,S]*/, const int* actions /*[N]*/, const int* starts /*[M]*/,
                     const int* starts_host /*[M]*/, int N, int M, int S, int A, double* G /*[P,P]*/, double* C /*[P,S]*/, void* ws,
                     size_t ws_bytes, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The reward head fitted on a recording (csrc/headfit.hip; srlz/headfit.py, LatentDynamics.refit_reward,
 * evaluation/predict_forward.py --fit --fit-reward).  Replaces the reward part of the learner's minibatch loop,
 *   reward_pred = model.rewardModel(states, next_states); rewardModelLoss(...) -> nn.CrossEntropyLoss; loss.backward();
 *   optimizer.step()                                       models/learner.py:444-449, losses/losses.py:158
 * with the classifier Linear(2S,H)-ReLU-Linear(H,H)-ReLU-Linear(H,2) on th.cat((state, next_state), dim=1)
 *                                                                                         models/forward_inverse.py:78-95
 * by ONE launch per training epoch (srlz_headfit_fit) and ONE per validation phase (srlz_headfit_eval).  The general form of
 * srlz_reward_probe_* (H = 4), which keep their own bits.
 *   states [N, S] fp32 and labels [N] int32 (class 1 where the label is 1, class 0 otherwise: a compare, nothing is indexed by a
 *   label) stay on the device.  idx [n, B] int32 on the device, idx_host the SAME table on the host: every entry is checked there
 *   against [0, N - 2] before anything is launched; the device copy is clamped to that range as it is read, so no address outside
 *   states is ever formed.  Row b of minibatch s is the 2S floats at states + idx[s][b] * S, i.e. the rows i and i + 1 — the
 *   concatenation is never written; its label is labels[idx[s][b]].
 *   params / m / v / last_grad: srlz_headfit_n_params(S, H) = 2S*H + H + H*H + H + 2*H + 2 floats each in state_dict order
 *   (reward_net.0.weight [H, 2S], 0.bias, 2.weight [H, H], 2.bias, 4.weight [2, H], 4.bias).
 *   running_loss [1] fp64 and counts [5] int64 (correct, correct of class 0, of class 1, rows of class 0, of class 1) are ADDED TO.
 *   Argmax ties go to class 0, as th.max does.
 * fit: n_steps consecutive Adam steps (torch's defaults are the caller's to pass; the arithmetic of srlz_adam_step) in one launch
 *   of one persistent workgroup of 256 threads.  Parameters and gradient stay in LDS from the first step to the last; the Adam
 *   moments m and v stay in GLOBAL memory in state_dict order, read and written once per step (two more copies in LDS would halve
 *   the envelope).  Step s uses the bias corrections of t = t0 + s + 1.  Forward in fp32, cross-entropy as the mean over B in
 *   log-sum-exp form; no gradient into the states.  Rows are processed in chunks of srlz_headfit_chunk_rows(S, H).  Order of every
 *   sum, a function of (S, H, B) alone: layer 1 — 16 lanes per row, lane kk adds k = kk, kk + 16, .. ascending, then a butterfly
 *   over the 16 lanes (offsets 8, 4, 2, 1); layers 2 and 3 and their transposes — one thread per output, the index ascending from
 *   the bias; every parameter's gradient — one thread per element, rows in row order, chunk after chunk; the loss — per chunk, lane
 *   l of one wave adds rows l, l + 64 in fp64, then a butterfly, chunks in order.  running_loss += (sum of row losses / B) * B per
 *   step in fp64; step_loss (may be NULL) receives the n_steps mean losses; last_grad (may be NULL) the gradient of the LAST step.
 *   No float atomics, plain vector stores.  Two calls leave identical bits; n steps in one call and n calls of one step leave
 *   identical bits in params, m, v, running_loss, counts and step_loss.
 * eval: the same forward over n_batches * B independent rows, 64 per workgroup, the row loss in fp64; per-workgroup sums go to ws
 *   (srlz_headfit_eval_workspace(n_batches, B) bytes) and are added in workgroup order by the workgroup that finishes last
 *   (`ticket`: one zeroed unsigned the kernel leaves zeroed; no spinning, no grid barrier); counts by integer atomics.  params are
 *   only read.
 * Limits.  With K = 2S, HP = H rounded up to a multiple of 4, HPAD = HP | 4, the LDS image of the parameters holds
 *   PL = (K + H + 4) * HPAD + 4 floats (W1 as [k][HPAD], b1, W2 transposed, b2, W3, b3; pads zero) and a row of a chunk costs
 *   (K | 1) + 4 * HPAD + 7 floats (the row, its record d a1 | h1 | d a2 | h2 | dz, loss, flag, label).
 *   srlz_headfit_chunk_rows(S, H) = min(128, floor((40956 - 2 * PL - 512) / ((K | 1) + 4 * HPAD + 7))), and 0 where that is below 16
 *   or (S, H) lies outside [1, 512] x [1, 32];  srlz_headfit_supported(S, H) = srlz_headfit_chunk_rows(S, H) > 0.
 *   That accepts every S <= 200 with H <= 16 (S = 200, H = 16: 67,232 bytes of parameters and gradient, chunks of 48 rows,
 *   162,976 bytes in all), S <= 512 up to H = 4, S <= 489 up to H = 12, S <= 341 up to H = 16, S <= 256 up to H = 24 and
 *   S <= 201 at H = 32.
 * Refused before anything is enqueued, nothing written: an unsupported (S, H), N < 2, n < 1, B < 1, N * S >= 2^31, n * B >= 2^31,
 *   t0 < 0, an entry of idx_host outside [0, N - 2]: SRLZ_ERR_BAD_DESC; a missing pointer SRLZ_ERR_NULL; ws_bytes below
 *   srlz_headfit_eval_workspace: SRLZ_ERR_WORKSPACE.  srlz_headfit_eval_workspace returns 0 for n_batches < 1, B < 1 or 2^31 rows.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_headfit_supported(int S, int H);
long long srlz_headfit_n_params(int S, int H); /* 0 for S < 1 or H < 1 */
int srlz_headfit_chunk_rows(int S, int H);     /* rows of a chunk; 0 for a shape the launchers reject */
int srlz_headfit_fit(const float* states /*[N,S]*/, const int* labels /*[N]*/, int N, int S, int H, const int* idx /*[n_steps,B]*/,
                     const int* idx_host /*[n_steps,B]*/, int n_steps, int B, float* params, float* m, float* v, int t0, double lr,
                     double beta1, double beta2, double eps, double* running_loss /*[1]*/, long long* counts /*[5]*/,
                     double* step_loss /*[n_steps] or NULL*/, float* last_grad /*[P] or NULL*/, srlz_stream_t stream);
size_t srlz_headfit_eval_workspace(int n_batches, int B);
int srlz_headfit_eval(const float* states /*[N,S]*/, const int* labels /*[N]*/, int N, int S, int H, const int* idx /*[n_batches,B]*/,
                      const int* idx_host /*[n_batches,B]*/, int n_batches, int B, const float* params, double* running_loss /*[1]*/,
                      long long* counts /*[5]*/, void* ws, size_t ws_bytes, unsigned* ticket, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The inverse head fitted on a recording (csrc/invfit.hip; srlz/invfit.py, LatentDynamics.refit_inverse / action_accuracy,
 * evaluation/predict_forward.py --fit --fit-inverse).  Replaces the inverse part of the learner's minibatch loop,
 *   actions_pred = model.inverseModel(states, next_states)      models/forward_inverse.py inverseModel (:62-70): the head
 *                                                               nn.Linear(2S, A) on th.cat((state, next_state), dim=1)
 *   inverseModelLoss(...) -> nn.CrossEntropyLoss                losses/losses.py:117-129
 *   loss.backward(); optimizer.step()                           the learner's Adam loop (models/learner.py)
 * by ONE launch per training epoch (srlz_invfit_fit) and ONE per validation phase (srlz_invfit_eval): multinomial logistic
 * regression, z = W [s_i ; s_{i+1}] + b.  The shape of srlz_headfit_*, whose entry points and bits are unchanged.
 *   states [N, S] fp32 and labels [N] int32 (the action of frame i) stay on the device.  idx / idx_host: as srlz_headfit_fit takes
 *   them (every entry checked on the host against [0, N - 2], the device copy clamped as it is read).  Row b of minibatch s is the
 *   2S floats at states + idx[s][b] * S; its label is labels[idx[s][b]].  A label outside [0, A) indexes nothing: its row adds
 *   zero to the loss and to the gradient (the mean still divides by B) and is counted in `bad`.
 *   params / m / v / last_grad: srlz_invfit_n_params(S, A) = 2S*A + A floats each in state_dict order (inverse_net.weight [A, 2S],
 *   inverse_net.bias [A]).  running_loss [1] fp64 and counts [3 + 2A] int64 are ADDED TO; counts = rows, correct, bad, then
 *   support[A] (rows labelled a) and hits[A] (of which predicted a): rows = sum(support) + bad, correct = sum(hits), and
 *   hits[a] / support[a] is the recall of action a.  An argmax tie goes to the lowest class, as th.max does.
 * fit: n_steps consecutive Adam steps (the arithmetic of srlz_adam_step) in one launch of one persistent workgroup of 256 threads.
 *   Parameters and gradient stay in LDS from the first step to the last; the Adam moments m and v stay in GLOBAL memory in
 *   state_dict order, read and written once per step (two more copies in LDS would halve the envelope).  Step s uses the bias
 *   corrections of t = t0 + s + 1.  Forward in fp32, cross-entropy as the mean over B in log-sum-exp form; no gradient into the
 *   states.  Rows are processed in chunks of srlz_invfit_chunk_rows(S, A).  Order of every sum, a function of (S, A, B) alone:
 *   logits — 16 lanes per row, lane kk adds k = kk, kk + 16, .. ascending, then a butterfly over the 16 lanes (offsets 8, 4, 2, 1),
 *   then + bias; softmax — one thread per row, the maximum and e_j = exp(z_j - max) over j ascending, the e_j beside the label's
 *   added over j ascending and the label's added last; loss = log1p(others) where the label holds the maximum, else log(sum) -
 *   (z_label - max); dz_j = e_j / sum / B, the label's -(others) / sum / B; every parameter's gradient — one thread per element,
 *   rows in row order, chunk after chunk; the loss — per chunk, lane l of one wave adds rows l, l + 64 in fp64, then a butterfly,
 *   chunks in order.  running_loss += (sum of row losses / B) * B per step in fp64; step_loss (may be NULL) receives the n_steps
 *   mean losses; last_grad (may be NULL) the gradient of the LAST step.  No float atomics (support and hits are integer atomics
 *   in LDS), plain vector stores.  Two calls leave identical bits; n steps in one call and n calls of one step leave identical
 *   bits in params, m, v, running_loss, counts and step_loss.
 * eval: the same logits over n_batches * B independent rows, 64 per workgroup (16 at a time), the row loss in fp64 as
 *   max + log(sum_j exp(z_j - max)) - z_label, j ascending; per-workgroup sums (lane l = row l, a butterfly) go to ws
 *   (srlz_invfit_eval_workspace(n_batches, B) bytes) and are added in workgroup order by the workgroup that finishes last
 *   (`ticket`: one zeroed unsigned the kernel leaves zeroed; no spinning, no grid barrier); counts by integer atomics.  params
 *   are only read.
 * Limits: the LDS budget and nothing else.  With K = 2S, AP = A rounded up to a multiple of 4, APAD = AP | 4, the LDS image of the
 *   parameters holds (K + 1) * APAD floats (row k < K is W[:, k], row K the bias; pads zero and never written back), the gradient
 *   as many, the per-action counters 2 * APAD, Adam's table 512, and a row of a chunk costs (K | 1) + APAD + 3 floats (the row,
 *   its z / dz, loss, flag, label), within the 160 KB srlz_headfit_fit uses:
 *   srlz_invfit_chunk_rows(S, A) = min(128, floor((40444 - 2 * (K + 2) * APAD) / ((K | 1) + APAD + 3))), and 0 where that is below
 *   16, S < 1 or A < 2;  srlz_invfit_supported(S, A) = srlz_invfit_chunk_rows(S, A) > 0.
 *   That accepts S = 200 with A = 6 (chunks of 74 rows), S <= 501 up to A = 8, S <= 356 up to A = 16, S <= 225 up to
 *   A = 32, S <= 839 up to A = 4, and at S = 1 up to A = 1676.
 * Refused before anything is enqueued, nothing written: an unsupported (S, A), N < 2, n < 1, B < 1, N * S >= 2^31, n * B >= 2^31,
 *   t0 < 0, an entry of idx_host outside [0, N - 2]: SRLZ_ERR_BAD_DESC; a missing pointer SRLZ_ERR_NULL; ws_bytes below
 *   srlz_invfit_eval_workspace: SRLZ_ERR_WORKSPACE.  srlz_invfit_eval_workspace returns 0 for n_batches < 1, B < 1 or 2^31 rows.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_invfit_supported(int S, int A);
long long srlz_invfit_n_params(int S, int A); /* 2S*A + A; 0 for S < 1 or A < 2 */
int srlz_invfit_chunk_rows(int S, int A);     /* rows of a chunk; 0 for a shape the launchers reject */
int srlz_invfit_fit(const float* states /*[N,S]*/, const int* labels /*[N]*/, int N, int S, int A, const int* idx /*[n_steps,B]*/,
                    const int* idx_host /*[n_steps,B]*/, int n_steps, int B, float* params, float* m, float* v, int t0, double lr,
                    double beta1, double beta2, double eps, double* running_loss /*[1]*/, long long* counts /*[3 + 2A]*/,
                    double* step_loss /*[n_steps] or NULL*/, float* last_grad /*[P] or NULL*/, srlz_stream_t stream);
size_t srlz_invfit_eval_workspace(int n_batches, int B);
int srlz_invfit_eval(const float* states /*[N,S]*/, const int* labels /*[N]*/, int N, int S, int A, const int* idx /*[n_batches,B]*/,
                     const int* idx_host /*[n_batches,B]*/, int n_batches, int B, const float* params, double* running_loss /*[1]*/,
                     long long* counts /*[3 + 2A]*/, void* ws, size_t ws_bytes, unsigned* ticket, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The robotic priors (csrc/robotic.hip): roboticPriorsLoss of the reference, losses/losses.py:62-99 — temporal coherence,
 * causality, proportionality and repeatability of one minibatch of states, over the pair lists of losses/utils.py:75-116
 * (findPriorsPairs; srl-zoo_amd/losses/utils.py here).  states, next_states: fp32 [B, S].  With D_b = next_states[b] - states[b],
 * n_b = |D_b|, e_ij = exp(-|s_i - s_j|^2), `dis` the dissimilar pairs [n_dis, 2] and `same` the same-action pairs [n_same, 2]
 * (int32 positions inside the minibatch, in any order, duplicates, i > j and i == j allowed):
 *   terms[0] temporal coherence = mean_b n_b^2            (losses.py:78-81)
 *   terms[1] causality          = mean_dis e_ij            (losses.py:80, 82-83)
 *   terms[2] proportionality    = mean_same (n_i - n_j)^2  (losses.py:84-85)
 *   terms[3] repeatability      = mean_same e_ij |D_i - D_j|^2   (losses.py:87-90)
 * fwd: ONE launch of one workgroup of 256 threads.  Order of every sum, a function of (B, S, n_dis, n_same) alone: a row's or a
 *   pair's value in fp32, k ascending with fma; thread t adds rows t, t + 256, .. (pairs likewise, list order) in fp64; a wave adds
 *   by a butterfly (offsets 32 .. 1); the four wave sums are added left to right; then the division by the count.  terms: four
 *   fp64 values; terms32: the same, rounded to fp32; norms [B]: the n_b, kept for the backward.
 * bwd: ONE launch that writes dstates and dnext_states [B, S] whole, one thread per element:
 *   d next_states[r] = g_tc 2 D_r / B + sum over r's same-action partners q of
 *                        g_pr 2 (n_r - n_q) / n_r / n_same D_r   (nothing where n_r = 0, as torch.norm's backward)
 *                      + g_re 2 e_rq / n_same (D_r - D_q)
 *   d states[r]      = - d next_states[r] - sum over the same-action partners of g_re 2 e_rq |D_r - D_q|^2 / n_same (s_r - s_q)
 *                                         - sum over the dissimilar partners  of g_ca 2 e_rq / n_dis (s_r - s_q)
 *   Both ends of a pair receive the same expression, so the kernel reads an INCIDENCE table per list, which the host builds
 *   (srlz/ops.py robotic_incidence): int32 offsets [B + 1], then 2 * n partners; pair p = [i, j] gives row i the partner j and
 *   row j the partner i (i == j: twice itself, which adds zero), a row's partners in pair order.  The thread adds its same-action
 *   partners in table order, then the dissimilar ones, in fp64; the pair scalars are recomputed by every thread, k ascending, so
 *   the cost is S^2 per incidence: the loss is meant for states of a few dimensions.  g_*: four fp32 device scalars, the upstream
 *   gradients of the four terms.  No atomics; two calls give identical bits.
 * Every index read on the device is clamped to the tensor it addresses (pair entries and partners to [0, B), offsets to
 *   [0, 2n]); the host checks the lists before it uploads them.
 * Refused before anything is enqueued, nothing written: B < 1, S < 1, B * S >= 2^31, an empty pair list (the reference's mean of
 *   nothing is NaN) or 2^30 pairs: SRLZ_ERR_BAD_DESC; a missing pointer: SRLZ_ERR_NULL.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_robotic_fwd(const float* states, const float* next_states, int B, int S, const int* dis /*[n_dis,2]*/, int n_dis,
                     const int* same /*[n_same,2]*/, int n_same, float* norms /*[B]*/, double* terms /*[4]*/,
                     float* terms32 /*[4]*/, srlz_stream_t stream);
int srlz_robotic_bwd(const float* states, const float* next_states, const float* norms /*[B]*/, int B, int S,
                     const int* same_incidence /*[B + 1 + 2 n_same]*/, int n_same, const int* dis_incidence /*[B + 1 + 2 n_dis]*/,
                     int n_dis, const float* g_tc, const float* g_ca, const float* g_pr, const float* g_re, float* dstates,
                     float* dnext_states, srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * A linear state map fitted on a recording by the robotic priors alone (csrc/robotic.hip, srlz/priorsfit.py): s = W x + b with
 * W [S, D] — nn.Linear(D, S) under roboticPriorsLoss (losses/losses.py:62-99, weight 1 each) and torch.optim.Adam, the learner's
 * loop (models/learner.py:277-297, 420-489) without its encoder.  features: fp32 [N, D]; row b of minibatch k is the transition
 * (features[i], features[i + 1]) with i = idx[k][b] clamped to [0, N - 2].  params, m, v: fp32 [S * D + S] in state_dict order
 * (weight, bias).  The pair tables of ALL minibatches live in ONE int32 buffer `tables` [tables_len]; `dir` [n_minibatches][6]
 * names, per minibatch: the offset of its dissimilar pairs [n_dis, 2], n_dis, the offset of its same-action pairs [n_same, 2],
 * n_same, the offsets of the two incidence tables (srlz_robotic_bwd's format: [B + 1] offsets, then the partners).  `order` lists
 * the minibatch ids a call walks.  idx, dir and order are passed twice: the device copy the kernel reads and a host copy the
 * entry point checks.
 * fit: n_steps consecutive Adam steps in ONE launch of ONE workgroup of 256 threads; parameters and gradient stay in LDS from the
 *   first step to the last, the moments in global memory.  Order of every sum, a function of (D, S, B) and the tables alone:
 *   states — 16 lanes per feature row, lane kk adds d = kk, kk + 16, .. ascending, a butterfly over the 16 lanes (offsets 8 .. 1),
 *   + bias; the four terms and the gradient with respect to both state tiles — as srlz_robotic_fwd / _bwd with upstream gradients
 *   1; every parameter's gradient — one thread per element, b ascending, the x_i product before the x_{i+1} product (fma); Adam —
 *   the arithmetic of srlz_adam_step, the step scalars evaluated in double from t0 + step.  running [4] += the four terms of every
 *   step (fp64); step_terms (may be NULL) receives [n_steps][4]; last_grad (may be NULL) the gradient of the LAST step.  No float
 *   atomics.  Two calls leave identical bits; n steps in one call and n calls of one step leave identical bits in params, m, v,
 *   running and step_terms.
 * eval: one workgroup per listed minibatch, the same states and terms; the terms go to ws (srlz_robotic_eval_workspace(n) bytes)
 *   and are added to running [4] in LIST order by the workgroup that finishes last (`ticket`: one zeroed unsigned the kernel leaves
 *   zeroed; no spinning, no grid barrier): the result does not depend on which workgroup that is.  params are only read.
 * Limits: the LDS budget and nothing else.  With SPAD = (S rounded up to a multiple of 4) | 4 the LDS image of the parameters holds
 *   (D + 1) * SPAD floats (row d < D is W[:, d], row D the bias; pads zero and never written back), the gradient as many, Adam's
 *   table 512, the four tiles (states, next states, their gradients) B * SPAD each, the norms B rounded up to 4 and the block sums' 32, within the
 *   160 KB srlz_headfit_fit uses:
 *   srlz_robotic_supported(D, S, B) = D, S, B >= 1 and 2 * (D + 1) * SPAD + 512 + 4 * B * SPAD + ((B + 3) & ~3) + 32 <= 40960.
 *   That accepts D <= 200 with S <= 8 and B <= 256 (17 912 floats at the three ends), D = 768 with S <= 12 at B = 256, D = 4983
 *   at S = 3 with B = 32, and refuses D = 4984 there.
 * Every index read on the device is clamped: rows to [0, N - 2], minibatch ids to [0, n_minibatches), table offsets and counts so
 *   that a list lies inside [0, tables_len), pair entries and partners to [0, B).
 * Refused before anything is enqueued, nothing written: an unsupported (D, S, B), N < 2, N * D >= 2^31, no minibatch, no step,
 *   n_minibatches * B >= 2^31, t0 < 0, an entry of idx_host outside [0, N - 2], of order_host outside [0, n_minibatches), a
 *   directory entry with an empty list or one reaching outside the tables: SRLZ_ERR_BAD_DESC; a missing pointer SRLZ_ERR_NULL;
 *   ws_bytes below srlz_robotic_eval_workspace: SRLZ_ERR_WORKSPACE.  srlz_robotic_eval_workspace returns 0 for n < 1.
 * ------------------------------------------------------------------------------------------------------------ */
int srlz_robotic_supported(int D, int S, int B);
long long srlz_robotic_n_params(int D, int S); /* S*D + S; 0 for D < 1 or S < 1 */
int srlz_robotic_fit(const float* features /*[N,D]*/, int N, int D, int S, const int* idx /*[n_minibatches,B]*/,
                     const int* idx_host, int n_minibatches, int B, const int* tables /*[tables_len]*/, int tables_len,
                     const int* dir /*[n_minibatches,6]*/, const int* dir_host, const int* order /*[n_steps]*/,
                     const int* order_host, int n_steps, float* params, float* m, float* v, int t0, double lr, double beta1,
                     double beta2, double eps, double* running /*[4]*/, double* step_terms /*[n_steps,4] or NULL*/,
                     float* last_grad /*[P] or NULL*/, srlz_stream_t stream);
size_t srlz_robotic_eval_workspace(int n);
int srlz_robotic_eval(const float* features /*[N,D]*/, int N, int D, int S, const int* idx /*[n_minibatches,B]*/,
                      const int* idx_host, int n_minibatches, int B, const int* tables /*[tables_len]*/, int tables_len,
                      const int* dir /*[n_minibatches,6]*/, const int* dir_host, const int* order /*[n]*/, const int* order_host,
                      int n, const float* params, double* running /*[4]*/, void* ws, size_t ws_bytes, unsigned* ticket,
                      srlz_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Debug / calibration hooks (not on the product path).
 * ------------------------------------------------------------------------------------------------------------ */
/* Host-only: dump the virtual-grid program of a 64->64 convolution (tests interpret it on the CPU).
 * out: N,PH,PW,ss,Hs,Ws,ds,Hd,Wd,min_off,span,s2, then 9 x {src class, dst class, flat offset, weight tap}. */
int srlz_conv64_debug_program(const srlz_conv64_desc* d, int backward_data, int* out, int cap);
/* Host-only, launches nothing: the route an nn.Linear entry point would take (csrc/linear.hip decides it in one function, which the
 * entry points execute and this call reports).  op: 0 = srlz_linear_fwd / _fwd_res, 1 = srlz_linear_bwd_data / _bwd_data_res (Kout = K
 * for the plain one; the other ops ignore Kout), 2 = srlz_linear_bwd_weight.  a, b: the two operand ADDRESSES in the entry point's own
 * order ((x, w), (dy, w), (dy, x)); only their alignment is looked at, they are not dereferenced.  has_ws / ws_bytes: whether the call
 * would pass a workspace, and its size.
 * out[0] = kernel: 0 gemm_strided_kernel, 1 gemm_vec_kernel<0,0>, 2 gemm_vec_kernel<0,1>, 3 gemm_vec_kernel<1,1>;
 * out[1] = nz, the number of reduction chunks (1: the result is written directly and the workspace is not touched; > 1: the first
 *          nz * I * J floats of the workspace hold the partial results, I x J the shape of the result);
 * out[2] = rchunk, the length of a chunk (the whole reduction when nz = 1).
 * SRLZ_ERR_BAD_DESC for an unknown op, an empty GEMM, or Kout outside [1, K] with op 1. */
int srlz_linear_debug_route(int op, int M, int N, int K, int Kout, const void* a, const void* b, int has_ws, size_t ws_bytes,
                            int out[3]);
/* Back-to-back fp32 MFMA on random operands (no memory traffic): the matrix rate the chip sustains under load. */
int srlz_debug_mfma_peak(float* out, int blocks, int iters, srlz_stream_t stream);
/* The same MFMA stream with valu_per_mfma (0, 1, 2, 4, 8, 16) independent instructions of `kind` (0 v_fma_f32, 1 v_add_u32,
 * 2 v_pk_fma_f32, 3 v_mov_b32) behind every MFMA — in the same wave, or (split) in the SIMD's second wave: what an
 * instruction next to fp32 MFMAs costs on this chip (profiles/NOTES.md 5.3).  out: blocks * 512 floats. */
int srlz_debug_mfma_valu(float* out, int blocks, int iters, int valu_per_mfma, int kind, int split, srlz_stream_t stream);
/* Debug: out[4*b..] = {XCC id, HW_ID register, start clock, end clock} of workgroup b of a launch whose workgroups each
 * hold lds_bytes of LDS and spin for `spin` ticks (how the dispatcher places / replaces co-resident workgroups). */
int srlz_debug_placement(unsigned* out, int blocks, int lds_bytes, int spin, srlz_stream_t stream);
/* srlz_conv1_fwd(_u8) and srlz_conv1_bwd_weight_fused(_u8) through the generic-pointer window staging, whatever
 * srlz_conv1_buffer_staging_supported says: the reference the buffer staging is compared with, bit for bit.  Arguments as theirs. */
int srlz_debug_conv1_fwd_generic(const float* x_nchw, const float* w_ref, float* y_nhwc, float* stats_partial,
                                 const srlz_skinny_desc* d, srlz_stream_t stream);
int srlz_debug_conv1_fwd_u8_generic(const uint8_t* x_u8, const float* norm_lut, const float* w_ref, float* y_nhwc,
                                    float* stats_partial, const srlz_skinny_desc* d, srlz_stream_t stream);
int srlz_debug_conv1_bwd_weight_fused_generic(const float* x_nchw, const float* y_nhwc, const float* bnp, const uint8_t* argmax,
                                              const float* dpooled, const float* sums, int training, float* dw_ref, void* ws,
                                              size_t ws_bytes, const srlz_skinny_desc* d, const struct srlz_pool_desc_s* pd,
                                              srlz_stream_t stream);
int srlz_debug_conv1_bwd_weight_fused_u8_generic(const uint8_t* x_u8, const float* norm_lut, const float* y_nhwc, const float* bnp,
                                                 const uint8_t* argmax, const float* dpooled, const float* sums, int training,
                                                 float* dw_ref, void* ws, size_t ws_bytes, const srlz_skinny_desc* d,
                                                 const struct srlz_pool_desc_s* pd, srlz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRLZ_H */
