"""Autograd seam between the host-side model classes and the HIP kernels (include/srlz.h).

The reference relies on ``loss.backward()`` (models/learner.py:489); here each fused block is one
``torch.autograd.Function`` whose forward/backward enqueue C-ABI calls on the current HIP stream.  PyTorch tensors are
used for storage only: no torch compute op touches an activation.  Activations are NHWC between the first conv and the
last transposed conv; images and everything the caller sees stay in the reference's NCHW layout.
"""
import ctypes
import weakref

import numpy as np

import torch
from torch.autograd import Function

from . import _cabi as C
from ._cabi import ptr, stream, Conv64Desc, SkinnyDesc, PoolDesc, ConvNDesc

BN_EPS = 1e-5
BN_MOMENTUM = 0.1

# ---- BatchNorm groups -------------------------------------------------------------------------------------------------
# The reference calls the model twice per step, self.model(obs) and self.model(next_obs) (models/learner.py:392-393): two
# independent BatchNorm calls.  Inside `with batch_groups(2):` a forward over the CONCATENATED batch [obs ; next_obs] is
# that pair of calls as ONE launch per layer: every kernel treats images [g*N/G, (g+1)*N/G) as group g with its own batch
# statistics / BatchNorm record, running statistics take the groups' momentum updates in order, num_batches_tracked
# advances by G, weight gradients are summed over the groups by the kernels.  Eval mode has no batch statistics: one group.
_GROUPS = 1


class batch_groups(object):
    def __init__(self, groups):
        self.groups = int(groups)

    def __enter__(self):
        global _GROUPS
        self.prev, _GROUPS = _GROUPS, self.groups
        return self

    def __exit__(self, *exc):
        global _GROUPS
        _GROUPS = self.prev
        return False


def cur_groups(training):
    return _GROUPS if training else 1


# ---- optional per-launch timing (bench.py's roofline leg): HIP events recorded on the stream the kernels run on ----
_timers_on = False
_timer_events = []  # (kernel symbol, layer key, algorithmic flop, start event, end event)


def timers_enable(flag):
    global _timers_on
    _timers_on = bool(flag)
    if flag:
        del _timer_events[:]


def _launch(kernel, key, flop, fn):
    if not _timers_on:
        return fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    _timer_events.append((kernel, key, flop, start, end))
    return out


def timers_report():
    """{kernel or kernel/layer: {"ms", "launches", "flop"}} over everything recorded since timers_enable(True)."""
    torch.cuda.synchronize()
    rep = {}
    for kernel, key, flop, start, end in _timer_events:
        ms = start.elapsed_time(end)
        for name in (kernel, "%s/%s" % (kernel, key)):
            r = rep.setdefault(name, {"ms": 0.0, "launches": 0, "flop": 0.0})
            r["ms"] += ms
            r["launches"] += 1
            r["flop"] += flop
    return rep


# Direct gradient delivery (srlz.optim.FlatParams.grad_buffer / deliver): a parameter re-homed into the flat bucket
# carries `_srlz_flat`; its weight-gradient kernel writes straight into a staging copy of the bucket and autograd gets
# None, which removes one tiny `grad += new` launch per parameter and contribution.  Parameters that are not re-homed (a bare module
# without FlatParams) or whose stages are used up (a fourth contribution in one pass) take autograd's classic accumulation; tests
# clear _DIRECT_GRADS in-process to compare the two.
_DIRECT_GRADS = True


def _gbuf(param, shape=None, device=None):
    """Output buffer for the gradient of `param` (a staging view when the parameter lives in a FlatParams bucket)."""
    if param is not None and _DIRECT_GRADS:
        home = getattr(param, "_srlz_flat", None)
        if home is not None:
            buf = home[0].grad_buffer(home[1])
            if buf is not None:
                buf._srlz_staged = True
                return buf
    if param is not None:
        return torch.empty_like(param)
    return torch.empty(shape, dtype=torch.float32, device=device)


def _give(param, grad):
    """What a backward function returns to autograd for `param`: None when `grad` was written into a staging bucket."""
    if grad is not None and getattr(grad, "_srlz_staged", False):
        return None
    return grad


def _conv64_flop(d):
    # algorithmic FLOP (2 x MAC) of the layer: 9 taps x 64 x 64 per position of the low-resolution side
    pos = d.n * (d.hi * d.wi if d.transposed else d.ho * d.wo)
    return 2.0 * 9 * 64 * 64 * pos


def _convT_out_flop(d):
    # ConvTranspose2d(64, C, 4, 2): 16 taps x 64 x C per feature position
    return 2.0 * 16 * 64 * d.c * d.n * d.hf * d.wf


def _conv1_flop(d):
    # Conv2d(C, 64, 7, 2, 3): 49 taps x C x 64 per feature position
    return 2.0 * 49 * 64 * d.c * d.n * d.hf * d.wf


def _skinny_key(d, what):
    return "%s n%d c%d %dx%d<->%dx%d %s" % ("conv1" if d.kind == 0 else "convT5", d.n, d.c, d.himg, d.wimg, d.hf, d.wf, what)


def _conv64_key(d, what):
    return "%s s%d n%d %dx%d->%dx%d %s" % ("convT" if d.transposed else "conv", d.stride, d.n, d.hi, d.wi, d.ho, d.wo, what)


_workspaces = {}


def _ws(nbytes, device, slot=0):
    """Grow-only scratch buffer per (device, current stream, slot): work on one stream is ordered, so a buffer is only
    ever shared by launches of the stream that owns it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, slot)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def _stats_output(ctx, stats, device):
    """The per-tile statistics of a convolution as the non-differentiable second output of its node (empty when none were asked for)."""
    if stats is None:
        stats = torch.empty(0, device=device)
    ctx.mark_non_differentiable(stats)
    ctx.set_materialize_grads(False)  # no zero tensor for the statistics output in backward
    return stats


def _check(t, name):
    if t.device.type != "cuda":
        raise C.SrlzError("%s must live on the GPU: the srl-zoo_amd hot path has no CPU fallback" % name)
    if t.dtype != torch.float32:
        raise C.SrlzError("%s must be float32 (got %s)" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------------------------
# uint8 frames: observations that are still the loader's bytes, [N,C,W,H] planar (the reference's tensor layout,
# preprocessing/data_loader.py:255, before preprocessInput).  conv1 (forward, fused weight gradient) and the fused reconstruction
# loss normalise them through a 3 x 256 table while they stage their windows; everything else asks for the float tensor.
# ----------------------------------------------------------------------------------------------------------------
_NORM_LUT = {}


def norm_lut(device):
    """((v / 255) - mean[c]) / std[c] for v = 0..255, c = R, G, B (preprocessing/utils.py:20-32), one table per device.

    Built ONCE and made visible to every stream before it is returned (the fill is followed by a device synchronisation), so a
    later launch on another stream reads a finished table.  The first request must not fall inside a hipGraph capture — the fill
    would be recorded instead of executed; SRL4robotics.__init__ asks for the table eagerly for that reason."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    lut = _NORM_LUT.get(index)
    if lut is None:
        if torch.cuda.is_current_stream_capturing():
            raise C.SrlzError("norm_lut: first use inside a stream capture; call srlz.ops.norm_lut(device) once before capturing")
        lut = torch.empty((3, 256), dtype=torch.float32, device=torch.device("cuda", index))
        C.normalize_lut(ptr(lut), stream())
        torch.cuda.synchronize(index)
        _NORM_LUT[index] = lut
    return lut


def is_u8_frames(t):
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8


def _check_u8(t, name):
    if t.device.type != "cuda":
        raise C.SrlzError("%s must live on the GPU: the srl-zoo_amd hot path has no CPU fallback" % name)
    if t.dim() != 4 or t.shape[1] not in (3, 6, 9):
        raise C.SrlzError("%s: uint8 frames must be [N,C,W,H] planar with C in (3, 6, 9), got %s" % (name, tuple(t.shape)))
    return t if t.is_contiguous() else t.contiguous()


def frames_as_float(frames, out=None):
    """uint8 [N,C,W,H] planar frames -> the normalised fp32 observation tensor (float tensors pass through)."""
    if not is_u8_frames(frames):
        return frames
    frames = _check_u8(frames, "frames")
    n, c = frames.shape[:2]
    if out is None:
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.float32 or not out.is_contiguous():
        raise C.SrlzError("frames_as_float: `out` must be a contiguous float32 tensor of the frames' shape")
    lut, plane = norm_lut(frames.device), frames[0, 0].numel()
    per = max(1, 65535 // c)  # one launch takes n * c <= 65535 planes (grid.y)
    for i in range(0, n, per):
        m = min(per, n - i)
        C.normalize_u8_planar(ptr(frames[i:i + m]), ptr(lut), ptr(out[i:i + m]), m, c, plane, stream())
    return out


# ----------------------------------------------------------------------------------------------------------------
# conv1: nn.Conv2d(C, 64, 7, stride 2, pad 3, bias=False) — models/models.py:49
# ----------------------------------------------------------------------------------------------------------------
def _skinny_desc(n, c, himg, wimg, kind, groups=1):
    if kind == 0:
        hf, wf = (himg + 6 - 7) // 2 + 1, (wimg + 6 - 7) // 2 + 1
    else:
        hf, wf = (himg - 4) // 2 + 1, (wimg - 4) // 2 + 1
    return SkinnyDesc(n, c, himg, wimg, hf, wf, kind, groups)


def _conv1_forward(x, w, groups, want_stats):
    """conv1 over float images or the loader's bytes (normalised inside the kernel's window staging) -> the checked (x, w), y (NHWC),
    the per-tile statistics of y (or None) and the descriptor."""
    u8 = is_u8_frames(x)
    x, w = (_check_u8(x, "conv1 input") if u8 else _check(x, "conv1 input")), _check(w, "conv1 weight")
    n, c, h, wd = x.shape
    d = _skinny_desc(n, c, h, wd, 0, groups)
    y = torch.empty((n, d.hf, d.wf, 64), dtype=torch.float32, device=x.device)
    stats = torch.empty((C.skinny_tiles(d), 128), dtype=torch.float32, device=x.device) if want_stats else None
    if u8:
        lut = norm_lut(x.device)
        _launch("skinny_conv_kernel", _skinny_key(d, "fwd u8"), _conv1_flop(d),
                lambda: C.conv1_fwd_u8(ptr(x), ptr(lut), ptr(w), ptr(y), ptr(stats), d, stream()))
    else:
        _launch("skinny_conv_kernel", _skinny_key(d, "fwd"), _conv1_flop(d),
                lambda: C.conv1_fwd(ptr(x), ptr(w), ptr(y), ptr(stats), d, stream()))
    return x, w, y, stats, d


class Conv1Fn(Function):
    @staticmethod
    def forward(ctx, x, w, want_stats):
        # (float images only: the backward's kernels have no byte form)
        x, w, y, stats, d = _conv1_forward(_check(x, "conv1 input"), w, cur_groups(want_stats), want_stats)
        ctx.save_for_backward(x, w)
        ctx.desc = d
        return y, _stats_output(ctx, stats, x.device)

    @staticmethod
    def backward(ctx, dy, _dstats):
        x, w = ctx.saved_tensors
        d = ctx.desc
        dy = _check(dy, "conv1 dy")
        dw = None
        if ctx.needs_input_grad[1]:
            dw = _gbuf(w)
            nbytes = C.skinny_bwd_weight_workspace(d)
            ws = _ws(nbytes, x.device)
            C.conv1_bwd_weight(ptr(x), ptr(dy), ptr(dw), ptr(ws), nbytes, d, stream())
        dx = None
        if ctx.needs_input_grad[0]:  # only when the image carries a gradient (frozen denoiser of the perceptual loss)
            dx = torch.empty_like(x)
            C.conv1_bwd_data(ptr(dy), ptr(w), ptr(dx), d, stream())
        return dx, _give(w, dw), None


# ----------------------------------------------------------------------------------------------------------------
# 64 -> 64 convs: conv3x3 (models/models.py:54,59,217-226) and ConvTranspose2d(64,64,3,2) (models.py:66,70,74,78)
# ----------------------------------------------------------------------------------------------------------------
def conv64_desc(n, hi, wi, stride, pad, transposed, groups=1):
    if transposed:
        ho, wo = (hi - 1) * stride - 2 * pad + 3, (wi - 1) * stride - 2 * pad + 3
    else:
        ho, wo = (hi + 2 * pad - 3) // stride + 1, (wi + 2 * pad - 3) // stride + 1
    return Conv64Desc(n, hi, wi, ho, wo, 3, stride, pad, 1 if transposed else 0, groups)


def _cached_pack(conv, slot, build):
    """The kernel-layout copy `build()` of a frozen convolution's weights, kept on the module under `slot` and rebuilt only if the
    parameter was moved or written (load_state_dict, .to(device))."""
    key = (conv.weight.data_ptr(), conv.weight._version)
    cached = getattr(conv, slot, None)
    if cached is None or cached[0] != key:
        cached = (key, build())
        setattr(conv, slot, cached)
    return cached[1]


def _conv64_forward(x, w, bias, d, want_stats, x_bnp=None, frozen=None):
    """y = conv(x) — or conv(relu(bn(x))) with x's BatchNorm record(s) x_bnp — for checked NHWC x and weights w [64, 64, 3, 3]
    -> (y, per-tile statistics of y or None, packs, wino).  wino: conv3x3 stride 1 pad 1 on an even map (conv2, models/models.py:54;
    layer1 of the ResNet trunk) runs as Winograd F(2x2, 3x3) — 16 multiplications per 2x2 output patch and (ci, co) instead of 36
    (csrc/wino.hip), forward and data gradient; the weight gradient stays the direct contraction.  packs[0] / packs[1] are the
    weights in that kernel's layout for the forward / the data gradient, packed on every call; with `frozen` (the module that owns
    w) they are kept on the module instead, and the Winograd layout is packed for the forward alone."""
    wino = bool(C.conv64_wino_supported(d))

    def build():
        packs = torch.empty((1 if (wino and frozen is not None) else 2, C.conv64_wino_packed_floats() if wino else C.conv64_packed_floats()),
                            dtype=torch.float32, device=x.device)
        back = ptr(packs[1]) if packs.shape[0] == 2 else None
        if wino:
            C.conv64_wino_pack_weights(ptr(w), ptr(packs[0]), back, stream())
        else:
            C.conv64_pack_weights(ptr(w), ptr(packs[0]), back, d, stream())
        return packs
    packs = build() if frozen is None else _cached_pack(frozen, "_srlz_pack_wino" if wino else "_srlz_pack64", build)
    y = torch.empty((d.n, d.ho, d.wo, 64), dtype=torch.float32, device=x.device)
    tiles = C.conv64_wino_tiles(d) if wino else C.conv64_fwd_tiles(d)
    stats = torch.empty((tiles, 128), dtype=torch.float32, device=x.device) if want_stats else None
    if wino:
        name, fwd = "conv64_wino_kernel", C.conv64_wino_fwd
    else:
        pipe = bias is None and x_bnp is None and C.conv64_gather_pipe_supported(d, 0)
        name, fwd = "conv64_gather_pipe_kernel" if pipe else "conv64_fwd_kernel", C.conv64_fwd
    _launch(name, _conv64_key(d, "fwd"), _conv64_flop(d),
            lambda: fwd(ptr(x), ptr(packs[0]), ptr(bias), ptr(y), ptr(stats), ptr(x_bnp), d, stream()))
    return y, stats, packs, wino


class PoolLink:
    """Hand-over between an encoder block (conv -> BatchNorm -> ReLU -> MaxPool, producer of a pooled map) and the convolution that
    consumes the pooled map: the consumer's data-gradient launch computes d(pooled) tile by tile and can take the two
    BatchNorm-backward sums of the producing block in its epilogue (srlz_conv64_bwd_data_pool_sums) instead of the producer running a
    pass of its own over (d pooled, pooled, argmax).  The producer's forward leaves (pooled, bnp, y, argmax, pool descriptor) here; the
    consumer's backward leaves the per-tile records; the producer's backward finalises them.  One producer, one consumer, one pass."""

    def __init__(self):
        self.record = None    # (pooled, bnp, y, argmax, pool desc), set by the producer's forward
        self.partials = None  # [tiles, 128] per-tile sums, set by the consumer's backward

    def take_partials(self):
        p, self.partials, self.record = self.partials, None, None
        return p


_POOL_LINK = True  # (the route without it — hotpath.TAPS on, link = None — runs srlz_bn_relu_pool_bwd_sums in the producer instead)


class Conv64Fn(Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, transposed, want_stats, in_link=None):
        x, w = _check(x, "conv64 input"), _check(w, "conv64 weight")
        n, hi, wi, ch = x.shape
        assert ch == 64 and tuple(w.shape) == (64, 64, 3, 3)
        d = conv64_desc(n, hi, wi, stride, pad, transposed, cur_groups(want_stats))
        y, stats, packs, ctx.wino = _conv64_forward(x, w, bias, d, want_stats)
        ctx.save_for_backward(x, packs)
        ctx.desc = d
        ctx.has_bias = bias is not None
        ctx.needs_dx = ctx.needs_input_grad[0]
        ctx.params = (w, bias)
        ctx.in_link = in_link  # (x is the pooled map of the block that filled this link)
        return y, _stats_output(ctx, stats, x.device)

    @staticmethod
    def backward(ctx, dy, _dstats):
        x, packs = ctx.saved_tensors
        d = ctx.desc
        dy = _check(dy, "conv64 dy")
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):  # (a frozen layer needs neither)
            dw = _gbuf(ctx.params[0])
            db = _gbuf(ctx.params[1]) if ctx.has_bias else None
            nbytes = C.conv64_wino_bwd_weight_workspace(d) if (ctx.wino and not ctx.has_bias) else 0
            if nbytes > 0:  # (0: not a shape the transposed Winograd kernel takes — it indexes ALL groups' images with 32-bit offsets)
                ws = _ws(nbytes, x.device, slot=1)
                _launch("conv64_wino_wgrad_kernel", _conv64_key(d, "wgrad"), _conv64_flop(d),
                        lambda: C.conv64_wino_bwd_weight(ptr(x), ptr(dy), ptr(dw), ptr(ws), nbytes, d, stream()))
            else:
                nbytes = C.conv64_bwd_weight_workspace(d)
                ws = _ws(nbytes, x.device, slot=1)
                _launch("conv64_wgrad_kernel", _conv64_key(d, "wgrad"), _conv64_flop(d),
                        lambda: C.conv64_bwd_weight(ptr(x), ptr(dy), ptr(dw), ptr(db), None, None, ptr(ws), nbytes, d,
                                                    stream()))
        dx = None
        if ctx.needs_dx:
            dx = torch.empty_like(x)
            link = ctx.in_link
            rec = link.record if (link is not None and _POOL_LINK) else None
            if rec is not None and rec[0].data_ptr() == x.data_ptr():
                # dx = d(pooled): the pooled block's BatchNorm-backward sums come out of this launch's epilogue
                pooled, pbnp, py, pargmax, pd = rec
                if ctx.wino:
                    part = torch.empty((C.conv64_wino_bwd_data_rows(d), 128), dtype=torch.float32, device=x.device)
                    _launch("conv64_wino_kernel", _conv64_key(d, "dgrad"), _conv64_flop(d),
                            lambda: C.conv64_wino_bwd_data_pool_sums(ptr(dy), ptr(packs[1]), ptr(dx), ptr(pooled), ptr(pbnp), ptr(py),
                                                                     ptr(pargmax), pd, ptr(part), d, stream()))
                else:
                    part = torch.empty((C.conv64_bwd_data_tiles(d), 128), dtype=torch.float32, device=x.device)
                    _launch("conv64_dgrad_poolsum_kernel", _conv64_key(d, "dgrad"), _conv64_flop(d),
                            lambda: C.conv64_bwd_data_pool_sums(ptr(dy), ptr(packs[1]), ptr(dx), ptr(pooled), ptr(pbnp), ptr(py),
                                                                ptr(pargmax), pd, ptr(part), d, stream()))
                link.partials = part
            elif ctx.wino:
                _launch("conv64_wino_kernel", _conv64_key(d, "dgrad"), _conv64_flop(d),
                        lambda: C.conv64_wino_bwd_data(ptr(dy), ptr(packs[1]), ptr(dx), d, stream()))
            else:
                _launch("conv64_gather_pipe_kernel" if C.conv64_gather_pipe_supported(d, 1) else "conv64_fwd_kernel",
                        _conv64_key(d, "dgrad"), _conv64_flop(d),
                        lambda: C.conv64_bwd_data(ptr(dy), ptr(packs[1]), ptr(dx), None, d, stream()))
        return dx, _give(ctx.params[0], dw), _give(ctx.params[1], db), None, None, None, None, None


# ----------------------------------------------------------------------------------------------------------------
# BatchNorm2d + ReLU (+ MaxPool2d(3, 2, pad)) — models/models.py:50-52,55-57,60-62 / 67-68,71-72,75-76,79-80
# ----------------------------------------------------------------------------------------------------------------
# When the two frames of a step are encoded on two different streams (learner.trainStep), the momentum updates of one
# BatchNorm layer's running statistics must still happen in program order (obs, then next_obs): every update waits for
# the event the previous update of the same buffers recorded.
_bn_last_update = {}


def _ordered_bn_update(running_mean, fn):
    """Run `fn` (a launch that updates the running statistics of one layer — or of several: a list) behind the previous update of the
    same buffers, whichever stream that was enqueued on."""
    rms = running_mean if isinstance(running_mean, (list, tuple)) else [running_mean]
    cur = torch.cuda.current_stream(rms[0].device)
    for rm in rms:
        prev = _bn_last_update.get(rm.data_ptr())
        if prev is not None and prev[0] != cur.cuda_stream:
            cur.wait_event(prev[1])
    fn()
    ev = torch.cuda.Event()
    ev.record(cur)
    for rm in rms:
        _bn_last_update[rm.data_ptr()] = (cur.cuda_stream, ev)


def _bn_params(stats, count, gamma, beta, running_mean, running_var, training, device, tick=None):
    """BatchNorm record(s) of a layer: training -> one 256-float record per group from the producing convolution's
    per-tile partials (`count` = positions of ALL groups together), eval -> one record from the running statistics."""
    groups = cur_groups(training)
    if tick is None:
        tick = getattr(running_mean, "_srlz_tick", None)  # num_batches_tracked of the layer (hotpath._bn_args)
    bnp = torch.empty(256 * groups, dtype=torch.float32, device=device)
    batch_stat = None
    if training:
        batch_stat = torch.empty(128 * groups, dtype=torch.float32, device=device)
        nbytes = C.bn_bwd_workspace(0)
        ws = _ws(nbytes, device)

        def update():  # (tick = num_batches_tracked: advanced by `groups` inside the same launch)
            C.bn_finalize(ptr(stats), stats.shape[0], groups, count // groups, ptr(gamma), ptr(beta), BN_EPS, BN_MOMENTUM, 1,
                          ptr(running_mean), ptr(running_var), ptr(tick), ptr(bnp), ptr(batch_stat), ptr(ws), nbytes, stream())
        _ordered_bn_update(running_mean, update)
    else:
        C.bn_eval_params(ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), BN_EPS, ptr(bnp), stream())
    return bnp, batch_stat


def _bn_backward_sums_from_partials(partial, gb=(None, None), groups=1):
    """The two BatchNorm-backward sums per group, dgamma and dbeta (of the parameters gb) from the per-tile partials that the epilogue
    of a data-gradient kernel left (PoolLink, the decoder's fused backward kernels)."""
    dev = partial.device
    sums = torch.empty(128 * groups, dtype=torch.float32, device=dev)
    dgamma = _gbuf(gb[0], 64, dev)
    dbeta = _gbuf(gb[1], 64, dev)
    nbytes = C.bn_bwd_workspace(0)
    ws = _ws(nbytes, dev)
    C.bn_bwd_finalize_partials(ptr(partial), partial.shape[0], groups, ptr(sums), ptr(dgamma), ptr(dbeta), ptr(ws), nbytes,
                               stream())
    return sums, dgamma, dbeta


def pool_desc(n, h, w, pool_pad, out_nchw, groups):
    """MaxPool2d(3, 2, pool_pad) over an [n, h, w, 64] map."""
    return PoolDesc(n, h, w, (h + 2 * pool_pad - 3) // 2 + 1, (w + 2 * pool_pad - 3) // 2 + 1, pool_pad, 1 if out_nchw else 0, groups)


def _bn_relu_pool(y, stats, bn, training, pool_pad, out_nchw, need_bwd, stat_sink, out_link):
    """maxpool(relu(bn(y))) of a raw convolution output y (NHWC) with per-tile statistics `stats`, bn = (gamma, beta, running mean,
    running var) -> (pooled, BatchNorm record, argmax bytes or None, pool descriptor).  The batch statistics go to stat_sink; with a
    backward to come (need_bwd) the argmax is kept and an NHWC block leaves its record in out_link (PoolLink)."""
    n, h, w, _ = y.shape
    d = pool_desc(n, h, w, pool_pad, out_nchw, cur_groups(training))
    bnp, batch_stat = _bn_params(stats, n * h * w, *bn, training, y.device)
    if stat_sink is not None and batch_stat is not None:
        stat_sink.append(batch_stat)
    pooled = torch.empty((n, 64, d.hp, d.wp) if out_nchw else (n, d.hp, d.wp, 64), dtype=torch.float32, device=y.device)
    argmax = torch.empty((n, d.hp, d.wp, 64), dtype=torch.uint8, device=y.device) if need_bwd else None
    C.bn_relu_pool_fwd(ptr(y), ptr(bnp), ptr(pooled), ptr(argmax), d, stream())
    if need_bwd and out_link is not None and not out_nchw:
        out_link.record = (pooled, bnp, y, argmax, d)
    return pooled, bnp, argmax, d


class BNReLUPoolFn(Function):
    """y (raw conv output, NHWC) -> maxpool(relu(bn(y))).  `stats` are the conv's per-tile partial sums."""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, running_mean, running_var, training, pool_pad, out_nchw, stat_sink, out_link=None):
        y = _check(y, "bn input")
        need_bwd = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        pooled, bnp, argmax, d = _bn_relu_pool(y, stats, (gamma, beta, running_mean, running_var), training, pool_pad, out_nchw,
                                               need_bwd, stat_sink, out_link)
        if need_bwd:
            ctx.save_for_backward(y, bnp, argmax, pooled)
        ctx.desc, ctx.training, ctx.out_link = d, training, out_link
        ctx.params = (gamma, beta)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        y, bnp, argmax, pooled = ctx.saved_tensors
        dpooled = _check(dpooled, "pool grad")
        dy = torch.empty_like(y)
        part = ctx.out_link.take_partials() if ctx.out_link is not None else None
        if part is not None:  # the consumer's data gradient took the two sums in its epilogue (PoolLink)
            sums, dgamma, dbeta = _bn_backward_sums_from_partials(part, ctx.params, max(ctx.desc.groups, 1))
            C.bn_relu_pool_bwd_apply(ptr(y), ptr(bnp), ptr(argmax), ptr(dpooled), ptr(sums), ptr(dy), 1 if ctx.training else 0,
                                     ctx.desc, stream())
        else:
            dgamma, dbeta = _gbuf(ctx.params[0]), _gbuf(ctx.params[1])
            nbytes = C.bn_bwd_workspace(0)
            ws = _ws(nbytes, y.device)
            C.bn_relu_pool_bwd(ptr(y), ptr(bnp), ptr(argmax), ptr(dpooled), ptr(pooled), ptr(dy), ptr(dgamma), ptr(dbeta),
                               1 if ctx.training else 0, ptr(ws), nbytes, ctx.desc, stream())
        return dy, None, _give(ctx.params[0], dgamma), _give(ctx.params[1], dbeta), None, None, None, None, None, None, None


class EncInFn(Function):
    """First encoder block as ONE autograd node: Conv2d(C,64,7,2,3,bias=False) -> BatchNorm2d -> ReLU -> MaxPool(3,2,1)
    (models/models.py:49-52).  Forward = Conv1Fn + BNReLUPoolFn; backward never writes d(loss)/d(conv output): the
    weight-gradient kernel rebuilds it from (y, argmax, dpooled, BN sums) while staging its operand
    (srlz_conv1_bwd_weight_fused).  Saved tensors start with (y, bnp, argmax) like BNReLUPoolFn's."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, training, pool_pad, stat_sink, out_link=None):
        x, w, y, stats, d = _conv1_forward(x, w, cur_groups(training), training)
        need_bwd = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        pooled, bnp, argmax, pd = _bn_relu_pool(y, stats, (gamma, beta, running_mean, running_var), training, pool_pad, False,
                                                need_bwd, stat_sink, out_link)
        if need_bwd:
            ctx.save_for_backward(y, bnp, argmax, pooled, x, w)
        ctx.out_link = out_link
        ctx.desc, ctx.pdesc, ctx.training = d, pd, training
        ctx.params = (gamma, beta)
        ctx.mark_non_differentiable(y)
        ctx.set_materialize_grads(False)  # no 0.8 GB zero tensor for the (non-differentiable) second output
        return pooled, y

    @staticmethod
    def backward(ctx, dpooled, _dy):
        y, bnp, argmax, pooled, x, w = ctx.saved_tensors
        dpooled = _check(dpooled, "pool grad")
        dev = y.device
        part = ctx.out_link.take_partials() if ctx.out_link is not None else None
        if part is not None:  # conv2's data gradient took the two sums in its epilogue (PoolLink)
            sums, dgamma, dbeta = _bn_backward_sums_from_partials(part, ctx.params, max(ctx.pdesc.groups, 1))
        else:
            sums = torch.empty(128 * max(ctx.pdesc.groups, 1), dtype=torch.float32, device=dev)
            dgamma, dbeta = _gbuf(ctx.params[0]), _gbuf(ctx.params[1])
            nbytes = C.bn_bwd_workspace(0)
            ws = _ws(nbytes, dev)
            C.bn_relu_pool_bwd_sums(ptr(y), ptr(bnp), ptr(argmax), ptr(dpooled), ptr(pooled), ptr(sums), ptr(dgamma), ptr(dbeta),
                                    ptr(ws), nbytes, ctx.pdesc, stream())
        dw = _gbuf(w)
        nbytes = C.skinny_bwd_weight_workspace(ctx.desc)
        ws = _ws(nbytes, dev)
        if is_u8_frames(x):
            lut = norm_lut(dev)
            _launch("skinny_wgrad_kernel", _skinny_key(ctx.desc, "wgrad fused u8"), _conv1_flop(ctx.desc),
                    lambda: C.conv1_bwd_weight_fused_u8(ptr(x), ptr(lut), ptr(y), ptr(bnp), ptr(argmax), ptr(dpooled), ptr(sums),
                                                        1 if ctx.training else 0, ptr(dw), ptr(ws), nbytes, ctx.desc, ctx.pdesc,
                                                        stream()))
        else:
            _launch("skinny_wgrad_kernel", _skinny_key(ctx.desc, "wgrad fused"), _conv1_flop(ctx.desc),
                    lambda: C.conv1_bwd_weight_fused(ptr(x), ptr(y), ptr(bnp), ptr(argmax), ptr(dpooled), ptr(sums),
                                                     1 if ctx.training else 0, ptr(dw), ptr(ws), nbytes, ctx.desc, ctx.pdesc,
                                                     stream()))
        return None, _give(w, dw), _give(ctx.params[0], dgamma), _give(ctx.params[1], dbeta), None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------------------------
# Decoder blocks with the BatchNorm-apply + ReLU fused into the NEXT layer's operand load
# (models/models.py:67-82: BatchNorm2d -> ReLU -> ConvTranspose2d).  Input = RAW output of the previous transposed
# convolution + its BatchNorm statistics; the activated tensor relu(bn(y)) is never written to memory.
# ----------------------------------------------------------------------------------------------------------------
def _groups_of(bnp):
    """Number of BatchNorm groups a record tensor holds (256 floats per group)."""
    return bnp.numel() // 256


def _bn_relu_backward(y, bnp, da, training, gb=(None, None)):
    dy = torch.empty_like(y)
    dgamma = _gbuf(gb[0], 64, y.device)
    dbeta = _gbuf(gb[1], 64, y.device)
    nbytes = C.bn_bwd_workspace(0)
    ws = _ws(nbytes, y.device)
    C.bn_relu_bwd(ptr(y), ptr(bnp), ptr(da), ptr(dy), ptr(dgamma), ptr(dbeta), 1 if training else 0, ptr(ws), nbytes,
                  y.numel() // 64, _groups_of(bnp), stream())
    return dy, dgamma, dbeta


class BwdLink:
    """Hand-over of a DEFERRED BatchNorm+ReLU backward between two consecutive decoder blocks.

    Block k+1 (consumer of y_k) owns the backward of BatchNorm_k + ReLU.  Instead of materialising d(loss)/dy_k it only
    computes the two BatchNorm sums, leaves (y_k, bnp_k, sums_k) here and hands dA_k back through autograd; block k
    (producer of y_k, the ONLY consumer of that gradient) picks the record up in its own backward and lets its two
    kernels rebuild d(loss)/dy_k while loading their operand (srlz_bn_bwd_operand).  A link is created per forward
    pass by hotpath.decoder_forward, connects exactly one producer with one consumer, and is only used when nothing
    else looks at y_k's gradient (hotpath.TAPS off)."""

    def __init__(self):
        self.record = None

    def put(self, y, bnp, sums, training):
        self.record = (y, bnp, sums, training)

    def take(self):
        rec, self.record = self.record, None
        return rec


def _bn_relu_backward_sums(y, bnp, da, gb=(None, None)):
    dev = y.device
    groups = _groups_of(bnp)
    sums = torch.empty(128 * groups, dtype=torch.float32, device=dev)
    dgamma = _gbuf(gb[0], 64, dev)
    dbeta = _gbuf(gb[1], 64, dev)
    nbytes = C.bn_bwd_workspace(0)
    ws = _ws(nbytes, dev)
    C.bn_relu_bwd_sums(ptr(y), ptr(bnp), ptr(da), ptr(sums), ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, y.numel() // 64,
                       groups, stream())
    return sums, dgamma, dbeta


def _bn_backward_for_producer(link, y_prev, bnp, da, training, partial=None, gb=(None, None)):
    """BatchNorm+ReLU backward of the block input: deferred to the producer through `link`, or materialised.
    `partial`: per-tile partial sums already written by the epilogue of the kernel that produced `da`."""
    if link is not None:
        if partial is not None:
            sums, dgamma, dbeta = _bn_backward_sums_from_partials(partial, gb, _groups_of(bnp))
        else:
            sums, dgamma, dbeta = _bn_relu_backward_sums(y_prev, bnp, da, gb)
        link.put(y_prev, bnp, sums, training)
        return da, dgamma, dbeta
    return _bn_relu_backward(y_prev, bnp, da, training, gb)


def _operand_from(link, materialise=True):
    """(ctypes record or None, dy_out or None, keep-alive tuple) for the gradient arriving at a producer block.
    materialise: the record asks the data-gradient kernel to also store the rebuilt d(loss)/dy (dy_out) for a separate
    weight-gradient launch; False when one kernel consumes the operand for both gradients (srlz_conv64_bwd_fused)."""
    rec = link.take() if link is not None else None
    if rec is None:
        return None, None, None
    y, bnp, sums, training = rec
    dy_out = torch.empty_like(y) if materialise else None
    op = C.BnBwdOperand(y.data_ptr(), bnp.data_ptr(), sums.data_ptr(), y.numel() // 64 // _groups_of(bnp), 1 if training else 0,
                        dy_out.data_ptr() if materialise else None)
    return op, dy_out, rec


# Data + weight + bias gradient of a decoder block's ConvTranspose are ONE launch wherever the shape allows
# (srlz_conv64_bwd_fused_supported: at least 8 tiles, a low-resolution grid of at most 63 columns, two BatchNorm groups at most);
# other shapes take a data-gradient launch that stores the rebuilt d(loss)/dy and a weight-gradient launch that reads it back.


class DecBlockFn(Function):
    """(y_prev raw, stats_prev, gamma, beta, running stats) -> y = ConvTranspose2d(64,64,3,2)(relu(bn(y_prev))) + stats.
    in_link: BwdLink shared with the producer of y_prev (or None); out_link: shared with the consumer of y (or None)."""

    @staticmethod
    def forward(ctx, y_prev, stats_prev, gamma, beta, running_mean, running_var, training, w, bias, want_stats,
                in_link=None, out_link=None):
        y_prev, w = _check(y_prev, "decoder block input"), _check(w, "convT weight")
        n, hi, wi, _ = y_prev.shape
        bnp, _ = _bn_params(stats_prev, n * hi * wi, gamma, beta, running_mean, running_var, training, y_prev.device)
        d = conv64_desc(n, hi, wi, 2, 0, True, cur_groups(training))
        y, stats, packs, _ = _conv64_forward(y_prev, w, bias, d, want_stats, bnp)
        ctx.save_for_backward(y_prev, bnp, packs)
        ctx.desc, ctx.training = d, training
        ctx.in_link, ctx.out_link = in_link, out_link
        ctx.params = (gamma, beta, w, bias)
        return y, _stats_output(ctx, stats, y_prev.device)

    @staticmethod
    def backward(ctx, dy, _dstats):
        y_prev, bnp, packs = ctx.saved_tensors
        d = ctx.desc
        dy = _check(dy, "decoder block dy")
        da = torch.empty_like(y_prev)
        if ctx.out_link is not None and ctx.out_link.record is not None and C.conv64_bwd_fused_supported(d):
            # `dy` is dA of the following BatchNorm+ReLU: ONE kernel rebuilds the true dy while staging it and contracts it both ways
            # (data gradient and weight / bias gradient) — it is never written to memory
            dy_bn, _, keep = _operand_from(ctx.out_link, materialise=False)
            dw = _gbuf(ctx.params[2])
            db = _gbuf(ctx.params[3], 64, dy.device)
            nbytes = C.conv64_bwd_fused_workspace(d)
            ws = _ws(nbytes, dy.device, slot=1)
            # with the producer's BatchNorm backward deferred (in_link), its two sums come out of this launch's flush as partial records
            part = torch.empty((C.conv64_bwd_fused_bn_rows(d), 128), dtype=torch.float32, device=dy.device) if ctx.in_link is not None else None
            _launch("conv64_bwd_fused_kernel", _conv64_key(d, "dgrad+wgrad"), 2.0 * _conv64_flop(d),
                    lambda: C.conv64_bwd_fused(ptr(y_prev), ptr(bnp), ptr(dy), dy_bn, ptr(packs[1]), ptr(da), ptr(dw), ptr(db), ptr(part),
                                               ptr(ws), nbytes, d, stream()))
        else:
            # dy_bn not None: `dy` is dA of the following BatchNorm+ReLU; the data-gradient kernel rebuilds the true dy in its
            # operand load and stores it (dy_true) for the weight-gradient kernel, which therefore runs second
            dy_bn, dy_true, keep = _operand_from(ctx.out_link)
            # (the fused-operand launch is a different instantiation of the kernel: timed under its own name)
            _launch("conv64_fwd_kernel" if dy_bn is None else "conv64_fwd_kernel<bn-bwd operand>", _conv64_key(d, "dgrad"),
                    _conv64_flop(d), lambda: C.conv64_bwd_data(ptr(dy), ptr(packs[1]), ptr(da), dy_bn, d, stream()))
            if dy_true is not None:
                dy = dy_true
            dw = _gbuf(ctx.params[2])
            db = _gbuf(ctx.params[3], 64, dy.device)
            nbytes = C.conv64_bwd_weight_workspace(d)
            ws = _ws(nbytes, dy.device, slot=1)
            _launch("conv64_wgrad_kernel", _conv64_key(d, "wgrad"), _conv64_flop(d),
                    lambda: C.conv64_bwd_weight(ptr(y_prev), ptr(dy), ptr(dw), ptr(db), ptr(bnp), None, ptr(ws), nbytes, d,
                                                stream()))
            part = None
        dy_prev, dgamma, dbeta = _bn_backward_for_producer(ctx.in_link, y_prev, bnp, da, ctx.training, partial=part, gb=ctx.params[:2])
        gp, bp, wp, cp = ctx.params
        return dy_prev, None, _give(gp, dgamma), _give(bp, dbeta), None, None, None, _give(wp, dw), _give(cp, db), None, None, None


# The last ConvTranspose's backward is ONE fused launch whenever the BatchNorm backward in front of it is deferred (in_link) and the
# shape is supported (C = 3 / 6); the two-launch form serves hotpath.TAPS (no link) and is the reference of the fused kernel's tests.


def _dec_out_open(y_prev, stats_prev, bn, training, w):
    """What both forms of the last ConvTranspose start with: the checked (y_prev, w), the BatchNorm record of y_prev from its per-tile
    statistics and bn = (gamma, beta, running mean, running var), and the descriptor of ConvTranspose2d(64, C, 4, 2) over y_prev's map."""
    y_prev, w = _check(y_prev, "decoder output input"), _check(w, "convT_out weight")
    n, hf, wf, _ = y_prev.shape
    bnp, _ = _bn_params(stats_prev, n * hf * wf, *bn, training, y_prev.device)
    return y_prev, w, bnp, SkinnyDesc(n, w.shape[1], (hf - 1) * 2 + 4, (wf - 1) * 2 + 4, hf, wf, 1, cur_groups(training))


class DecOutFn(Function):
    """(y_prev raw, stats, BN params) -> ConvTranspose2d(64, C, 4, 2)(relu(bn(y_prev))), NCHW (models/models.py:79-82)."""

    @staticmethod
    def forward(ctx, y_prev, stats_prev, gamma, beta, running_mean, running_var, training, w, bias, in_link=None):
        y_prev, w, bnp, d = _dec_out_open(y_prev, stats_prev, (gamma, beta, running_mean, running_var), training, w)
        y = torch.empty((d.n, d.c, d.himg, d.wimg), dtype=torch.float32, device=y_prev.device)
        _launch("convT_out_os_kernel", _skinny_key(d, "fwd"), _convT_out_flop(d),
                lambda: C.convT_out_fwd(ptr(y_prev), ptr(w), ptr(bias), ptr(y), ptr(bnp), d, stream()))
        ctx.save_for_backward(y_prev, bnp, w)
        ctx.desc, ctx.training, ctx.in_link = d, training, in_link
        ctx.params = (gamma, beta, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        y_prev, bnp, w = ctx.saved_tensors
        dy = _check(dy, "decoder output dy")
        return _dec_out_backward(ctx, y_prev, bnp, w, dy, None) + (None,)


def _dec_out_backward(ctx, y_prev, bnp, w, dy, gain):
    """Backward of the last ConvTranspose (DecOutFn / DecOutLossFn): gradients for (y_prev, stats, gamma, beta, rm, rv, training,
    w, bias).  gain = (upstream scalar tensor, div, coef): `dy` holds the reconstruction error and the loss gradient is
    ((upstream / div) * coef) * dy — applied inside the fused kernel, or materialised in place for the two-launch path."""
    d = ctx.desc
    dw = _gbuf(w)
    db = _gbuf(ctx.params[2], d.c, dy.device)
    if ctx.in_link is not None and C.convT_out_bwd_fused_supported(d):
        # data gradient, its BatchNorm-backward partials and the weight / bias gradients in one pass over (dy, y_prev)
        da = torch.empty_like(y_prev)
        partial = torch.empty((C.convT_out_bwd_fused_tiles(d), 128), dtype=torch.float32, device=dy.device)
        nbytes = C.convT_out_bwd_fused_workspace(d)
        ws = _ws(nbytes, dy.device, slot=1)
        g_dev, g_div, g_coef = (ptr(gain[0]), gain[1], gain[2]) if gain is not None else (None, 1.0, 1.0)
        _launch("convT_out_os_bwd_kernel", _skinny_key(d, "dgrad+wgrad"), 2.0 * _convT_out_flop(d),
                lambda: C.convT_out_bwd_fused(ptr(dy), ptr(w), ptr(da), ptr(y_prev), ptr(bnp), ptr(partial), ptr(dw), ptr(db), ptr(ws),
                                              nbytes, g_dev, g_div, g_coef, d, stream()))
        dy_prev, dgamma, dbeta = _bn_backward_for_producer(ctx.in_link, y_prev, bnp, da, ctx.training, partial, gb=ctx.params[:2])
        gp, bp, cp = ctx.params
        return dy_prev, None, _give(gp, dgamma), _give(bp, dbeta), None, None, None, _give(w, dw), _give(cp, db)
    if gain is not None:  # the two-launch kernels take the gradient itself: error -> gradient, in place (the error has no other use)
        C.scale_by_scalar(ptr(dy), ptr(gain[0]), gain[1], gain[2], ptr(dy), dy.numel(), stream())
    nbytes = C.skinny_bwd_weight_workspace(d)
    ws = _ws(nbytes, dy.device, slot=1)
    C.convT_out_bwd_weight(ptr(y_prev), ptr(dy), ptr(dw), ptr(db), ptr(bnp), ptr(ws), nbytes, d, stream())
    da = torch.empty_like(y_prev)
    # with the BatchNorm backward deferred (in_link), its two sums come out of this kernel's epilogue
    partial = None
    if ctx.in_link is not None:
        partial = torch.empty((C.skinny_tiles(d), 128), dtype=torch.float32, device=dy.device)
    C.convT_out_bwd_data(ptr(dy), ptr(w), ptr(da), ptr(y_prev) if partial is not None else None,
                         ptr(bnp) if partial is not None else None, ptr(partial), d, stream())
    dy_prev, dgamma, dbeta = _bn_backward_for_producer(ctx.in_link, y_prev, bnp, da, ctx.training, partial, gb=ctx.params[:2])
    gp, bp, cp = ctx.params
    return dy_prev, None, _give(gp, dgamma), _give(bp, dbeta), None, None, None, _give(w, dw), _give(cp, db)


class DecOutLossFn(Function):
    """The last ConvTranspose AND the step's reconstruction / generation loss as one node (K11 / K12 of SURVEY.md 8a'; reference
    models/models.py:79-82 followed by losses/losses.py:172-214): (y_prev raw, stats, BN params, weights, target [obs ; next_obs])
    -> (loss scalar, err = dec - target [not differentiable; the backward's operand]).  mean: reconstructionLoss x 2
    (sum / numel per frame, added), else F.mse_loss(reduction='sum') x 2.  The batch is the pair of frames of a step.
    Backward: d(loss)/d(dec) = ((upstream / div) * 2) * err, formed inside the ConvTranspose's backward kernel."""

    @staticmethod
    def forward(ctx, y_prev, stats_prev, gamma, beta, running_mean, running_var, training, w, bias, in_link, target, mean):
        u8 = is_u8_frames(target)
        target = _check_u8(target, "reconstruction target") if u8 else _check(target, "reconstruction target")
        y_prev, w, bnp, d = _dec_out_open(y_prev, stats_prev, (gamma, beta, running_mean, running_var), training, w)
        if tuple(target.shape) != (d.n, d.c, d.himg, d.wimg) or d.n % 2:
            raise C.SrlzError("fused reconstruction loss: target %s does not match the decoder output %s"
                              % (tuple(target.shape), (d.n, d.c, d.himg, d.wimg)))
        err = torch.empty((d.n, d.c, d.himg, d.wimg), dtype=torch.float32, device=y_prev.device)
        nwg = C.convT_out_fwd_loss_workgroups(d)
        part = _ws(2 * nwg * 8, y_prev.device, slot=2)
        if u8:
            lut = norm_lut(y_prev.device)
            _launch("convT_out_os_kernel", _skinny_key(d, "fwd+loss u8"), _convT_out_flop(d),
                    lambda: C.convT_out_fwd_loss_u8(ptr(y_prev), ptr(w), ptr(bias), ptr(target), ptr(lut), ptr(err), None, ptr(bnp),
                                                    ptr(part), d, stream()))
        else:
            _launch("convT_out_os_kernel", _skinny_key(d, "fwd+loss"), _convT_out_flop(d),
                    lambda: C.convT_out_fwd_loss(ptr(y_prev), ptr(w), ptr(bias), ptr(target), ptr(err), None, ptr(bnp), ptr(part), d,
                                                 stream()))
        sums = torch.empty(2, dtype=torch.float32, device=y_prev.device)
        comb = torch.empty((), dtype=torch.float32, device=y_prev.device)
        per_frame = err.numel() // 2
        C.pair_loss_finalize(ptr(part), nwg, per_frame, 1 if mean else 0, ptr(sums), ptr(comb), stream())
        ctx.save_for_backward(y_prev, bnp, w, err)
        ctx.desc, ctx.training, ctx.in_link = d, training, in_link
        ctx.params = (gamma, beta, bias)
        ctx.div = float(per_frame) if mean else 1.0
        ctx.mark_non_differentiable(err)
        ctx.set_materialize_grads(False)
        return comb, err

    @staticmethod
    def backward(ctx, g, _derr):
        y_prev, bnp, w, err = ctx.saved_tensors
        g = _check(g, "loss grad")
        return _dec_out_backward(ctx, y_prev, bnp, w, err, (g, ctx.div, 2.0)) + (None, None, None)


def bn_relu_materialise(y, bnp_source):
    """relu(bn(y)) as a tensor — debug / test helper only (the product path fuses it into the consumer)."""
    a = torch.empty_like(y)
    C.bn_relu_fwd(ptr(y), ptr(bnp_source), ptr(a), y.numel() // 64, stream())
    return a


# ----------------------------------------------------------------------------------------------------------------
# nn.Linear — autoencoders.py:94-100, vae.py:52-57, forward_inverse.py:16,48-55
# ----------------------------------------------------------------------------------------------------------------
class LinearFn(Function):
    @staticmethod
    def forward(ctx, x, w, b, relu):
        x, w = _check(x, "linear input"), _check(w, "linear weight")
        m, k = x.shape
        n = w.shape[0]
        assert w.shape[1] == k
        y = torch.empty((m, n), dtype=torch.float32, device=x.device)
        nbytes = C.linear_workspace(m, n, k)
        ws = _ws(nbytes, x.device)
        C.linear_fwd(ptr(x), ptr(w), ptr(b), ptr(y), m, n, k, 1 if relu else 0, ptr(ws), nbytes, stream())
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.relu, ctx.has_bias, ctx.needs_dx = relu, b is not None, ctx.needs_input_grad[0]
        ctx.params = (b,)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = _check(dy, "linear dy")
        m, k = x.shape
        n = w.shape[0]
        if ctx.relu:
            dy = dy.clone()
            C.relu_bwd_inplace(ptr(y), ptr(dy), dy.numel(), stream())
        nbytes = C.linear_workspace(m, n, k)
        ws = _ws(nbytes, x.device)
        dx = None
        if ctx.needs_dx:
            dx = torch.empty_like(x)
            C.linear_bwd_data(ptr(dy), ptr(w), ptr(dx), m, n, k, ptr(ws), nbytes, stream())
        dw = _gbuf(w)
        db = _gbuf(ctx.params[0]) if ctx.has_bias else None
        C.linear_bwd_weight(ptr(dy), ptr(x), ptr(dw), ptr(db), m, n, k, ptr(ws), nbytes, stream())
        return dx, _give(w, dw), _give(ctx.params[0], db), None


# ----------------------------------------------------------------------------------------------------------------
# Dense layers of the mlp / linear models — nn.Linear(input_dim, h) / nn.Linear(h, input_dim), autoencoders.py:6-81,
# vae.py:6-40, priors.py:71-125 (csrc/dense.hip).  The image side is x.view(M, -1) of [M, C, W, H] frames: fp32, or the
# loader's planar uint8 bytes normalised inside the kernels (same table as frames_as_float, same values bit for bit).
# ----------------------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


def _dense_image(x, name):
    """(fp32 tensor or None, uint8 tensor or None, M, K) of an image operand [M, C, W, H] (or an fp32 [M, K])."""
    if is_u8_frames(x):
        x = _check_u8(x, name)
        return None, x, x.shape[0], x[0].numel()
    x = _check(x, name)
    return x, None, x.shape[0], x[0].numel()


def _dense_require(m, n, k, plane):
    if not C.dense_supported(m, n, k, plane):
        raise C.SrlzError("dense layer M = %d, n = %d, K = %d (plane %d): %s" % (m, n, k, plane, C.error_text()))


def _dense_flop(m, n, k):
    return 2.0 * m * n * k


class DenseInFn(Function):
    """y[M,n] = act(x.view(M, -1) . W^T + b) with act none / ReLU / tanh; backward: the weight and bias gradients only (the images
    carry no gradient in these models)."""

    @staticmethod
    def forward(ctx, x, w, b, act, plane):
        if x.requires_grad:
            raise C.SrlzError("dense input layer: the image operand must not require a gradient (no data-gradient kernel)")
        xf, x8, m, k = _dense_image(x, "dense input")
        w = _check(w, "dense weight")
        n = w.shape[0]
        if w.shape[1] != k:
            raise C.SrlzError("dense input layer: weight %s does not match K = %d" % (tuple(w.shape), k))
        _dense_require(m, n, k, plane)
        y = torch.empty((m, n), dtype=torch.float32, device=w.device)
        nbytes = C.dense_in_workspace(m, n, k)
        ws = _ws(nbytes, w.device)
        lut = norm_lut(w.device) if x8 is not None else None
        _launch("dense_tile_kernel", "in_fwd m%d n%d k%d%s" % (m, n, k, " u8" if x8 is not None else ""), _dense_flop(m, n, k),
                lambda: C.dense_in_fwd(ptr(xf), ptr(x8), ptr(lut), ptr(w), ptr(b), ptr(y), m, n, k, plane, act, ptr(ws), nbytes,
                                       stream()))
        ctx.save_for_backward(xf if xf is not None else x8, w, y if act != ACT_NONE else None)
        ctx.u8, ctx.act, ctx.plane, ctx.has_bias = x8 is not None, act, plane, b is not None
        ctx.params = (b,)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = _check(dy, "dense dy")
        m, n, k = x.shape[0], w.shape[0], w.shape[1]
        if ctx.act == ACT_RELU:
            dy = dy.clone()
            C.relu_bwd_inplace(ptr(y), ptr(dy), dy.numel(), stream())
        elif ctx.act == ACT_TANH:
            d = torch.empty_like(dy)
            C.tanh_bwd(ptr(y), ptr(dy), ptr(d), dy.numel(), stream())
            dy = d
        dw = _gbuf(w)
        db = _gbuf(ctx.params[0]) if ctx.has_bias else None
        xf, x8 = (None, x) if ctx.u8 else (x, None)
        lut = norm_lut(w.device) if ctx.u8 else None
        _launch("dense_tile_kernel", "in_wgrad m%d n%d k%d%s" % (m, n, k, " u8" if ctx.u8 else ""), _dense_flop(m, n, k),
                lambda: C.dense_in_wgrad(ptr(dy), ptr(xf), ptr(x8), ptr(lut), ptr(dw), ptr(db), m, n, k, ctx.plane, stream()))
        return None, _give(w, dw), _give(ctx.params[0], db), None, None


def _dense_out_grads(ctx, z, w, m, n, k, nbytes, call):
    """Shared tail of the two backward passes of the output layer: buffers (a workspace of nbytes), then `call(dz, dw, db, ws, nbytes)`."""
    dz = torch.empty((m, n), dtype=torch.float32, device=z.device) if ctx.needs_input_grad[0] else None
    dw = _gbuf(w)
    b = ctx.params[0]
    db = _gbuf(b) if b is not None else torch.empty(k, dtype=torch.float32, device=z.device)
    # (a per-call buffer, not a grow-only slot: the dOut staging of the fused route is M * K floats, and the allocator may hand it
    # to the next layer's backward as soon as this launch sequence is enqueued)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=z.device)
    _launch("dense_tile_kernel", "out_bwd m%d n%d k%d" % (m, n, k), 3 * _dense_flop(m, n, k), lambda: call(dz, dw, db, ws, nbytes))
    return dz, _give(w, dw), (_give(b, db) if b is not None else None)


class DenseOutFn(Function):
    """out[M,K] = z . W^T + b — the decoded frames, flat (the caller views them as [M, C, W, H])."""

    @staticmethod
    def forward(ctx, z, w, b, plane):
        z, w = _check(z, "dense output input"), _check(w, "dense output weight")
        m, n = z.shape
        k = w.shape[0]
        if w.shape[1] != n:
            raise C.SrlzError("dense output layer: weight %s does not match n = %d" % (tuple(w.shape), n))
        _dense_require(m, n, k, plane)
        out = torch.empty((m, k), dtype=torch.float32, device=z.device)
        _launch("dense_tile_kernel", "out_fwd m%d n%d k%d" % (m, n, k), _dense_flop(m, n, k),
                lambda: C.dense_out_fwd(ptr(z), ptr(w), ptr(b), ptr(out), m, n, k, plane, stream()))
        ctx.save_for_backward(z, w)
        ctx.plane = plane
        ctx.params = (b,)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, w = ctx.saved_tensors
        dout = _check(dout, "dense output grad")
        m, n = z.shape
        k = w.shape[0]
        # (the given dOut needs no staging: only the data gradient's split partials)
        return _dense_out_grads(ctx, z, w, m, n, k, C.dense_in_workspace(m, n, k), lambda dz, dw, db, ws, nbytes: C.dense_out_bwd_from(
            ptr(dout), ptr(z), ptr(w), ptr(dz), ptr(dw), ptr(db), m, n, k, ctx.plane, ptr(ws), nbytes, stream())) + (None,)


class DenseOutLossFn(Function):
    """The output layer AND the step's reconstruction (mean=True: sum / numel per frame, added) or generation (sums added) loss
    against target [M, C, W, H] (fp32 or uint8 frames; M = the two frames of a step) as one node: the decoded frames are never
    written.  Backward: d(loss)/d(out) = ((upstream / div) * 2) * (out - target) recomputed inside the backward kernels."""

    @staticmethod
    def forward(ctx, z, w, b, target, mean, plane):
        z, w = _check(z, "dense output input"), _check(w, "dense output weight")
        tf, t8, mt, kt = _dense_image(target, "reconstruction target")
        m, n = z.shape
        k = w.shape[0]
        if w.shape[1] != n or mt != m or kt != k or m % 2:
            raise C.SrlzError("fused dense reconstruction loss: target %s does not match the output [%d, %d]"
                              % (tuple(target.shape), m, k))
        _dense_require(m, n, k, plane)
        nwg = C.dense_out_fwd_loss_workgroups(m, k)
        part = _ws(2 * nwg * 8, z.device, slot=2)
        lut = norm_lut(z.device) if t8 is not None else None
        _launch("dense_tile_kernel", "out_fwd+loss m%d n%d k%d%s" % (m, n, k, " u8" if t8 is not None else ""), _dense_flop(m, n, k),
                lambda: C.dense_out_fwd_loss(ptr(z), ptr(w), ptr(b), ptr(tf), ptr(t8), ptr(lut), ptr(part), m, n, k, plane, m // 2,
                                             stream()))
        sums = torch.empty(2, dtype=torch.float32, device=z.device)
        comb = torch.empty((), dtype=torch.float32, device=z.device)
        per_frame = (m // 2) * k
        C.pair_loss_finalize(ptr(part), nwg, per_frame, 1 if mean else 0, ptr(sums), ptr(comb), stream())
        ctx.save_for_backward(z, w, tf if tf is not None else t8)
        ctx.u8, ctx.plane, ctx.div = t8 is not None, plane, float(per_frame) if mean else 1.0
        ctx.params = (b,)
        return comb

    @staticmethod
    def backward(ctx, g):
        z, w, t = ctx.saved_tensors
        g = _check(g, "loss grad")
        m, n = z.shape
        k = w.shape[0]
        tf, t8 = (None, t) if ctx.u8 else (t, None)
        lut = norm_lut(z.device) if ctx.u8 else None
        b = ctx.params[0]
        return _dense_out_grads(ctx, z, w, m, n, k, C.dense_out_bwd_workspace(m, n, k), lambda dz, dw, db, ws, nbytes: C.dense_out_bwd(
            ptr(z), ptr(w), ptr(b), ptr(tf), ptr(t8), ptr(lut), ptr(g), ctx.div, ptr(dz), ptr(dw), ptr(db), m, n, k, ctx.plane,
            ptr(ws), nbytes, stream())) + (None, None, None)


class TanhFn(Function):
    """nn.Tanh (autoencoders.py:52-62)."""

    @staticmethod
    def forward(ctx, x):
        x = _check(x, "tanh input")
        y = torch.empty_like(x)
        C.tanh_fwd(ptr(x), ptr(y), x.numel(), stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        dy = _check(dy, "tanh dy")
        dx = torch.empty_like(dy)
        C.tanh_bwd(ptr(y), ptr(dy), ptr(dx), dy.numel(), stream())
        return dx


class AddConstFn(Function):
    """x + c for a constant tensor c (GaussianNoiseVariant's x + noise, custom_layers.py:49-50); the gradient passes through."""

    @staticmethod
    def forward(ctx, x, c):
        x, c = _check(x, "add input"), _check(c, "add constant")
        out = torch.empty_like(x)
        C.add_f32(ptr(x), ptr(c), ptr(out), x.numel(), stream())
        return out

    @staticmethod
    def backward(ctx, dy):
        return dy, None


class TotalLossFn(Function):
    """total = sum_i w_i * l_i over 0-dim device scalars, as LossManager.computeTotalLoss forms it (reference losses/losses.py:55-56:
    Python's left-to-right sum of separately rounded fp32 products), in ONE launch that also drops [total, l_0, l_1, ...] into
    `tail` (the gradient bucket's scalar tail) when given; backward: d l_i = w_i * d total, one launch."""

    @staticmethod
    def forward(ctx, weights, tail, *losses):
        n = len(losses)
        losses = [_check(l, "loss term").reshape(()) for l in losses]
        ptrs = (ctypes.c_void_p * n)(*[l.data_ptr() for l in losses])
        w = (ctypes.c_float * n)(*[float(x) for x in weights])
        total = torch.empty((), dtype=torch.float32, device=losses[0].device)
        C.weighted_total(ptrs, w, n, ptr(total), ptr(tail), stream())
        ctx.weights, ctx.n = w, n
        ctx.keep = losses  # (the kernel is asynchronous: the terms must outlive it)
        return total

    @staticmethod
    def backward(ctx, dout):
        g = torch.empty(ctx.n, dtype=torch.float32, device=dout.device)
        C.weighted_total_bwd(ptr(dout.contiguous()), ctx.weights, ctx.n, ptr(g), stream())
        return (None, None) + tuple(g[i] for i in range(ctx.n))


class MaskColumnsFn(Function):
    """x with every column outside [lo, hi) zeroed — SRLModulesSplit.detachSplit (reference models/modules.py:191-236)
    rebuilds the state from th.zeros_like blocks and one kept slice, i.e. applies this mask; gradient = same mask."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        x = _check(x, "split input")
        rows, cols = x.shape
        y = torch.empty_like(x)
        C.mask_columns(ptr(x), ptr(y), rows, cols, lo, hi, stream())
        ctx.range = (lo, hi)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _check(dy, "split grad")
        rows, cols = dy.shape
        dx = torch.empty_like(dy)
        C.mask_columns(ptr(dy), ptr(dx), rows, cols, ctx.range[0], ctx.range[1], stream())
        return dx, None, None


_param_tables = {}
_grad_tables = {}


def _param_table(params):
    """Device arrays (addresses, lengths) of a parameter list, cached per list of storage addresses."""
    key = tuple((p.data_ptr(), p.numel()) for p in params)
    tab = _param_tables.get(key)
    if tab is None:
        dev = params[0].device
        tab = (torch.tensor([k[0] for k in key], dtype=torch.int64, device=dev),
               torch.tensor([k[1] for k in key], dtype=torch.int64, device=dev))
        _param_tables.clear()  # parameters are re-homed rarely (FlatParams): keep one table
        _param_tables[key] = tab
    return tab


class ParamNormFn(Function):
    """mode 0: sum_i sum|p_i| (l1Loss, reference losses.py:132-142); mode 1: (sum_i ||p_i||_2) / len(params) (l2Loss,
    losses.py:145-155).  One launch over the whole parameter list (one workgroup per tensor, fp64 accumulation)."""

    @staticmethod
    def forward(ctx, mode, *params):
        for p in params:
            _check(p, "regularised parameter")
        nseg = len(params)
        ptrs, lens = _param_table(params)
        dev = params[0].device
        norms = torch.empty(nseg, dtype=torch.float32, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        scale = 1.0 if mode == 0 else 1.0 / nseg
        C.param_norms(ptr(ptrs), ptr(lens), nseg, mode, scale, ptr(norms), ptr(out), stream())
        ctx.save_for_backward(norms, ptrs, lens, *params)
        ctx.mode, ctx.scale = mode, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        norms, ptrs, lens = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        dout = dout.contiguous()
        grads = [_gbuf(p) for p in params]  # staging views for bucketed parameters: fixed addresses, table cached
        key = tuple(g.data_ptr() for g in grads)
        gptrs = _grad_tables.get(key)
        if gptrs is None:
            gptrs = torch.tensor(key, dtype=torch.int64, device=norms.device)
            _grad_tables.clear()
            _grad_tables[key] = gptrs
        C.param_norms_grad(ptr(ptrs), ptr(gptrs), ptr(lens), len(params), ctx.mode, ptr(norms), ptr(dout), ctx.scale,
                           stream())
        return (None,) + tuple(_give(p, g) for p, g in zip(params, grads))


class ToNHWCFn(Function):
    """[N,C,H,W] -> [N,H,W,C] (the decoder_fc -> view(N,64,6,6) seam, autoencoders.py:116-117)."""

    @staticmethod
    def forward(ctx, x):
        x = _check(x, "layout input")
        n, c, h, w = x.shape
        y = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
        C.nchw_to_nhwc(ptr(x), ptr(y), n, c, h, w, stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _check(dy, "layout grad")
        n, h, w, c = dy.shape
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
        C.nhwc_to_nchw(ptr(dy), ptr(dx), n, c, h, w, stream())
        return dx


# ----------------------------------------------------------------------------------------------------------------
# losses — losses/losses.py
# ----------------------------------------------------------------------------------------------------------------
class SqDiffSumFn(Function):
    """sum((a-b)^2) — F.mse_loss(sum) (losses.py:210) — or, with mean=True, sum((a-b)^2) / numel — reconstructionLoss (losses.py:181):
    the fp32 division behind the sum's own rounding, in the reduction's last launch, and (g / numel) formed inside the gradient kernel."""

    @staticmethod
    def forward(ctx, a, b, mean=False):
        a, b = _check(a, "loss input"), _check(b, "loss target")
        assert a.shape == b.shape
        out = torch.empty((), dtype=torch.float32, device=a.device)
        nbytes = C.reduce_workspace(a.numel())
        ws = _ws(nbytes, a.device)
        if mean:
            C.sqdiff_mean(ptr(a), ptr(b), a.numel(), float(a.numel()), ptr(out), ptr(ws), nbytes, stream())
        else:
            C.sqdiff_sum(ptr(a), ptr(b), a.numel(), ptr(out), ptr(ws), nbytes, stream())
        ctx.save_for_backward(a, b)
        ctx.div = float(a.numel()) if mean else None
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = db = None
        for k, coef in ((0, 2.0), (1, -2.0)):
            if not ctx.needs_input_grad[k]:
                continue
            d = torch.empty_like(a)
            if ctx.div is None:
                C.sqdiff_grad(ptr(a), ptr(b), ptr(g), coef, ptr(d), a.numel(), stream())
            else:
                C.sqdiff_grad_groups(ptr(a), ptr(b), ptr(g), 0, ctx.div, coef, ptr(d), a.numel(), 1, stream())
            if k == 0:
                da = d
            else:
                db = d
        return da, db, None


class MSETargetFn(Function):
    """nn.MSELoss()(pred, target.detach()) of the supervised baseline (reference srl_baselines/supervised.py:85,103) — loss and
    d loss / d pred for a unit incoming gradient in ONE launch (srlz_mse_target_fwd); backward scales the latter by the incoming
    scalar (srlz_scale_by_scalar).  The target carries no gradient."""

    @staticmethod
    def forward(ctx, pred, target):
        if target.requires_grad:
            raise C.SrlzError("mse_target: the target must not require a gradient")
        pred, target = _check(pred, "mse_target prediction"), _check(target, "mse_target target")
        if pred.dim() != 2 or pred.shape != target.shape:
            raise C.SrlzError("mse_target: prediction %s and target %s must be the same [B, S]" % (tuple(pred.shape), tuple(target.shape)))
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        unit = torch.empty_like(pred)
        C.mse_target_fwd(ptr(pred), ptr(target), pred.shape[0], pred.shape[1], ptr(loss), ptr(unit), stream())
        ctx.save_for_backward(unit)
        return loss

    @staticmethod
    def backward(ctx, g):
        unit, = ctx.saved_tensors
        dpred = torch.empty_like(unit)
        C.scale_by_scalar(ptr(unit), ptr(_check(g, "mse_target gradient")), 1.0, 1.0, ptr(dpred), unit.numel(), stream())
        return dpred, None


def mse_target(pred, target):
    return MSETargetFn.apply(pred, target)


class DropoutFn(Function):
    """F.dropout(x, p, training=True) (reference models/supervised.py:26) with the mask the caller drew: y = x * mask / (1 - p),
    dx = dy * mask / (1 - p) (srlz_dropout_fwd / srlz_dropout_bwd).  mask: uint8 [rows, cols] on x's device."""

    @staticmethod
    def forward(ctx, x, mask, p):
        x = _check(x, "dropout input")
        if mask.dtype != torch.uint8 or mask.device != x.device or tuple(mask.shape) != tuple(x.shape) or x.dim() != 2:
            raise C.SrlzError("dropout: the mask must be a uint8 tensor of the input's [rows, cols] on its device")
        if not 0.0 <= p < 1.0:
            raise C.SrlzError("dropout: p = %r must lie in [0, 1)" % (p,))
        mask = mask if mask.is_contiguous() else mask.contiguous()
        y = torch.empty_like(x)
        C.dropout_fwd(ptr(x), ptr(mask), 1.0 - p, ptr(y), x.shape[0], x.shape[1], stream())
        ctx.save_for_backward(mask)
        ctx.keep = 1.0 - p
        return y

    @staticmethod
    def backward(ctx, dy):
        mask, = ctx.saved_tensors
        dy = _check(dy, "dropout dy")
        dx = torch.empty_like(dy)
        C.dropout_bwd(ptr(dy), ptr(mask), ctx.keep, ptr(dx), dy.shape[0], dy.shape[1], stream())
        return dx, None, None


def weighted(loss, weight):
    """weight * loss — what every loss function of the reference returns (losses/losses.py:102-256; the trainer itself reads the
    terms from the LossManager) — as one HIP launch: 0 + weight * loss with a separately rounded product is exactly that."""
    return TotalLossFn.apply((float(weight),), None, loss)


def add_scalars(a, b):
    """a + b of two 0-dim loss tensors as one HIP launch (srlz_weighted_total with weights 1, 1: (0 + 1 * a) + 1 * b is exactly a + b)."""
    return TotalLossFn.apply((1.0, 1.0), None, a, b)


class FanOutFn(Function):
    """A tensor with several consumers, made explicit: n aliases go out, and the backward sums the gradients that come back with ONE
    launch in a fixed order (srlz_sum_terms: ((g0 + g1) + g2) + g3) — what autograd would otherwise do with one accumulation kernel
    per extra consumer.  An alias nobody differentiates through contributes nothing."""

    @staticmethod
    def forward(ctx, t, n):
        ctx.set_materialize_grads(False)
        return tuple(t.view_as(t) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        terms = [_check(g, "fan-out gradient") for g in grads if g is not None]
        if not terms:
            return None, None
        if len(terms) == 1:
            return terms[0], None
        out = torch.empty_like(terms[0])
        while len(terms) > 1:  # (at most four terms per launch)
            head, terms = terms[:4], terms[4:]
            ptrs = (ctypes.c_void_p * len(head))(*[g.data_ptr() for g in head])
            C.sum_terms(ptrs, len(head), ptr(out), out.numel(), stream())
            terms = [out] + terms
            if len(terms) > 1:
                out = torch.empty_like(out)
        return terms[0], None


def fan_out(t, n):
    """n aliases of t whose gradients are summed by one launch (FanOutFn); t itself n times when it carries no gradient."""
    if n <= 1 or not (torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled()):
        return (t,) * n
    return FanOutFn.apply(t, n)


class Fan(object):
    """Hands out the aliases of a FanOutFn one consumer at a time: Fan(t, n).take() n times.  n <= 1 (or a tensor without gradient):
    the tensor itself."""

    def __init__(self, t, n):
        self.parts = list(fan_out(t, n)) if n > 1 else None
        self.t = t

    def take(self):
        return self.parts.pop() if self.parts else self.t


class CatColsFn(Function):
    """th.cat((a, b), dim=1) of two [B, *] matrices — the input of the inverse / reward heads (forward_inverse.py:62,78-95) — and the
    split of its gradient, one launch each."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _check(a, "cat input"), _check(b, "cat input")
        assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0]
        out = torch.empty((a.shape[0], a.shape[1] + b.shape[1]), dtype=torch.float32, device=a.device)
        C.cat_cols(ptr(a), ptr(b), ptr(out), a.shape[0], a.shape[1], b.shape[1], stream())
        ctx.cols = (a.shape[1], b.shape[1])
        return out

    @staticmethod
    def backward(ctx, d):
        d = _check(d, "cat gradient")
        ca, cb = ctx.cols
        da = torch.empty((d.shape[0], ca), dtype=torch.float32, device=d.device) if ctx.needs_input_grad[0] else None
        db = torch.empty((d.shape[0], cb), dtype=torch.float32, device=d.device) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            C.split_cols(ptr(d), ptr(da), ptr(db), d.shape[0], ca, cb, stream())
        return da, db


class ForwardModelFn(Function):
    """next-state prediction as ONE node (forward_inverse.py:27-37): state + Linear([state ; onehot(action)]).  The concatenation is
    one launch, the residual add sits in the GEMM's epilogue (separately rounded, as `state + self.forward_net(concat)` rounds it);
    backward: d state = dy + (dy . W)[:, :S] — the residual branch's gradient in the data-gradient GEMM's epilogue, only the state
    columns computed — and the weight / bias gradients of the linear layer."""

    @staticmethod
    def forward(ctx, state, action, w, b, n_actions):
        state, w = _check(state, "state"), _check(w, "forward model weight")
        action = action.contiguous()
        assert action.dtype == torch.int64 and action.device == state.device
        m, sdim = state.shape
        k = sdim + n_actions
        assert tuple(w.shape) == (sdim, k)
        cat = torch.empty((m, k), dtype=torch.float32, device=state.device)
        C.concat_onehot(ptr(state), ptr(action), ptr(cat), m, sdim, n_actions, stream())
        y = torch.empty((m, sdim), dtype=torch.float32, device=state.device)
        nbytes = C.linear_workspace(m, sdim, k)
        ws = _ws(nbytes, state.device)
        C.linear_fwd_res(ptr(cat), ptr(w), ptr(b), ptr(state), ptr(y), m, sdim, k, 0, ptr(ws), nbytes, stream())
        ctx.save_for_backward(cat, w)
        ctx.params = (b,)
        ctx.dims = (m, sdim, k)
        return y

    @staticmethod
    def backward(ctx, dy):
        cat, w = ctx.saved_tensors
        dy = _check(dy, "forward model dy")
        m, sdim, k = ctx.dims
        nbytes = C.linear_workspace(m, sdim, k)
        ws = _ws(nbytes, dy.device)
        dstate = None
        if ctx.needs_input_grad[0]:
            dstate = torch.empty((m, sdim), dtype=torch.float32, device=dy.device)
            C.linear_bwd_data_res(ptr(dy), ptr(w), ptr(dy), ptr(dstate), m, sdim, k, sdim, ptr(ws), nbytes, stream())
        dw = _gbuf(w)
        db = _gbuf(ctx.params[0]) if ctx.params[0] is not None else None
        C.linear_bwd_weight(ptr(dy), ptr(cat), ptr(dw), ptr(db), m, sdim, k, ptr(ws), nbytes, stream())
        return dstate, None, _give(w, dw), _give(ctx.params[0], db), None


# ----------------------------------------------------------------------------------------------------------------
# The two frames of a step as ONE batch (models/learner.py:392-393 calls the model on obs, then on next_obs).
# pair_cat joins them (zero-copy when they already are the two halves of one buffer), the model runs once inside
# batch_groups(2), pair_split hands the halves back to the loop body as views.  Losses that see both halves of a pair
# (pair_of) reduce them in one launch and return ONE gradient for the batched tensor.
# ----------------------------------------------------------------------------------------------------------------
def pair_cat(a, b):
    """[a ; b] along dim 0.  No copy when b starts where a ends in the same storage."""
    if is_u8_frames(a) and is_u8_frames(b):  # the loader's bytes: no gradient, any route
        a, b = _check_u8(a, "pair half"), _check_u8(b, "pair half")
        if a.shape == b.shape and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() \
                and b.storage_offset() == a.storage_offset() + a.numel():
            return torch.empty(0, dtype=a.dtype, device=a.device).set_(a.untyped_storage(), a.storage_offset(),
                                                                       (2 * a.shape[0],) + tuple(a.shape[1:]))
        return torch.cat([a, b], 0)
    a, b = frames_as_float(a), frames_as_float(b)
    a, b = _check(a, "pair half"), _check(b, "pair half")
    if a.shape != b.shape:
        raise C.SrlzError("pair_cat: the two halves differ in shape (%s vs %s)" % (tuple(a.shape), tuple(b.shape)))
    shape = (2 * a.shape[0],) + tuple(a.shape[1:])
    same = a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
    if same and b.storage_offset() == a.storage_offset() + a.numel() and not (a.requires_grad or b.requires_grad):
        return torch.empty(0, dtype=a.dtype, device=a.device).set_(a.untyped_storage(), a.storage_offset(), shape)
    return JoinFn.apply(a, b)


class JoinFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty((2 * a.shape[0],) + tuple(a.shape[1:]), dtype=torch.float32, device=a.device)
        C.join2(ptr(a), ptr(b), ptr(out), a.numel(), stream())
        return out

    @staticmethod
    def backward(ctx, d):
        half = d.shape[0] // 2
        return d[:half], d[half:]


class SplitFn(Function):
    """t [2B, ...] -> (t[:B], t[B:]) as views; the backward joins the two gradients (a missing one counts as zero)."""

    @staticmethod
    def forward(ctx, t):
        half = t.shape[0] // 2
        ctx.half_shape = (half,) + tuple(t.shape[1:])
        ctx.set_materialize_grads(False)
        return t[:half], t[half:]

    @staticmethod
    def backward(ctx, da, db):
        if da is None and db is None:
            return None
        dev = (da if da is not None else db).device
        out = torch.empty((2 * ctx.half_shape[0],) + ctx.half_shape[1:], dtype=torch.float32, device=dev)
        half = out.shape[0] // 2
        if da is not None and db is not None:
            da, db = _check(da, "pair grad"), _check(db, "pair grad")
            if da.numel() % 4 == 0 and da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0:
                C.join2(ptr(da), ptr(db), ptr(out), da.numel(), stream())
            else:
                out[:half].copy_(da)
                out[half:].copy_(db)
        else:
            out.zero_()
            (out[:half] if da is not None else out[half:]).copy_(da if da is not None else db)
        return out


def pair_split(t):
    """The two halves of a batched tensor, remembered as a pair so that pair-aware consumers can find the whole."""
    a, b = SplitFn.apply(t)
    # (weak references to the sibling: a <-> b would otherwise be a cycle that keeps the batched tensor — 300 MB for the
    # reconstructions at bs = 256 — alive until Python's cyclic collector runs)
    a._srlz_pair = (t, 0, weakref.ref(b))
    b._srlz_pair = (t, 1, weakref.ref(a))
    return a, b


def pair_of(a, b):
    """The batched tensor whose halves are exactly (a, b) — or None."""
    ra = getattr(a, "_srlz_pair", None)
    if ra is not None and ra[1] == 0 and ra[2]() is b:
        return ra[0]
    if torch.is_tensor(a) and torch.is_tensor(b) and not (a.requires_grad or b.requires_grad) and a.is_cuda and b.is_cuda \
            and a.dtype in (torch.float32, torch.uint8) and a.dtype == b.dtype and a.shape == b.shape \
            and a.is_contiguous() and b.is_contiguous() \
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() \
            and b.storage_offset() == a.storage_offset() + a.numel():
        return pair_cat(a, b)  # two adjacent constant tensors (obs, next_obs): a view over both
    return None


class SqDiffPairLossFn(Function):
    """The reconstruction (mean=True: sum/numel per frame, added) or generation (mean=False: sums added) loss of BOTH frames
    from batched tensors a, b [2B, ...] as ONE scalar: two launches forward, one backward, no scalar glue kernels.  Each
    frame's sum and the combination are rounded exactly like the two-call path's separate fp32 operations."""

    @staticmethod
    def forward(ctx, a, b, mean):
        a, b = _check(a, "loss input"), _check(b, "loss target")
        assert a.shape == b.shape and a.shape[0] % 2 == 0
        sums = torch.empty(2, dtype=torch.float32, device=a.device)
        comb = torch.empty((), dtype=torch.float32, device=a.device)
        nbytes = C.reduce_workspace(a.numel())
        ws = _ws(nbytes, a.device)
        C.sqdiff_pair_loss(ptr(a), ptr(b), a.numel() // 2, 1 if mean else 0, ptr(sums), ptr(comb), ptr(ws), nbytes, stream())
        ctx.save_for_backward(a, b)
        ctx.div = float(a.numel() // 2) if mean else 1.0
        return comb

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _check(g, "loss grad")
        da = db = None
        n = a.numel() // 2
        if ctx.needs_input_grad[0]:
            da = torch.empty_like(a)
            C.sqdiff_grad_groups(ptr(a), ptr(b), ptr(g), 0, ctx.div, 2.0, ptr(da), n, 2, stream())
        if ctx.needs_input_grad[1]:
            db = torch.empty_like(b)
            C.sqdiff_grad_groups(ptr(a), ptr(b), ptr(g), 0, ctx.div, -2.0, ptr(db), n, 2, stream())
        return da, db, None


class KLSumFn(Function):
    """-0.5 * sum(1 + logvar - mu^2 - exp(logvar)) — losses.py:253."""

    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = _check(mu, "mu"), _check(logvar, "logvar")
        out = torch.empty((), dtype=torch.float32, device=mu.device)
        nbytes = C.reduce_workspace(mu.numel())
        ws = _ws(nbytes, mu.device)
        C.kl_sum(ptr(mu), ptr(logvar), mu.numel(), ptr(out), ptr(ws), nbytes, stream())
        ctx.save_for_backward(mu, logvar)
        return out

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        g = g.contiguous()
        dmu, dlv = torch.zeros_like(mu), torch.zeros_like(logvar)
        C.kl_grad(ptr(mu), ptr(logvar), ptr(g), 1.0, ptr(dmu), ptr(dlv), mu.numel(), stream())
        return dmu, dlv


class ReparamFn(Function):
    """z = eps * exp(0.5*logvar) + mu — BaseModelVAE.reparameterize, models/models.py:157-163."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar, eps = _check(mu, "mu"), _check(logvar, "logvar"), _check(eps, "eps")
        z = torch.empty_like(mu)
        C.reparam_fwd(ptr(mu), ptr(logvar), ptr(eps), ptr(z), mu.numel(), stream())
        ctx.save_for_backward(logvar, eps)
        return z

    @staticmethod
    def backward(ctx, dz):
        logvar, eps = ctx.saved_tensors
        dz = _check(dz, "dz")
        dmu, dlv = torch.empty_like(dz), torch.empty_like(dz)
        C.reparam_bwd(ptr(dz), ptr(logvar), ptr(eps), ptr(dmu), ptr(dlv), dz.numel(), stream())
        return dmu, dlv, None


class CrossEntropyFn(Function):
    """nn.CrossEntropyLoss()(logits, target) (mean) — inverseModelLoss, losses.py:126-127."""

    @staticmethod
    def forward(ctx, logits, target):
        logits = _check(logits, "logits")
        target = target.contiguous()
        assert target.dtype == torch.int64 and target.device == logits.device
        b, a = logits.shape
        out = torch.empty((), dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits)
        C.cross_entropy(ptr(logits), ptr(target), b, a, ptr(out), ptr(dlogits), stream())
        ctx.save_for_backward(dlogits)
        return out

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        out = torch.empty_like(dlogits)
        C.scale_by_scalar(ptr(dlogits), ptr(_check(g, "loss grad")), 1.0, 1.0, ptr(out), dlogits.numel(), stream())
        return out, None


class PReLUFn(Function):
    """nn.PReLU() with a single slope — EmbeddingNet.fc[0], reference models/triplet.py:24."""

    @staticmethod
    def forward(ctx, x, slope):
        x, slope = _check(x, "prelu input"), _check(slope, "prelu slope")
        assert slope.numel() == 1
        y = torch.empty_like(x)
        C.prelu_fwd(ptr(x), ptr(slope), ptr(y), x.numel(), stream())
        ctx.save_for_backward(x, slope)
        ctx.params = (slope,)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, slope = ctx.saved_tensors
        dy = _check(dy, "prelu dy")
        dx = torch.empty_like(x)
        ds = _gbuf(ctx.params[0])
        C.prelu_bwd(ptr(x), ptr(slope), ptr(dy), ptr(dx), ptr(ds), x.numel(), stream())
        return dx, _give(ctx.params[0], ds)


class TripletLossFn(Function):
    """mean_b relu(|s - p|^2 - |s - n|^2 + alpha) — tripletLoss, reference losses/losses.py:360-376."""

    @staticmethod
    def forward(ctx, s, p, n, alpha):
        s, p, n = _check(s, "anchor states"), _check(p, "positive states"), _check(n, "negative states")
        assert s.shape == p.shape == n.shape and s.dim() == 2
        b, sd = s.shape
        out = torch.empty((), dtype=torch.float32, device=s.device)
        hinge = torch.empty(b, dtype=torch.float32, device=s.device)
        C.triplet_fwd(ptr(s), ptr(p), ptr(n), b, sd, alpha, ptr(out), ptr(hinge), stream())
        ctx.save_for_backward(s, p, n, hinge)
        return out

    @staticmethod
    def backward(ctx, g):
        s, p, n, hinge = ctx.saved_tensors
        g = g.contiguous()
        ds, dp, dn = torch.empty_like(s), torch.empty_like(p), torch.empty_like(n)
        C.triplet_bwd(ptr(s), ptr(p), ptr(n), ptr(hinge), ptr(g), s.shape[0], s.shape[1], ptr(ds), ptr(dp), ptr(dn), stream())
        return ds, dp, dn, None


class RewardPriorFn(Function):
    """1 - mean_j |clamp(corr[S, j], -1, 1)| of the correlation matrix of cat([states, rewards], 1)^T — rewardPriorLoss with
    correlationMatrix, reference losses/losses.py:290-304, losses/utils.py:120-134.  `rewards`: the raw float rewards [B] or [B, 1].
    One launch forward (fp64 column statistics, kept for the backward), one launch backward."""

    @staticmethod
    def forward(ctx, states, rewards):
        states, rewards = _check(states, "reward-prior states"), _check(rewards, "reward-prior rewards")
        if states.dim() != 2 or rewards.numel() != states.shape[0]:
            raise C.SrlzError("reward prior: states [B, S] and rewards [B] expected, got %s and %s"
                              % (tuple(states.shape), tuple(rewards.shape)))
        b, s = states.shape
        if b < 2:
            raise C.SrlzError("reward prior: the correlation needs at least 2 rows (got %d)" % b)
        nbytes = C.reward_prior_workspace(s)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=states.device)
        out = torch.empty((), dtype=torch.float32, device=states.device)
        C.reward_prior_fwd(ptr(states), ptr(rewards), b, s, ptr(out), ptr(ws), nbytes, stream())
        ctx.save_for_backward(states, rewards, ws)
        return out

    @staticmethod
    def backward(ctx, g):
        states, rewards, ws = ctx.saved_tensors
        b, s = states.shape
        ds = torch.empty_like(states)
        C.reward_prior_bwd(ptr(states), ptr(rewards), ptr(ws), ws.numel() * 8, ptr(_check(g, "loss grad")), b, s, ptr(ds), stream())
        return ds, None


_EP_TICKETS = {}


def _episode_ticket(device):
    """The episode-prior forward's completion counter (one int per device, zero between launches)."""
    t = _EP_TICKETS.get(device.index)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=device)
        _EP_TICKETS[device.index] = t
    return t


class EpisodePriorFn(Function):
    """BCELoss(reduction='sum')(Discriminator(cat(s, s[others])), same) with the gradient into the states reversed — episodePriorLoss
    with ReverseLayerF (lambda = 1) and Discriminator, reference losses/losses.py:307-359, models/priors.py:129-175.
    `others`: int32 [B] indices in [0, B) — a device tensor as losses.episodeInputs uploads it, or a host tensor / array, which is
    range-checked here and uploaded (on the device an index outside the batch pairs its row with itself, include/srlz.h);
    `same`: float32 [B] (1 where others[i] is in row i's episode);
    `disc_params`: net.0.weight, net.0.bias, net.2.weight, net.2.bias, net.4.weight, net.4.bias.  One launch forward, two backward;
    the six parameter gradients are written straight into the gradient bucket when the parameters live there."""

    @staticmethod
    def forward(ctx, states, others, same, w1, b1, w2, b2, w3, b3):
        states, same = _check(states, "episode-prior states"), _check(same, "episode-prior targets")
        if states.dim() != 2:
            raise C.SrlzError("episode prior: states [B, S] expected, got %s" % (tuple(states.shape),))
        b, s = states.shape
        if not torch.is_tensor(others) or others.device.type == "cpu":
            host = torch.as_tensor(others)
            if host.dtype not in (torch.int32, torch.int64) or host.numel() != b or \
                    (b and (int(host.min()) < 0 or int(host.max()) >= b)):
                raise C.SrlzError("episode prior: partner indices must be %d integers in [0, %d)" % (b, b))
            others = host.to(torch.int32).to(states.device)
        if others.dtype != torch.int32 or others.device != states.device or others.numel() != b or same.numel() != b:
            raise C.SrlzError("episode prior: others must be int32 [%d] and same float32 [%d] on the states' device" % (b, b))
        shapes = ((64, 2 * s), (64,), (64, 64), (64,), (1, 64), (1,))
        params = (w1, b1, w2, b2, w3, b3)
        for p, shape in zip(params, shapes):
            if tuple(p.shape) != shape:
                raise C.SrlzError("episode prior: discriminator parameter of shape %s, expected %s" % (tuple(p.shape), shape))
        ps = [_check(p, "discriminator parameter") for p in params]
        others = others.contiguous()
        nbytes = C.episode_prior_workspace(b, s)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=states.device)
        out = torch.empty((), dtype=torch.float32, device=states.device)
        C.episode_prior_fwd(ptr(states), ptr(others), ptr(same), b, s, *[ptr(p) for p in ps], ptr(out), ptr(ws), nbytes,
                            ptr(_episode_ticket(states.device)), stream())
        ctx.save_for_backward(states, others, same, ws, ps[0], ps[2], ps[4])
        ctx.params = params
        return out

    @staticmethod
    def backward(ctx, g):
        states, others, same, ws, w1, w2, w3 = ctx.saved_tensors
        b, s = states.shape
        ds = torch.empty_like(states)
        grads = [_gbuf(p) for p in ctx.params]
        C.episode_prior_bwd(ptr(states), ptr(others), ptr(same), ptr(_check(g, "loss grad")), b, s, ptr(w1), ptr(w2), ptr(w3), ptr(ws),
                            ws.numel(), ptr(ds), *[ptr(x) for x in grads], stream())
        return (ds, None, None) + tuple(_give(p, x) for p, x in zip(ctx.params, grads))


_ONES = {}


class ReverseLayerF(Function):
    """Identity forward, -lambda * gradient backward (reference models/priors.py:129-152).  The episode prior applies the reversal
    inside EpisodePriorFn's backward; this stand-alone form is kept for callers of the reference's name."""

    @staticmethod
    def forward(ctx, x, lambda_):
        ctx.lambda_ = float(lambda_)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        dy = _check(dy, "reversed gradient")
        one = _ONES.get(dy.device.index)
        if one is None:
            one = _ONES[dy.device.index] = torch.ones(1, dtype=torch.float32, device=dy.device)
        dx = torch.empty_like(dy)
        C.scale_by_scalar(ptr(dy), ptr(one), 1.0, -ctx.lambda_, ptr(dx), dy.numel(), stream())
        return dx, None


class ConcatOneHotFn(Function):
    """cat([s, onehot(a)], 1) — forwardModel's input, forward_inverse.py:30 + models/models.py:229-237."""

    @staticmethod
    def forward(ctx, s, a, n_actions):
        s = _check(s, "state")
        a = a.contiguous()
        assert a.dtype == torch.int64 and a.device == s.device
        b, sdim = s.shape
        cat = torch.empty((b, sdim + n_actions), dtype=torch.float32, device=s.device)
        C.concat_onehot(ptr(s), ptr(a), ptr(cat), b, sdim, n_actions, stream())
        ctx.sdim = sdim
        return cat

    @staticmethod
    def backward(ctx, dcat):
        return dcat[:, :ctx.sdim].contiguous(), None, None


def _eval_host_array(a, name, who="knn"):
    """numpy / torch, float32 / float64, 2-D, finite -> C-contiguous float64 numpy (an exact conversion)."""
    import numpy as np
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError("%s: %s must be float32 or float64 (got %s)" % (who, name, a.dtype))
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("%s: %s must be a non-empty [rows, D] array (got shape %s)" % (who, name, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s: %s holds NaN or infinite values" % (who, name))
    return np.ascontiguousarray(a, dtype=np.float64)


KNN_MAX_K = 32  # include/srlz.h, srlz_knn_f64


def knn(db, k, queries=None):
    """The k nearest rows of `db` [N, D] for every row of `queries` [Q, D] (None: the database itself, so every row finds itself
    first) — the exact fp64 search of csrc/knn.hip in place of the reference's ball tree (evaluation/knn_images.py:83-84).
    numpy or torch, float32 or float64; uploaded as fp64.  Order: (dist2, index) ascending, equal distances to the lower index.
    :return: (idx int64 [Q, k], dist2 float64 [Q, k]) as CPU numpy — SQUARED distances.
    ValueError: non-finite input, mismatched D, k outside [1, min(32, N)].  RuntimeError without a GPU: there is no CPU fallback."""
    import numpy as np
    dbh = _eval_host_array(db, "db")
    qh = dbh if queries is None else _eval_host_array(queries, "queries")
    if qh.shape[1] != dbh.shape[1]:
        raise ValueError("knn: queries have D = %d, the database D = %d" % (qh.shape[1], dbh.shape[1]))
    k = int(k)
    n, d = dbh.shape
    nq = qh.shape[0]
    if k < 1 or k > n or k > KNN_MAX_K:
        raise ValueError("knn: k must lie in [1, min(%d, N)] (k = %d, N = %d)" % (KNN_MAX_K, k, n))
    if n * d >= 2 ** 31 or nq * k >= 2 ** 31:
        raise ValueError("knn: N * D and Q * k must stay below 2^31 (N = %d, D = %d, Q = %d, k = %d)" % (n, d, nq, k))
    if not torch.cuda.is_available():
        raise C.SrlzError("knn runs on the GPU only (torch.cuda.is_available() is False): the srl-zoo_amd build has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    db_d = torch.from_numpy(dbh).to(device)
    q_d = db_d if queries is None else torch.from_numpy(qh).to(device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=device)
    dist2 = torch.empty((nq, k), dtype=torch.float64, device=device)
    nbytes = C.knn_workspace(n, nq, d, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    C.knn_f64(ptr(db_d), n, ptr(q_d), nq, d, k, ptr(idx), ptr(dist2), ptr(ws), nbytes, stream())
    return idx.cpu().numpy().astype(np.int64), dist2.cpu().numpy()


GTC_MAX_G = 16  # include/srlz.h, srlz_gtc_rows_f64


def gt_correlation(gt, states):
    """Rows 0 .. G-1 of np.corrcoef(gt, states, rowvar=0): the correlation of every ground-truth dimension with all G + S columns of
    [gt | states] — the rows the reference's plotCorrelation reads (plotting/representation_plot.py:283, :296-300) — by the two-pass
    fp64 kernels of csrc/gtc.hip.  gt [N, G] and states [N, S]: host arrays (numpy or torch), float32 or float64, uploaded as fp64.
    A zero-variance column gives NaN where numpy gives NaN; nothing is raised for it.
    :return: corr float64 [G, G + S] as CPU numpy
    ValueError: non-finite input, mismatched N, N < 2, G outside [1, 16], S < 1, N * (G + S) >= 2^31.  RuntimeError without a GPU:
    there is no CPU fallback."""
    gth = _eval_host_array(gt, "gt", "gt_correlation")
    sth = _eval_host_array(states, "states", "gt_correlation")
    n, g = gth.shape
    s = sth.shape[1]
    if sth.shape[0] != n:
        raise ValueError("gt_correlation: gt has %d rows, states %d" % (n, sth.shape[0]))
    if n < 2:
        raise ValueError("gt_correlation: needs N >= 2 rows (N = %d)" % n)
    if g > GTC_MAX_G:
        raise ValueError("gt_correlation: G must lie in [1, %d] (G = %d)" % (GTC_MAX_G, g))
    if n * (g + s) >= 2 ** 31:
        raise ValueError("gt_correlation: N * (G + S) must stay below 2^31 (N = %d, G = %d, S = %d)" % (n, g, s))
    if not torch.cuda.is_available():
        raise C.SrlzError("gt_correlation runs on the GPU only (torch.cuda.is_available() is False): the srl-zoo_amd build has no "
                          "CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    gt_d = torch.from_numpy(gth).to(device)
    st_d = torch.from_numpy(sth).to(device)
    corr = torch.empty((g, g + s), dtype=torch.float64, device=device)
    colstats = torch.empty((2, g + s), dtype=torch.float64, device=device)
    nbytes = C.gtc_workspace(n, g, s)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    C.gtc_rows_f64(ptr(gt_d), ptr(st_d), n, g, s, ptr(corr), ptr(colstats), ptr(ws), nbytes, stream())
    return corr.cpu().numpy()


def _check_decoded(dec, who):
    """A decoded batch [N, 3, W, H] for csrc/latent.hip: float32 on the GPU, three channels — the assertion of the reference's
    deNormalize (preprocessing/utils.py:49) as an SrlzError."""
    if not torch.is_tensor(dec) or dec.dim() != 4:
        raise C.SrlzError("%s: dec must be a [N, 3, W, H] tensor (got %s)" % (who, tuple(dec.shape) if torch.is_tensor(dec) else type(dec)))
    dec = _check(dec, "%s: dec" % who)
    if dec.shape[1] != 3:
        raise C.SrlzError("%s: dec must have 3 channels, [N, 3, W, H] (got %s)" % (who, tuple(dec.shape)))
    return dec


def decoded_to_bgr(dec):
    """Decoded images [N, 3, W, H] (the reference's tensor layout) -> the float32 [N, H, W, 3] BGR images of the reference's getImage
    (evaluation/enjoy_latent.py:36-39): transposed, de-normalised with the image_net constants, clipped to [0, 1], channels flipped
    — bit for bit the numpy expression (csrc/latent.hip)."""
    dec = _check_decoded(dec, "decoded_to_bgr")
    n, _, w, h = dec.shape
    img = torch.empty((n, h, w, 3), dtype=torch.float32, device=dec.device)
    C.decoded_to_bgr(ptr(dec), n, w, h, ptr(img), stream())
    return img


def sheet_size(n, w, h, cols, gap):
    """(sheet_h, sheet_w) of n pictures of h x w in a grid of `cols` columns with `gap` pixels between the tiles and around the grid."""
    rows = (n + cols - 1) // cols
    return rows * h + (rows + 1) * gap, cols * w + (cols + 1) * gap


def decoded_to_sheet(dec, cols, gap=2, fill=255, rgb=True):
    """Decoded images [N, 3, W, H] -> ONE uint8 sheet [SH, SW, 3] on the device: picture i at tile (i // cols, i % cols), `gap` pixels
    of `fill` between the tiles and around the grid, empty tiles `fill`.  Pixel values are np.rint(v * 255) of decoded_to_bgr's v;
    rgb=True keeps R, G, B (what PIL wants), False writes B, G, R (csrc/latent.hip)."""
    dec = _check_decoded(dec, "decoded_to_sheet")
    n, _, w, h = dec.shape
    cols, gap, fill = int(cols), int(gap), int(fill)
    if cols < 1 or gap < 0 or not 0 <= fill <= 255:
        raise C.SrlzError("decoded_to_sheet: needs cols >= 1, gap >= 0 and fill in [0, 255] (cols=%d, gap=%d, fill=%d)" % (cols, gap, fill))
    sh, sw = sheet_size(n, w, h, cols, gap)
    if sh * sw * 3 >= 2 ** 31:
        raise C.SrlzError("decoded_to_sheet: the sheet of %d x %d pixels must stay below 2^31 bytes" % (sh, sw))
    sheet = torch.empty((sh, sw, 3), dtype=torch.uint8, device=dec.device)
    C.decoded_to_sheet_u8(ptr(dec), n, w, h, cols, gap, fill, 1 if rgb else 0, ptr(sheet), sh, sw, stream())
    return sheet


REWARD_PROBE_MAX_S = 512  # include/srlz.h, srlz_reward_probe_fit: the parameters and their Adam moments stay in LDS
REWARD_PROBE_COUNTS = ("correct", "correct_0", "correct_1", "rows_0", "rows_1")  # the five int64 counters, in this order
_REWARD_PROBE_TICKET = {}


class RewardProbeData(object):
    """The dataset of the reward probe on the device: states fp32 [N, S] and labels int32 [N] (reward_probe_data)."""

    def __init__(self, states, labels):
        self.states, self.labels = states, labels
        self.n, self.s = int(states.shape[0]), int(states.shape[1])


def reward_probe_data(states, labels):
    """states [N, S] (host array, numpy or torch, float32 or float64, finite) and labels [N] (integers in {0, 1}) -> RewardProbeData,
    validated here on the host ONCE and uploaded for the whole run: the kernels never see a label they cannot count.
    ValueError: shapes, a non-integer label array, a label outside {0, 1}, S outside [1, 512].  SrlzError without a GPU."""
    import numpy as np
    sth = _eval_host_array(states, "states", "reward_probe")
    lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if lab.dtype.kind not in "iu":
        raise ValueError("reward_probe: labels must be integers (got %s)" % lab.dtype)
    if lab.ndim != 1 or lab.shape[0] != sth.shape[0]:
        raise ValueError("reward_probe: labels must be [N] with N = %d rows of states (got shape %s)" % (sth.shape[0], lab.shape))
    if sth.shape[0] < 2:
        raise ValueError("reward_probe: needs N >= 2 rows of states (N = %d)" % sth.shape[0])
    if sth.shape[1] > REWARD_PROBE_MAX_S:
        raise ValueError("reward_probe: the state dimension must lie in [1, %d] (S = %d)" % (REWARD_PROBE_MAX_S, sth.shape[1]))
    if lab.min() < 0 or lab.max() > 1:
        raise ValueError("reward_probe: labels must lie in {0, 1}, found [%d, %d]" % (int(lab.min()), int(lab.max())))
    if not torch.cuda.is_available():
        raise C.SrlzError("reward_probe runs on the GPU only (torch.cuda.is_available() is False): the srl-zoo_amd build has no "
                          "CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    return RewardProbeData(torch.from_numpy(sth.astype(np.float32)).to(device),
                           torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(device))


def reward_probe_n_params(s):
    """Linear(2S, 4), Linear(4, 4), Linear(4, 2) with their biases, flat in state_dict order."""
    return 8 * int(s) + 34


def reward_probe_chunk_rows(s):
    """Rows of a minibatch that srlz_reward_probe_fit processes at a time (a function of S alone)."""
    return C.reward_probe_chunk_rows(int(s))


def reward_probe_stats(device=None):
    """Zeroed statistics of one phase: (running_loss float64 [1], counts int64 [5] in the order of REWARD_PROBE_COUNTS)."""
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.zeros(1, dtype=torch.float64, device=device), torch.zeros(5, dtype=torch.int64, device=device)


def _reward_probe_buffer(t, name, dtype, numel, data, exact=False, who="reward_probe"):
    if not torch.is_tensor(t) or t.device != data.states.device:
        raise C.SrlzError("%s: %s must be a tensor on %s: the srl-zoo_amd hot path has no CPU fallback" % (who, name, data.states.device))
    if t.dtype != dtype:
        raise ValueError("%s: %s must be %s (got %s)" % (who, name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    if (t.numel() != numel) if exact else (t.numel() < numel):
        raise ValueError("%s: %s holds %d elements, needs %s%d (S = %d)" % (who, name, t.numel(), "" if exact else "at least ",
                                                                          numel, data.s))
    return t


def _reward_probe_table(data, idx, who="reward_probe"):
    """The minibatch table: int32 [n, B] on the HOST (the launcher checks every entry there), C-contiguous -> (host, device)."""
    import numpy as np
    if not isinstance(data, RewardProbeData):
        raise ValueError("%s: data must come from reward_probe_data()" % who)
    if isinstance(idx, np.ndarray):
        idx = torch.from_numpy(idx)
    if not torch.is_tensor(idx) or idx.device.type != "cpu":
        raise ValueError("%s: idx must be a host tensor (it is checked on the host, then uploaded)" % who)
    if idx.dtype != torch.int32:
        raise ValueError("%s: idx must be int32 (got %s)" % (who, idx.dtype))
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError("%s: idx must be a non-empty [minibatches, B] table (got shape %s)" % (who, tuple(idx.shape)))
    if not idx.is_contiguous():
        raise ValueError("%s: idx must be contiguous" % who)
    return idx, idx.to(data.states.device)


def reward_probe_fit(data, idx, params, m, v, t0, lr, running_loss, counts, step_loss=None, betas=(0.9, 0.999), eps=1e-8):
    """idx.shape[0] consecutive Adam steps of the reward probe (Linear(2S,4)-ReLU-Linear(4,4)-ReLU-Linear(4,2), cross-entropy) in
    ONE launch of srlz_reward_probe_fit: minibatch s is the rows [states[i] ; states[i + 1]] for i in idx[s].  No autograd: the
    kernel owns the backward.  params / m / v: float32 [8S + 34] on the device in state_dict order, updated in place; t0: the Adam
    steps already taken; running_loss float64 [1] and counts int64 [5] are added to (reward_probe_stats); step_loss: float64
    [>= steps] for the mean loss of every step, or None."""
    idx_h, idx_d = _reward_probe_table(data, idx)
    n_steps, b = int(idx_h.shape[0]), int(idx_h.shape[1])
    n_par = reward_probe_n_params(data.s)
    for t, name in ((params, "params"), (m, "m"), (v, "v")):
        _reward_probe_buffer(t, name, torch.float32, n_par, data, exact=True)
    _reward_probe_buffer(running_loss, "running_loss", torch.float64, 1, data)
    _reward_probe_buffer(counts, "counts", torch.int64, 5, data)
    if step_loss is not None:
        _reward_probe_buffer(step_loss, "step_loss", torch.float64, n_steps, data)
    C.reward_probe_fit(ptr(data.states), ptr(data.labels), data.n, data.s, ptr(idx_d), ctypes.c_void_p(idx_h.data_ptr()), n_steps, b,
                       ptr(params), ptr(m), ptr(v), int(t0), float(lr), float(betas[0]), float(betas[1]), float(eps),
                       ptr(running_loss), ptr(counts), ptr(step_loss), stream())


def reward_probe_eval(data, idx, params, running_loss, counts):
    """The forward, loss (float64 per row) and counts of idx.shape[0] minibatches in ONE launch of srlz_reward_probe_eval; params
    are only read, running_loss and counts are added to."""
    idx_h, idx_d = _reward_probe_table(data, idx)
    n_batches, b = int(idx_h.shape[0]), int(idx_h.shape[1])
    _reward_probe_buffer(params, "params", torch.float32, reward_probe_n_params(data.s), data, exact=True)
    _reward_probe_buffer(running_loss, "running_loss", torch.float64, 1, data)
    _reward_probe_buffer(counts, "counts", torch.int64, 5, data)
    device = data.states.device
    ticket = _REWARD_PROBE_TICKET.get(device.index)
    if ticket is None:
        ticket = _REWARD_PROBE_TICKET[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    nbytes = C.reward_probe_eval_workspace(n_batches, b)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
    C.reward_probe_eval(ptr(data.states), ptr(data.labels), data.n, data.s, ptr(idx_d), ctypes.c_void_p(idx_h.data_ptr()), n_batches, b,
                        ptr(params), ptr(running_loss), ptr(counts), ptr(ws), nbytes, ptr(ticket), stream())


def normalize_u8(frames, out=None):
    """uint8 [N,H,W,C] device tensor -> normalised fp32 [N,C,W,H] (the reference's observation tensor); `out`: where to
    write it (a contiguous [N,C,W,H] fp32 tensor, e.g. one half of a pair buffer)."""
    if frames.device.type != "cuda" or frames.dtype != torch.uint8:
        raise C.SrlzError("normalize_u8 expects a uint8 tensor on the GPU")
    frames = frames.contiguous()
    n, h, w, c = frames.shape
    if out is None:
        out = torch.empty((n, c, w, h), dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != (n, c, w, h) or out.dtype != torch.float32 or not out.is_contiguous():
        raise C.SrlzError("normalize_u8: `out` must be a contiguous float32 [N,C,W,H] tensor")
    C.normalize_u8(ptr(frames), ptr(out), n, h, w, c, stream())
    return out


def fold_grads(grad, stages):
    C.fold_grads(ptr(grad), ptr(stages), grad.numel(), stages.shape[0], stream())


def adam_step(p, g, m, v, lr, step, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    C.adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, step, grad_scale, stream())


def adam_step_dev(p, g, m, v, lr, step_dev, bc_dev, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    C.adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, ptr(step_dev), ptr(bc_dev),
                    grad_scale, stream())


def bn_replay(batch_stat, running_mean, running_var):
    C.bn_replay(ptr(batch_stat), BN_MOMENTUM, ptr(running_mean), ptr(running_var), stream())


def bn_replay_many(items):
    """[(batch_stat [128], running_mean, running_var, num_batches_tracked)] of up to 8 layers: one more momentum update each with the
    given batch statistics and the counters += 1, in ONE launch."""
    table = (C.BnReplayItem * len(items))()
    for i, (st, rm, rv, tick) in enumerate(items):
        table[i].batch_stat, table[i].running_mean, table[i].running_var = st.data_ptr(), rm.data_ptr(), rv.data_ptr()
        table[i].num_batches_tracked = tick.data_ptr() if tick is not None else None
    C.bn_replay_many(table, len(items), BN_MOMENTUM, stream())


# ----------------------------------------------------------------------------------------------------------------
# Deployment encoder (csrc/infer.hip): one eval-mode encoder block per launch, conv + BatchNorm + ReLU + MaxPool — models/models.py:47-63.
# Thin: the caller (srlz/deploy.py) owns every buffer; nothing is allocated here, and no autograd node is made.
# ----------------------------------------------------------------------------------------------------------------
INFER_IN, INFER_MID, INFER_LAST = C.INFER_IN, C.INFER_MID, C.INFER_LAST
INFER_POOL_PAD = {INFER_IN: 1, INFER_MID: 0, INFER_LAST: 0}  # models/models.py:52, 57, 62


def infer_desc(kind, n, c_in, hi, wi, strides=None, pool_pad=None, out_nchw=None):
    """srlz_infer_block_desc of `n` maps [c_in, hi, wi].  strides = element strides (n, c, y, x) of the input; None: the reference's
    planar bytes for kind IN, contiguous NHWC for the 64-channel kinds.  pool_pad / out_nchw default to the reference's block of that
    kind (the last block writes the NCHW-flat order the state head reads)."""
    if strides is None:
        strides = (c_in * hi * wi, hi * wi, wi, 1) if kind == INFER_IN else (hi * wi * 64, 1, wi * 64, 64)
    if pool_pad is None:
        pool_pad = INFER_POOL_PAD.get(kind, 0)
    if out_nchw is None:
        out_nchw = kind == INFER_LAST
    return C.InferBlockDesc(n, c_in, hi, wi, kind, pool_pad, 1 if out_nchw else 0, *[int(s) for s in strides])


def infer_supported(d):
    return bool(C.infer_block_supported(ctypes.byref(d)))


def infer_out_dims(d):
    """(hc, wc, hp, wp): convolution output (never stored) and pooled map of a supported descriptor; SrlzError for a rejected one."""
    v = [ctypes.c_int(0) for _ in range(4)]
    C.infer_block_out_dims(ctypes.byref(d), *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def infer_pack(weight, kind, out=None):
    """The kernels' copy of a Conv2d weight [64, c_in, k, k] (written into `out` when given: a refresh allocates nothing)."""
    weight = _check(weight.detach(), "infer_pack weight")
    c_in = weight.shape[1]
    nfl = C.infer_packed_floats(kind, c_in)
    k = 7 if kind == INFER_IN else 3
    if nfl <= 0 or tuple(weight.shape) != (64, c_in, k, k):
        raise C.SrlzError("infer_pack: no block of kind %d takes a weight of shape %s" % (kind, tuple(weight.shape)))
    if out is None:
        out = torch.empty(nfl, dtype=torch.float32, device=weight.device)
    elif out.numel() != nfl or out.dtype != torch.float32 or not out.is_contiguous():
        raise C.SrlzError("infer_pack: `out` must be %d contiguous float32 values" % nfl)
    C.infer_pack_weights(ptr(weight), ptr(out), kind, c_in, stream())
    return out


def infer_block(x, wpack, bnp, out, d, lut=None):
    """One launch: out = maxpool3x3s2(relu(conv(x) * scale + shift)) as `d` describes it.  x: uint8 frames (kind IN, with the
    normalisation table) or fp32 NHWC; `out` must hold n * 64 * hp * wp floats."""
    C.infer_block(ptr(x), ptr(lut), ptr(wpack), ptr(bnp), ptr(out), ctypes.byref(d), stream())
    return out


# ----------------------------------------------------------------------------------------------------------------
# Deployment decoder (csrc/infer_dec.hip): one eval-mode decoder layer per launch — models/models.py:65-83.  Blocks: ConvTranspose 3x3
# s2 + bias + BatchNorm affine + ReLU; out: ConvTranspose 4x4 s2 + bias to the decode tensor or to the picture's bytes.
# Thin: the caller (srlz/deploy.py) owns every buffer; nothing is allocated here, and no autograd node is made.
# ----------------------------------------------------------------------------------------------------------------
INFER_DEC_FIRST, INFER_DEC_MID, INFER_DEC_OUT = C.INFER_DEC_FIRST, C.INFER_DEC_MID, C.INFER_DEC_OUT


def infer_dec_desc(kind, n, hi, wi, c_out=None, out_u8=False, bgr=False, in_strides=None, out_strides=None, c_in=64):
    """srlz_infer_dec_desc of `n` maps [64, hi, wi].  c_out defaults to 64 (FIRST, MID) / 3 (OUT).  in_strides: element strides
    (n, c, y, x) of the input, None = the contiguous ones of that kind ([N,64,hi,wi] for FIRST, NHWC otherwise).  out_strides: byte
    output only, element strides (n, c, y, x) of the decode tensor [N,c_out,ho,wo] in the picture; None = the reference's planar
    [N,C,W,H] bytes."""
    if c_out is None:
        c_out = 3 if kind == INFER_DEC_OUT else 64
    if in_strides is None:
        in_strides = (64 * hi * wi, hi * wi, wi, 1) if kind == INFER_DEC_FIRST else (hi * wi * 64, 1, wi * 64, 64)
    if out_strides is None:
        ho, wo = (2 * hi + 2, 2 * wi + 2) if kind == INFER_DEC_OUT else (2 * hi + 1, 2 * wi + 1)
        out_strides = (c_out * ho * wo, ho * wo, wo, 1)
    return C.InferDecDesc(n, c_in, c_out, hi, wi, kind, 1 if out_u8 else 0, 1 if bgr else 0, *[int(s) for s in tuple(in_strides) + tuple(out_strides)])


def infer_dec_supported(d):
    return bool(C.infer_dec_supported(ctypes.byref(d)))


def infer_dec_out_dims(d):
    """(ho, wo) of a supported descriptor; SrlzError for a rejected one."""
    v = [ctypes.c_int(0) for _ in range(2)]
    C.infer_dec_out_dims(ctypes.byref(d), *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def infer_dec_pack(weight, kind, out=None):
    """The kernels' copy of a ConvTranspose2d weight [64, c_out, k, k] (written into `out` when given: a refresh allocates nothing)."""
    weight = _check(weight.detach(), "infer_dec_pack weight")
    c_out = weight.shape[1] if weight.dim() == 4 else -1
    nfl = C.infer_dec_packed_floats(kind, c_out)
    k = 4 if kind == INFER_DEC_OUT else 3
    if nfl <= 0 or tuple(weight.shape) != (64, c_out, k, k):
        raise C.SrlzError("infer_dec_pack: no layer of kind %d takes a weight of shape %s" % (kind, tuple(weight.shape)))
    if out is None:
        out = torch.empty(nfl, dtype=torch.float32, device=weight.device)
    elif out.numel() != nfl or out.dtype != torch.float32 or not out.is_contiguous():
        raise C.SrlzError("infer_dec_pack: `out` must be %d contiguous float32 values" % nfl)
    C.infer_dec_pack_weights(ptr(weight), ptr(out), kind, c_out, stream())
    return out


def infer_dec_block(x, wpack, bias, bnp, out, d):
    """One launch: out = relu((convT3x3s2(x) + bias) * scale + shift), fp32 NHWC; `out` must hold n * (2hi+1) * (2wi+1) * 64 floats."""
    C.infer_dec_block(ptr(x), ptr(wpack), ptr(bias), ptr(bnp), ptr(out), ctypes.byref(d), stream())
    return out


def infer_dec_out(x, wpack, bias, out, d):
    """One launch: convT4x4s2(x) + bias as fp32 [n,c_out,ho,wo], or (d.out_u8) as the picture's bytes by d's out strides."""
    C.infer_dec_out(ptr(x), ptr(wpack), ptr(bias), ptr(out), ctypes.byref(d), stream())
    return out


# ----------------------------------------------------------------------------------------------------------------
# Deployment dynamics (csrc/rollout.hip): R = N * K rows rolled T steps through forwardModel and rewardModel in one launch —
# models/forward_inverse.py:21-31, 78-95.  Thin: the caller (srlz/deploy.py) owns every buffer; nothing is allocated here beyond the
# upload of host plans, and no autograd node is made.
# ----------------------------------------------------------------------------------------------------------------
def rollout_supported(s, a, h=16, n_rewards=2):
    return bool(C.rollout_supported(int(s), int(a), int(h), int(n_rewards)))


def _rollout_f32(t, name, shape=None):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
        raise C.SrlzError("rollout: %s must be a contiguous float32 device tensor" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise C.SrlzError("rollout: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t.detach()


def rollout_plans(plans, n_actions, device):
    """A call's plans as a contiguous int32 device tensor.  Host plans (numpy, lists, CPU tensors) are range-checked against
    [0, n_actions) here and uploaded; device plans rely on the kernel's NaN rule (include/srlz.h) and are only converted to int32."""
    if not torch.is_tensor(plans) or plans.device.type == "cpu":
        host = torch.as_tensor(plans)
        if host.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise C.SrlzError("rollout: plans must be integers (got %s)" % (host.dtype,))
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= n_actions):
            raise C.SrlzError("rollout: plans must hold actions in [0, %d), got %d .. %d" % (n_actions, int(host.min()), int(host.max())))
        return host.to(torch.int32).contiguous().to(device)
    if plans.dtype not in (torch.int32, torch.int64):
        raise C.SrlzError("rollout: device plans must be int32 or int64 (got %s)" % (plans.dtype,))
    return plans.to(torch.int32).contiguous()


def rollout(states, plans, wf, bf, reward=None, final=None, returns=None, trajectory=None, reward_logits=None, gamma=1.0):
    """One launch of srlz_rollout.  states fp32 [N,S]; plans int [N,K,T] or [K,T] (shared by every environment, read with an
    environment stride of 0); wf / bf = forward_net.weight [S,S+A] / bias; reward = (w1, b1, w2, b2, w3, b3) of reward_net.0/2/4 or
    None (no reward work: returns / reward_logits must be None).  `final` [N,K,S] is made here when None; the other outputs are
    written only when given ([N,K], [N,K,T,S], [N,K,T,2]).  Returns `final`."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("rollout: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    wf = _rollout_f32(wf, "forward_net.weight")
    if wf.dim() != 2 or wf.shape[0] != s or wf.shape[1] <= s:
        raise C.SrlzError("rollout: forward_net.weight of shape %s does not take states of %d dimensions" % (tuple(wf.shape), s))
    a = wf.shape[1] - s
    bf = _rollout_f32(bf, "forward_net.bias", (s,))
    plans = rollout_plans(plans, a, states.device)
    if plans.device != states.device or plans.dim() not in (2, 3) or (plans.dim() == 3 and plans.shape[0] != n):
        raise C.SrlzError("rollout: plans must be [N,K,T] with N = %d or [K,T] on the states' device, got %s" % (n, tuple(plans.shape)))
    k, t = plans.shape[-2], plans.shape[-1]
    stride = k * t if plans.dim() == 3 else 0
    h, head = 0, (None,) * 6
    if reward is not None:
        h = reward[0].shape[0]
        shapes = ((h, 2 * s), (h,), (h, h), (h,), (2, h), (2,))
        head = tuple(_rollout_f32(p, "reward_net parameter", shape) for p, shape in zip(reward, shapes))
    if final is None:
        final = torch.empty((n, k, s), dtype=torch.float32, device=states.device)
    final = _rollout_f32(final, "final", (n, k, s))
    returns = _rollout_f32(returns, "returns", (n, k))
    trajectory = _rollout_f32(trajectory, "trajectory", (n, k, t, s))
    reward_logits = _rollout_f32(reward_logits, "reward_logits", (n, k, t, 2))
    C.rollout(ptr(states), ptr(plans), stride, ptr(wf), ptr(bf), *[ptr(p) for p in head], ptr(final), ptr(returns), ptr(trajectory),
              ptr(reward_logits), n, k, t, s, a, h, 2, float(gamma), stream())
    return final


# ----------------------------------------------------------------------------------------------------------------
# Deployment planner (csrc/plan.hip): a categorical cross-entropy method on the dynamics above, one launch per iteration, all of them
# enqueued here back to back.  Thin, as rollout: the caller owns every buffer, nothing is allocated and no autograd node is made.
# ----------------------------------------------------------------------------------------------------------------
def plan_supported(s, a, h, n_rewards, n_plans, horizon):
    return bool(C.plan_supported(int(s), int(a), int(h), int(n_rewards), int(n_plans), int(horizon)))


def plan_workspace(n, n_plans, horizon, keep_population=False):
    """Bytes of workspace of a plan_cem call; 0 for a shape it refuses."""
    return int(C.plan_workspace(int(n), int(n_plans), int(horizon), int(bool(keep_population))))


def _plan_buf(t, name, dtype, shape):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise C.SrlzError("plan_cem: %s must be a contiguous %s device tensor of shape %s" % (name, dtype, tuple(shape)))
    return t


def plan_cem(states, wf, bf, reward, n_plans, horizon, iterations, elites, sharpness, best_plan, best_return, cum, workspace,
             gamma=1.0, seed=0, init_weights=None, plans=None, returns=None):
    """`iterations` launches of plan_cem_kernel.  states fp32 [N,S]; wf / bf / reward = (w1 .. b3) as rollout takes them (the reward
    head is required); init_weights None (uniform) or int32 [N,T,A] / [T,A] on the device, every row's total positive and below 2^32;
    outputs best_plan int32 [N,T], best_return fp32 [N], cum int32 [N,T,A] (the bits are uint32); plans int32 [I,N,K,T] and returns
    fp32 [I,N,K] keep the whole population (both or neither); workspace: a uint8 device tensor of plan_workspace(...) bytes."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("plan_cem: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    wf = _rollout_f32(wf, "forward_net.weight")
    if wf.dim() != 2 or wf.shape[0] != s or wf.shape[1] <= s:
        raise C.SrlzError("plan_cem: forward_net.weight of shape %s does not take states of %d dimensions" % (tuple(wf.shape), s))
    a = wf.shape[1] - s
    bf = _rollout_f32(bf, "forward_net.bias", (s,))
    if reward is None:
        raise C.SrlzError("plan_cem: the planner scores by the reward head")
    h = reward[0].shape[0]
    shapes = ((h, 2 * s), (h,), (h, h), (h,), (2, h), (2,))
    head = tuple(_rollout_f32(p, "reward_net parameter", shape) for p, shape in zip(reward, shapes))
    k, t, it = int(n_plans), int(horizon), int(iterations)
    stride = 0
    if init_weights is not None:
        if tuple(init_weights.shape) not in ((t, a), (n, t, a)):
            raise C.SrlzError("plan_cem: init_weights must be [T,A] or [N,T,A], got %s" % (tuple(init_weights.shape),))
        stride = t * a if init_weights.dim() == 3 else 0
        init_weights = _plan_buf(init_weights, "init_weights", torch.int32, init_weights.shape)
    best_plan = _plan_buf(best_plan, "best_plan", torch.int32, (n, t))
    best_return = _plan_buf(best_return, "best_return", torch.float32, (n,))
    cum = _plan_buf(cum, "cum", torch.int32, (n, t, a))
    plans = _plan_buf(plans, "plans", torch.int32, (it, n, k, t))
    returns = _plan_buf(returns, "returns", torch.float32, (it, n, k))
    if not torch.is_tensor(workspace) or workspace.device.type != "cuda" or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise C.SrlzError("plan_cem: workspace must be a contiguous uint8 device tensor")
    C.plan_cem(ptr(states), ptr(wf), ptr(bf), *[ptr(p) for p in head], ptr(init_weights), stride, ptr(best_plan), ptr(best_return),
               ptr(cum), ptr(plans), ptr(returns), ptr(workspace), workspace.numel(), n, k, t, s, a, h, 2, it, int(elites),
               int(sharpness), float(gamma), int(seed) & 0xFFFFFFFFFFFFFFFF, stream())
    return best_plan


# ----------------------------------------------------------------------------------------------------------------
# Goal-distance scores (csrc/rollout_tile.h with its goal term compiled in): the rollout and the planner above scored by
# prob_t - w * |s_{t+1} - goal|^2, or by -w * |s_{t+1} - goal|^2 alone without a reward head (include/srlz.h states the rule).  Thin, as
# rollout and plan_cem: the caller owns every buffer.
# ----------------------------------------------------------------------------------------------------------------
GOAL_MODES = {"running": 0, "final": 1}


def rollout_goal_supported(s, a, h=16, n_rewards=2, has_reward=True):
    return bool(C.rollout_goal_supported(int(s), int(a), int(h), int(n_rewards), int(bool(has_reward))))


def plan_goal_supported(s, a, h, n_rewards, has_reward, n_plans, horizon):
    return bool(C.plan_goal_supported(int(s), int(a), int(h), int(n_rewards), int(bool(has_reward)), int(n_plans), int(horizon)))


def plan_goal_workspace(n, n_plans, horizon, keep_population=False):
    """Bytes of workspace of a plan_cem_goal call; 0 for a shape it refuses."""
    return int(C.plan_goal_workspace(int(n), int(n_plans), int(horizon), int(bool(keep_population))))


def _goal_args(goal, n, s, goal_mode, who):
    """(goal tensor, environment stride, mode as the C ABI's int) of a goal fp32 [S] (shared, stride 0) or [N,S]."""
    goal = _rollout_f32(goal, "goal")
    if goal is None or tuple(goal.shape) not in ((s,), (n, s)):
        raise C.SrlzError("%s: goal must be [S] = %s or [N,S] = %s, got %s"
                          % (who, (s,), (n, s), None if goal is None else tuple(goal.shape)))
    if goal_mode not in GOAL_MODES:
        raise C.SrlzError("%s: goal_mode must be 'running' or 'final', got %r" % (who, goal_mode))
    return goal, (s if goal.dim() == 2 else 0), GOAL_MODES[goal_mode]


def rollout_goal(states, plans, wf, bf, goal, reward=None, final=None, returns=None, trajectory=None, reward_logits=None, goal_dist=None,
                 gamma=1.0, goal_weight=1.0, goal_mode="running"):
    """One launch of srlz_rollout_goal: rollout's arguments, goal fp32 [S] (shared by every environment, read with a stride of 0) or
    [N,S], goal_weight > 0, goal_mode "running" / "final".  returns [N,K] is the score (allowed without a reward head), goal_dist
    [N,K,T] the squared distance of every step; both written only when given.  Returns `final`."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("rollout_goal: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    wf = _rollout_f32(wf, "forward_net.weight")
    if wf.dim() != 2 or wf.shape[0] != s or wf.shape[1] <= s:
        raise C.SrlzError("rollout_goal: forward_net.weight of shape %s does not take states of %d dimensions" % (tuple(wf.shape), s))
    a = wf.shape[1] - s
    bf = _rollout_f32(bf, "forward_net.bias", (s,))
    plans = rollout_plans(plans, a, states.device)
    if plans.device != states.device or plans.dim() not in (2, 3) or (plans.dim() == 3 and plans.shape[0] != n):
        raise C.SrlzError("rollout_goal: plans must be [N,K,T] with N = %d or [K,T] on the states' device, got %s" % (n, tuple(plans.shape)))
    k, t = plans.shape[-2], plans.shape[-1]
    stride = k * t if plans.dim() == 3 else 0
    goal, gstride, mode = _goal_args(goal, n, s, goal_mode, "rollout_goal")
    h, head = 0, (None,) * 6
    if reward is not None:
        h = reward[0].shape[0]
        shapes = ((h, 2 * s), (h,), (h, h), (h,), (2, h), (2,))
        head = tuple(_rollout_f32(p, "reward_net parameter", shape) for p, shape in zip(reward, shapes))
    if final is None:
        final = torch.empty((n, k, s), dtype=torch.float32, device=states.device)
    final = _rollout_f32(final, "final", (n, k, s))
    returns = _rollout_f32(returns, "returns", (n, k))
    trajectory = _rollout_f32(trajectory, "trajectory", (n, k, t, s))
    reward_logits = _rollout_f32(reward_logits, "reward_logits", (n, k, t, 2))
    goal_dist = _rollout_f32(goal_dist, "goal_dist", (n, k, t))
    C.rollout_goal(ptr(states), ptr(plans), stride, ptr(wf), ptr(bf), *[ptr(p) for p in head], ptr(final), ptr(returns), ptr(trajectory),
                   ptr(reward_logits), n, k, t, s, a, h, 2, float(gamma), ptr(goal), gstride, float(goal_weight), mode, ptr(goal_dist),
                   stream())
    return final


def plan_cem_goal(states, wf, bf, reward, goal, n_plans, horizon, iterations, elites, sharpness, best_plan, best_return, cum, workspace,
                  gamma=1.0, seed=0, init_weights=None, plans=None, returns=None, goal_weight=1.0, goal_mode="running"):
    """`iterations` launches of plan_cem_kernel<PlanGoalArgs>: plan_cem's arguments with the goal of rollout_goal; reward = (w1 .. b3) or None
    (the score is then the goal term alone).  best_return and returns are scores."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("plan_cem_goal: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    wf = _rollout_f32(wf, "forward_net.weight")
    if wf.dim() != 2 or wf.shape[0] != s or wf.shape[1] <= s:
        raise C.SrlzError("plan_cem_goal: forward_net.weight of shape %s does not take states of %d dimensions" % (tuple(wf.shape), s))
    a = wf.shape[1] - s
    bf = _rollout_f32(bf, "forward_net.bias", (s,))
    goal, gstride, mode = _goal_args(goal, n, s, goal_mode, "plan_cem_goal")
    h, head = 0, (None,) * 6
    if reward is not None:
        h = reward[0].shape[0]
        shapes = ((h, 2 * s), (h,), (h, h), (h,), (2, h), (2,))
        head = tuple(_rollout_f32(p, "reward_net parameter", shape) for p, shape in zip(reward, shapes))
    k, t, it = int(n_plans), int(horizon), int(iterations)
    stride = 0
    if init_weights is not None:
        if tuple(init_weights.shape) not in ((t, a), (n, t, a)):
            raise C.SrlzError("plan_cem_goal: init_weights must be [T,A] or [N,T,A], got %s" % (tuple(init_weights.shape),))
        stride = t * a if init_weights.dim() == 3 else 0
        init_weights = _plan_buf(init_weights, "init_weights", torch.int32, init_weights.shape)
    best_plan = _plan_buf(best_plan, "best_plan", torch.int32, (n, t))
    best_return = _plan_buf(best_return, "best_return", torch.float32, (n,))
    cum = _plan_buf(cum, "cum", torch.int32, (n, t, a))
    plans = _plan_buf(plans, "plans", torch.int32, (it, n, k, t))
    returns = _plan_buf(returns, "returns", torch.float32, (it, n, k))
    if not torch.is_tensor(workspace) or workspace.device.type != "cuda" or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise C.SrlzError("plan_cem_goal: workspace must be a contiguous uint8 device tensor")
    C.plan_cem_goal(ptr(states), ptr(wf), ptr(bf), *[ptr(p) for p in head], ptr(init_weights), stride, ptr(best_plan), ptr(best_return),
                    ptr(cum), ptr(plans), ptr(returns), ptr(workspace), workspace.numel(), n, k, t, s, a, h, 2, it, int(elites),
                    int(sharpness), float(gamma), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(goal), gstride, float(goal_weight), mode, stream())
    return best_plan


# ----------------------------------------------------------------------------------------------------------------
# Deployment tree search (csrc/beam.hip): exact enumeration or a beam over the action sequences of the dynamics above, one launch per
# level, all of them enqueued here back to back (include/srlz.h states the algorithm).  Thin, as plan_cem: the caller owns every
# buffer, nothing is allocated and no autograd node is made.
# ----------------------------------------------------------------------------------------------------------------
def beam_supported(s, a, h, n_rewards, has_reward, beam, horizon):
    return bool(C.beam_supported(int(s), int(a), int(h), int(n_rewards), int(bool(has_reward)), int(beam), int(horizon)))


def beam_workspace(n, beam, horizon, s, a):
    """Bytes of workspace of a beam_search call; 0 for a shape it refuses."""
    return int(C.beam_workspace(int(n), int(beam), int(horizon), int(s), int(a)))


def beam_leaves(beam, a, horizon):
    """L: the leaves a beam_search call keeps per environment; 0 outside the limits."""
    return int(C.beam_leaves(int(beam), int(a), int(horizon)))


def beam_search(states, wf, bf, reward, beam, horizon, best_plan, best_return, workspace, gamma=1.0, leaf_plans=None, leaf_returns=None,
                goal=None, goal_weight=1.0, goal_mode="running"):
    """`horizon` launches of beam_level_kernel.  states fp32 [N,S]; wf / bf / reward = (w1 .. b3) as rollout takes them (reward may be
    None with a goal); goal None, or as rollout_goal takes it.  Outputs best_plan int32 [N,T], best_return fp32 [N]; leaf_plans int32
    [N,L,T] and leaf_returns fp32 [N,L] keep the leaves (both or neither), L = beam_leaves(beam, A, horizon); workspace: a uint8
    device tensor of beam_workspace(...) bytes."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("beam_search: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    wf = _rollout_f32(wf, "forward_net.weight")
    if wf.dim() != 2 or wf.shape[0] != s or wf.shape[1] <= s:
        raise C.SrlzError("beam_search: forward_net.weight of shape %s does not take states of %d dimensions" % (tuple(wf.shape), s))
    a = wf.shape[1] - s
    bf = _rollout_f32(bf, "forward_net.bias", (s,))
    gstride, mode = 0, 0
    if goal is not None:
        goal, gstride, mode = _goal_args(goal, n, s, goal_mode, "beam_search")
    h, head = 0, (None,) * 6
    if reward is not None:
        h = reward[0].shape[0]
        shapes = ((h, 2 * s), (h,), (h, h), (h,), (2, h), (2,))
        head = tuple(_rollout_f32(p, "reward_net parameter", shape) for p, shape in zip(reward, shapes))
    w, t = int(beam), int(horizon)
    leaves = beam_leaves(w, a, t)
    best_plan = _plan_buf(best_plan, "best_plan", torch.int32, (n, t))
    best_return = _plan_buf(best_return, "best_return", torch.float32, (n,))
    leaf_plans = _plan_buf(leaf_plans, "leaf_plans", torch.int32, (n, leaves, t))
    leaf_returns = _plan_buf(leaf_returns, "leaf_returns", torch.float32, (n, leaves))
    if workspace is None or workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous():
        raise C.SrlzError("beam_search: workspace must be a contiguous uint8 device tensor")
    C.beam_search(ptr(states), ptr(wf), ptr(bf), *[ptr(p) for p in head], ptr(best_plan), ptr(best_return), ptr(leaf_plans),
                  ptr(leaf_returns), ptr(workspace), workspace.numel(), n, w, t, s, a, h, 2, float(gamma), ptr(goal), gstride,
                  float(goal_weight), mode, stream())
    return best_plan


# ----------------------------------------------------------------------------------------------------------------
# The k-step error of the dynamics on a recorded sequence (csrc/horizon.hip; include/srlz.h states the rule): two launches.  Thin,
# as rollout: the caller (srlz/deploy.py) owns every buffer and checks the contract starts[r] + len[r] <= N - 1, 0 <= len[r] <= T.
# ----------------------------------------------------------------------------------------------------------------
def horizon_supported(s, a, h=16, n_rewards=2, has_reward=True):
    return bool(C.horizon_supported(int(s), int(a), int(h), int(n_rewards), int(bool(has_reward))))


def _horizon_t(t, name, dtype, shape):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise C.SrlzError("horizon: %s must be a contiguous %s device tensor of shape %s" % (name, dtype, tuple(shape)))
    return t.detach()


def horizon_rows(states, actions, starts, lens, wf, bf, err, base, horizon, reward=None, reward_logits=None, trajectory=None):
    """One launch of srlz_horizon_rows.  states fp32 [N,S], actions int32 [N], starts / lens int32 [M]; err, base fp32 [M,T] with
    T = horizon; reward = (w1, b1, w2, b2, w3, b3) or None; reward_logits [M,T,2] and trajectory [M,T,S] written only when given."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("horizon: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    wf = _rollout_f32(wf, "forward_net.weight")
    if wf.dim() != 2 or wf.shape[0] != s or wf.shape[1] <= s:
        raise C.SrlzError("horizon: forward_net.weight of shape %s does not take states of %d dimensions" % (tuple(wf.shape), s))
    a = wf.shape[1] - s
    bf = _rollout_f32(bf, "forward_net.bias", (s,))
    t = int(horizon)
    actions = _horizon_t(actions, "actions", torch.int32, (n,))
    if starts is None or starts.dim() != 1:
        raise C.SrlzError("horizon: starts [M] expected")
    m = starts.shape[0]
    starts = _horizon_t(starts, "starts", torch.int32, (m,))
    lens = _horizon_t(lens, "lens", torch.int32, (m,))
    h, head = 0, (None,) * 6
    if reward is not None:
        h = reward[0].shape[0]
        shapes = ((h, 2 * s), (h,), (h, h), (h,), (2, h), (2,))
        head = tuple(_rollout_f32(p, "reward_net parameter", shape) for p, shape in zip(reward, shapes))
    err = _rollout_f32(err, "err", (m, t))
    base = _rollout_f32(base, "base", (m, t))
    reward_logits = _rollout_f32(reward_logits, "reward_logits", (m, t, 2))
    trajectory = _rollout_f32(trajectory, "trajectory", (m, t, s))
    C.horizon_rows(ptr(states), ptr(actions), ptr(starts), ptr(lens), ptr(wf), ptr(bf), *[ptr(p) for p in head], ptr(err), ptr(base),
                   ptr(reward_logits), ptr(trajectory), n, m, t, s, a, h, 2, stream())
    return err, base


def horizon_sums(err, base, starts, lens, count, sum_err, sum_base, reward_logits=None, labels=None, hits=None):
    """One launch of srlz_horizon_sums: err, base fp32 [M,T] -> count int64 [T], sum_err / sum_base fp64 [T]; with reward_logits
    [M,T,2], labels int32 [N] and hits int64 [T] (all three or none) the per-horizon hit counts of the reward head."""
    err = _rollout_f32(err, "err")
    if err.dim() != 2:
        raise C.SrlzError("horizon: err [M,T] expected, got %s" % (tuple(err.shape),))
    m, t = err.shape
    base = _rollout_f32(base, "base", (m, t))
    starts = _horizon_t(starts, "starts", torch.int32, (m,))
    lens = _horizon_t(lens, "lens", torch.int32, (m,))
    count = _horizon_t(count, "count", torch.int64, (t,))
    sum_err = _horizon_t(sum_err, "sum_err", torch.float64, (t,))
    sum_base = _horizon_t(sum_base, "sum_base", torch.float64, (t,))
    reward_logits = _rollout_f32(reward_logits, "reward_logits", (m, t, 2))
    if labels is not None and (not torch.is_tensor(labels) or labels.device.type != "cuda" or labels.dtype != torch.int32
                               or labels.dim() != 1 or not labels.is_contiguous()):
        raise C.SrlzError("horizon: labels must be a contiguous int32 device tensor [N]")
    hits = _horizon_t(hits, "hits", torch.int64, (t,))
    C.horizon_sums(ptr(err), ptr(base), ptr(reward_logits), ptr(labels), ptr(starts), ptr(lens), m, t, ptr(count), ptr(sum_err),
                   ptr(sum_base), ptr(hits), stream())
    return count, sum_err, sum_base, hits


# ----------------------------------------------------------------------------------------------------------------
# The forward head's normal equations on a recorded sequence (csrc/dynfit.hip; include/srlz.h states every sum's order): two
# launches.  Thin, as horizon_rows: the caller (srlz/dynfit.py) owns the data and has checked the actions on the host; the table of
# transitions is checked by the launcher itself, on its host copy.
# ----------------------------------------------------------------------------------------------------------------
def dynfit_supported(s, a):
    return bool(C.dynfit_supported(int(s), int(a)))


def dynfit_chunk_rows(m, s, a):
    return int(C.dynfit_chunk_rows(int(m), int(s), int(a)))


def dynfit_workspace(m, s, a):
    return int(C.dynfit_workspace(int(m), int(s), int(a)))


def dynfit_gram(states, actions, starts, n_actions, gram=None, cross=None, workspace=None):
    """srlz_dynfit_gram: states fp32 [N,S] and actions int32 [N] on the device, starts int32 [M] on the HOST (checked there against
    [0, N - 2], then uploaded) -> (G fp64 [P,P], C fp64 [P,S]) on the device, P = S + n_actions + 1.  gram / cross / workspace: the
    caller's buffers (a uint8 workspace of at least dynfit_workspace(M, S, A) bytes), made here when None."""
    states = _rollout_f32(states, "states")
    if states.dim() != 2:
        raise C.SrlzError("dynfit: states [N,S] expected, got %s" % (tuple(states.shape),))
    n, s = states.shape
    a = int(n_actions)
    if not dynfit_supported(s, a):
        raise C.SrlzError("dynfit: state_dim %d with %d actions is outside srlz_dynfit_supported" % (s, a))
    actions = _horizon_t(actions, "actions", torch.int32, (n,))
    if not torch.is_tensor(starts) or starts.device.type != "cpu" or starts.dtype != torch.int32 or starts.dim() != 1 \
            or not starts.is_contiguous() or starts.shape[0] < 1:
        raise C.SrlzError("dynfit: starts must be a non-empty contiguous int32 host tensor [M] (it is checked on the host, then uploaded)")
    m, p = int(starts.shape[0]), s + a + 1
    dev = states.device
    gram = torch.empty((p, p), dtype=torch.float64, device=dev) if gram is None else _horizon_t(gram, "gram", torch.float64, (p, p))
    cross = torch.empty((p, s), dtype=torch.float64, device=dev) if cross is None else _horizon_t(cross, "cross", torch.float64, (p, s))
    nbytes = dynfit_workspace(m, s, a)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous():
        raise C.SrlzError("dynfit: workspace must be a contiguous uint8 device tensor")
    d_starts = starts.to(dev)
    C.dynfit_gram(ptr(states), ptr(actions), ptr(d_starts), ctypes.c_void_p(starts.data_ptr()), n, m, s, a, ptr(gram), ptr(cross),
                  ptr(workspace), workspace.numel(), stream())
    return gram, cross


# ----------------------------------------------------------------------------------------------------------------
# The reward head on a recorded sequence (csrc/headfit.hip; include/srlz.h states the layout, every sum's order and the limits):
# an epoch of Adam steps in one launch, a validation phase in one more.  The (states, labels) pair is reward_probe_data's; the
# argument checks and error types are those of reward_probe_fit / reward_probe_eval.
# ----------------------------------------------------------------------------------------------------------------
def headfit_supported(s, h):
    return bool(C.headfit_supported(int(s), int(h)))


def headfit_n_params(s, h):
    """Linear(2S, H), Linear(H, H), Linear(H, 2) with their biases, flat in state_dict order (0 for S < 1 or H < 1)."""
    return int(C.headfit_n_params(int(s), int(h)))


def headfit_chunk_rows(s, h):
    """Rows of a minibatch that srlz_headfit_fit processes at a time (a function of S and H alone; 0 for a refused shape)."""
    return int(C.headfit_chunk_rows(int(s), int(h)))


class HeadfitTable(object):
    """A minibatch table int32 [n, B] on the host and its device copy (headfit_table): built once, passed to many launches."""

    def __init__(self, host, device):
        self.host, self.device = host, device


def headfit_table(data, idx):
    """int32 [n, B] host table -> HeadfitTable, uploaded once (the launchers check the host copy at every call)."""
    if isinstance(idx, HeadfitTable):
        if not isinstance(data, RewardProbeData) or idx.device.device != data.states.device:
            raise ValueError("headfit: the table was uploaded for other data")
        return idx
    return HeadfitTable(*_reward_probe_table(data, idx, who="headfit"))


def _headfit_shape(data, hidden):
    if not isinstance(data, RewardProbeData):
        raise ValueError("headfit: data must come from reward_probe_data()")
    h = int(hidden)
    if not headfit_supported(data.s, h):
        raise ValueError("headfit: state_dim %d with %d hidden units is outside srlz_headfit_supported" % (data.s, h))
    return h


def headfit_fit(data, idx, hidden, params, m, v, t0, lr, running_loss, counts, step_loss=None, last_grad=None, betas=(0.9, 0.999),
                eps=1e-8):
    """idx.shape[0] consecutive Adam steps of the reward head (Linear(2S,H)-ReLU-Linear(H,H)-ReLU-Linear(H,2), cross-entropy) in
    ONE launch of srlz_headfit_fit: minibatch s is the rows [states[i] ; states[i + 1]] for i in idx[s], labelled labels[i].  No
    autograd: the kernel owns the backward.  data: reward_probe_data(states, labels); idx: an int32 [n, B] host table or a
    headfit_table; params / m / v: float32 [headfit_n_params(S, H)] on the device in state_dict order, updated in place; t0: the
    Adam steps already taken; running_loss float64 [1] and counts int64 [5] are added to (reward_probe_stats); step_loss: float64
    [>= steps] for the mean loss of every step, or None; last_grad: float32 [n_params] for the last step's gradient, or None."""
    h = _headfit_shape(data, hidden)
    tb = headfit_table(data, idx)
    n_steps, b = int(tb.host.shape[0]), int(tb.host.shape[1])
    n_par = headfit_n_params(data.s, h)
    for t, name in ((params, "params"), (m, "m"), (v, "v")):
        _reward_probe_buffer(t, name, torch.float32, n_par, data, exact=True, who="headfit")
    _reward_probe_buffer(running_loss, "running_loss", torch.float64, 1, data, who="headfit")
    _reward_probe_buffer(counts, "counts", torch.int64, 5, data, who="headfit")
    if step_loss is not None:
        _reward_probe_buffer(step_loss, "step_loss", torch.float64, n_steps, data, who="headfit")
    if last_grad is not None:
        _reward_probe_buffer(last_grad, "last_grad", torch.float32, n_par, data, exact=True, who="headfit")
    C.headfit_fit(ptr(data.states), ptr(data.labels), data.n, data.s, h, ptr(tb.device), ctypes.c_void_p(tb.host.data_ptr()), n_steps, b,
                  ptr(params), ptr(m), ptr(v), int(t0), float(lr), float(betas[0]), float(betas[1]), float(eps), ptr(running_loss),
                  ptr(counts), ptr(step_loss), ptr(last_grad), stream())


def headfit_eval(data, idx, hidden, params, running_loss, counts, workspace=None):
    """The forward, loss (float64 per row) and counts of idx.shape[0] minibatches in ONE launch of srlz_headfit_eval; params are only
    read, running_loss and counts are added to.  workspace: a contiguous uint8 device tensor of at least
    srlz_headfit_eval_workspace(n, B) bytes, made here when None."""
    h = _headfit_shape(data, hidden)
    tb = headfit_table(data, idx)
    n_batches, b = int(tb.host.shape[0]), int(tb.host.shape[1])
    _reward_probe_buffer(params, "params", torch.float32, headfit_n_params(data.s, h), data, exact=True, who="headfit")
    _reward_probe_buffer(running_loss, "running_loss", torch.float64, 1, data, who="headfit")
    _reward_probe_buffer(counts, "counts", torch.int64, 5, data, who="headfit")
    device = data.states.device
    ticket = _REWARD_PROBE_TICKET.get(device.index)
    if ticket is None:
        ticket = _REWARD_PROBE_TICKET[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    nbytes = int(C.headfit_eval_workspace(n_batches, b))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
    else:
        _reward_probe_buffer(workspace, "workspace", torch.uint8, nbytes, data, who="headfit")
    C.headfit_eval(ptr(data.states), ptr(data.labels), data.n, data.s, h, ptr(tb.device), ctypes.c_void_p(tb.host.data_ptr()), n_batches,
                   b, ptr(params), ptr(running_loss), ptr(counts), ptr(workspace), workspace.numel(), ptr(ticket), stream())


# ----------------------------------------------------------------------------------------------------------------
# The inverse head on a recorded sequence (csrc/invfit.hip; include/srlz.h states the layout, every sum's order and the limits):
# an epoch of Adam steps in one launch, a validation phase in one more.  The data is a RewardProbeData of (states, actions) — the
# labels are the actions and are NOT range-checked here: the kernels count a label outside [0, A) in `bad` and index nothing by it
# (srlz/invfit.py checks host actions before it uploads them).  Tables are headfit_table's; the argument checks and error types are
# those of the headfit wrappers.
# ----------------------------------------------------------------------------------------------------------------
INVFIT_COUNTS = ("rows", "correct", "bad")  # the first three int64 counters; support[A] and hits[A] follow


def invfit_supported(s, a):
    return bool(C.invfit_supported(int(s), int(a)))


def invfit_n_params(s, a):
    """Linear(2S, A) with its bias, flat in state_dict order (0 for S < 1 or A < 2)."""
    return int(C.invfit_n_params(int(s), int(a)))


def invfit_chunk_rows(s, a):
    """Rows of a minibatch that srlz_invfit_fit processes at a time (a function of S and A alone; 0 for a refused shape)."""
    return int(C.invfit_chunk_rows(int(s), int(a)))


def invfit_n_counts(a):
    """The length of the counters: rows, correct, bad, support[A], hits[A]."""
    return len(INVFIT_COUNTS) + 2 * int(a)


def _invfit_shape(data, n_actions):
    if not isinstance(data, RewardProbeData):
        raise ValueError("invfit: data must be a RewardProbeData of (states, actions)")
    a = int(n_actions)
    if not invfit_supported(data.s, a):
        raise ValueError("invfit: state_dim %d with %d actions is outside srlz_invfit_supported" % (data.s, a))
    return a


def invfit_fit(data, idx, n_actions, params, m, v, t0, lr, running_loss, counts, step_loss=None, last_grad=None, betas=(0.9, 0.999),
               eps=1e-8):
    """idx.shape[0] consecutive Adam steps of the inverse head (Linear(2S, A), cross-entropy) in ONE launch of srlz_invfit_fit:
    minibatch s is the rows [states[i] ; states[i + 1]] for i in idx[s], labelled labels[i].  No autograd: the kernel owns the
    backward.  data: RewardProbeData(states fp32 [N,S], actions int32 [N]) on the device; idx: an int32 [n, B] host table or a
    headfit_table; params / m / v: float32 [invfit_n_params(S, A)] on the device in state_dict order, updated in place; t0: the Adam
    steps already taken; running_loss float64 [1] and counts int64 [invfit_n_counts(A)] are added to; step_loss: float64 [>= steps]
    for the mean loss of every step, or None; last_grad: float32 [n_params] for the last step's gradient, or None."""
    a = _invfit_shape(data, n_actions)
    tb = headfit_table(data, idx)
    n_steps, b = int(tb.host.shape[0]), int(tb.host.shape[1])
    n_par = invfit_n_params(data.s, a)
    for t, name in ((params, "params"), (m, "m"), (v, "v")):
        _reward_probe_buffer(t, name, torch.float32, n_par, data, exact=True, who="invfit")
    _reward_probe_buffer(running_loss, "running_loss", torch.float64, 1, data, who="invfit")
    _reward_probe_buffer(counts, "counts", torch.int64, invfit_n_counts(a), data, exact=True, who="invfit")
    if step_loss is not None:
        _reward_probe_buffer(step_loss, "step_loss", torch.float64, n_steps, data, who="invfit")
    if last_grad is not None:
        _reward_probe_buffer(last_grad, "last_grad", torch.float32, n_par, data, exact=True, who="invfit")
    C.invfit_fit(ptr(data.states), ptr(data.labels), data.n, data.s, a, ptr(tb.device), ctypes.c_void_p(tb.host.data_ptr()), n_steps, b,
                 ptr(params), ptr(m), ptr(v), int(t0), float(lr), float(betas[0]), float(betas[1]), float(eps), ptr(running_loss),
                 ptr(counts), ptr(step_loss), ptr(last_grad), stream())


def invfit_eval(data, idx, n_actions, params, running_loss, counts, workspace=None):
    """The forward, loss (float64 per row) and counts of idx.shape[0] minibatches in ONE launch of srlz_invfit_eval; params are only
    read, running_loss and counts (int64 [invfit_n_counts(A)]) are added to.  workspace: a contiguous uint8 device tensor of at least
    srlz_invfit_eval_workspace(n, B) bytes, made here when None."""
    a = _invfit_shape(data, n_actions)
    tb = headfit_table(data, idx)
    n_batches, b = int(tb.host.shape[0]), int(tb.host.shape[1])
    _reward_probe_buffer(params, "params", torch.float32, invfit_n_params(data.s, a), data, exact=True, who="invfit")
    _reward_probe_buffer(running_loss, "running_loss", torch.float64, 1, data, who="invfit")
    _reward_probe_buffer(counts, "counts", torch.int64, invfit_n_counts(a), data, exact=True, who="invfit")
    device = data.states.device
    ticket = _REWARD_PROBE_TICKET.get(device.index)
    if ticket is None:
        ticket = _REWARD_PROBE_TICKET[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    nbytes = int(C.invfit_eval_workspace(n_batches, b))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
    else:
        _reward_probe_buffer(workspace, "workspace", torch.uint8, nbytes, data, who="invfit")
    C.invfit_eval(ptr(data.states), ptr(data.labels), data.n, data.s, a, ptr(tb.device), ctypes.c_void_p(tb.host.data_ptr()), n_batches,
                  b, ptr(params), ptr(running_loss), ptr(counts), ptr(workspace), workspace.numel(), ptr(ticket), stream())


# ----------------------------------------------------------------------------------------------------------------
# The robotic priors (csrc/robotic.hip): roboticPriorsLoss, reference losses/losses.py:62-99
# ----------------------------------------------------------------------------------------------------------------
ROBOTIC_TERMS = ("temp_coherence_loss", "causality_loss", "proportionality_loss", "repeatability_loss")  # losses.py:92


def robotic_pairs(pairs, batch, name="pairs"):
    """A pair list as the kernels read it: int32 [n, 2], checked on the host.  Any order, duplicates, i > j and i == j are allowed.
    ValueError: an empty list (the reference's mean of nothing is NaN), another shape, non-integers, an index outside [0, batch)."""
    a = np.asarray(pairs)
    if a.size == 0:
        raise ValueError("robotic priors: the %s list is empty: the mean over no pair is NaN" % name)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("robotic priors: the %s must be an [n, 2] list of positions, got shape %s" % (name, a.shape))
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("robotic priors: the %s must be integers (got %s)" % (name, a.dtype))
    if a.shape[0] >= 2 ** 30:
        raise ValueError("robotic priors: fewer than 2^30 %s are supported" % name)
    lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= int(batch):
        raise ValueError("robotic priors: the %s must lie in [0, %d), got %d .. %d" % (name, int(batch), lo, hi))
    return np.ascontiguousarray(a, dtype=np.int32)


def robotic_incidence(pairs, batch):
    """The incidence table srlz_robotic_bwd walks (include/srlz.h): int32 [batch + 1 + 2n] — offsets [batch + 1], then the partners.
    Pair p = [i, j] gives row i the partner j and row j the partner i (i == j: twice itself); a row's partners stand in pair order,
    the i end of a pair before its j end.  Pure host function."""
    p = robotic_pairs(pairs, batch)
    rows, partners = p.reshape(-1), p[:, ::-1].reshape(-1)  # (i0, j0, i1, j1, ..) and (j0, i0, j1, i1, ..)
    order = np.argsort(rows, kind="stable")
    offsets = np.zeros(int(batch) + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=int(batch)), out=offsets[1:])
    return np.concatenate((offsets, partners[order])).astype(np.int32)


class RoboticTable(object):
    """The pair lists of ONE minibatch on the device, built and uploaded once (robotic_table): dis / same int32 [n, 2], their
    incidence tables, the counts and the batch size they were checked for."""
    __slots__ = ("batch", "n_dis", "n_same", "dis", "same", "dis_inc", "same_inc", "buffer")


def robotic_table(dissimilar_pairs, same_actions_pairs, batch, device):
    """Check both pair lists of a minibatch of `batch` rows on the host (robotic_pairs' ValueErrors), build both incidence tables
    and upload the four as ONE int32 buffer -> RoboticTable."""
    batch = int(batch)
    dis, same = robotic_pairs(dissimilar_pairs, batch, "dissimilar pairs"), robotic_pairs(same_actions_pairs, batch, "same-action pairs")
    parts = (dis.reshape(-1), same.reshape(-1), robotic_incidence(dis, batch), robotic_incidence(same, batch))
    host = torch.from_numpy(np.concatenate(parts))
    if torch.device(device).type == "cuda":
        host = host.pin_memory()
    buf = host.to(device, non_blocking=True)
    t = RoboticTable()
    t.batch, t.n_dis, t.n_same, t.buffer = batch, int(dis.shape[0]), int(same.shape[0]), buf
    off = 0
    for name, part in zip(("dis", "same", "dis_inc", "same_inc"), parts):
        setattr(t, name, buf[off:off + part.size])
        off += part.size
    return t


class RoboticPriorsFn(Function):
    """The four robotic priors of one minibatch -> (temporal coherence, causality, proportionality, repeatability), four 0-dim fp32
    tensors (views of one [4] tensor) — roboticPriorsLoss, reference losses/losses.py:62-99.  `table`: a RoboticTable for this batch
    size.  One launch forward (fp64 sums in one order, rounded once to fp32; robotic_priors_terms gives the fp64 values), one launch
    backward that writes both gradients whole, no atomics: two calls give identical bits."""

    @staticmethod
    def forward(ctx, states, next_states, table):
        terms32, _terms64, norms = _robotic_forward(states, next_states, table)
        ctx.save_for_backward(_check(states, "states"), _check(next_states, "next_states"), norms)
        ctx.table = table
        return tuple(terms32.unbind(0))

    @staticmethod
    def backward(ctx, g_tc, g_ca, g_pr, g_re):
        states, next_states, norms = ctx.saved_tensors
        t = ctx.table
        b, s = states.shape
        gs = [_check(g, "loss grad") for g in (g_tc, g_ca, g_pr, g_re)]
        ds, dns = torch.empty_like(states), torch.empty_like(next_states)
        C.robotic_bwd(ptr(states), ptr(next_states), ptr(norms), b, s, ptr(t.same_inc), t.n_same, ptr(t.dis_inc), t.n_dis,
                      ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(gs[3]), ptr(ds), ptr(dns), stream())
        return ds, dns, None


def _robotic_forward(states, next_states, table):
    states, next_states = _check(states, "states"), _check(next_states, "next_states")
    if states.dim() != 2 or states.shape != next_states.shape:
        raise ValueError("robotic priors: states and next_states must both be [B, S], got %s and %s"
                         % (tuple(states.shape), tuple(next_states.shape)))
    if not isinstance(table, RoboticTable):
        raise ValueError("robotic priors: the pair lists must be a RoboticTable (ops.robotic_table)")
    b, s = states.shape
    if table.batch != b or table.buffer.device != states.device:
        raise ValueError("robotic priors: the table was built for %d rows on %s, the states have %d rows on %s"
                         % (table.batch, table.buffer.device, b, states.device))
    terms64 = torch.empty(4, dtype=torch.float64, device=states.device)
    terms32 = torch.empty(4, dtype=torch.float32, device=states.device)
    norms = torch.empty(b, dtype=torch.float32, device=states.device)
    C.robotic_fwd(ptr(states), ptr(next_states), b, s, ptr(table.dis), table.n_dis, ptr(table.same), table.n_same, ptr(norms),
                  ptr(terms64), ptr(terms32), stream())
    return terms32, terms64, norms


def robotic_priors_terms(states, next_states, table):
    """The four terms as the forward launch sums them: a float64 [4] device tensor, no autograd."""
    return _robotic_forward(states.detach(), next_states.detach(), table)[1]


def robotic_supported(d, s, b):
    """srlz_robotic_supported: D features, state dimension S and minibatches of B fit the LDS budget of srlz_robotic_fit."""
    return bool(C.robotic_supported(int(d), int(s), int(b)))


def robotic_n_params(d, s):
    """Linear(D, S) with its bias, flat in state_dict order (0 for D < 1 or S < 1)."""
    return int(C.robotic_n_params(int(d), int(s)))


class _HostDevice(object):
    """An int32 table as the fit's entry points take it: the host copy they check and the device copy the kernels read."""
    __slots__ = ("host", "device")

    def __init__(self, host, device):
        self.host = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32))
        pinned = self.host.pin_memory() if torch.device(device).type == "cuda" else self.host
        self.device = pinned.to(device, non_blocking=True)

    def host_ptr(self):
        return ctypes.c_void_p(self.host.data_ptr())


class RoboticFitTables(object):
    """Everything srlz_robotic_fit / _eval read besides the features, built and uploaded ONCE per fit (robotic_fit_tables): idx
    [n, B] (the frames of every minibatch), tables (all pair lists and incidence tables), dir [n, 6]."""
    __slots__ = ("n", "batch", "idx", "tables", "dir")


def robotic_fit_tables(minibatches, dissimilar_pairs, same_actions_pairs, device):
    """minibatches: n arrays of B frame indices (as losses.utils.priors_pairs leaves them); the two pair lists per minibatch.  The
    pair lists are checked here (robotic_pairs' ValueErrors); the frame indices by the entry points, against the features."""
    mb = np.asarray(minibatches)
    if mb.ndim != 2 or mb.shape[0] < 1 or mb.shape[1] < 1 or not np.issubdtype(mb.dtype, np.integer):
        raise ValueError("robotic fit: the minibatches must be an integer [n, B] table, got %s %s" % (mb.dtype, mb.shape))
    n, b = int(mb.shape[0]), int(mb.shape[1])
    if len(dissimilar_pairs) != n or len(same_actions_pairs) != n:
        raise ValueError("robotic fit: %d minibatches, but %d and %d pair lists" % (n, len(dissimilar_pairs), len(same_actions_pairs)))
    if mb.min() < 0 or mb.max() >= 2 ** 31 - 1:
        raise ValueError("robotic fit: frame indices must lie in [0, 2^31 - 1)")
    parts, entries, off = [], np.zeros((n, 6), np.int64), 0
    for k in range(n):
        dis = robotic_pairs(dissimilar_pairs[k], b, "dissimilar pairs of minibatch %d" % k)
        same = robotic_pairs(same_actions_pairs[k], b, "same-action pairs of minibatch %d" % k)
        four = (dis.reshape(-1), same.reshape(-1), robotic_incidence(dis, b), robotic_incidence(same, b))
        offs = off + np.concatenate(([0], np.cumsum([p.size for p in four])))
        entries[k] = (offs[0], dis.shape[0], offs[1], same.shape[0], offs[2], offs[3])
        off = int(offs[4])
        parts.extend(four)
    if off >= 2 ** 31:
        raise ValueError("robotic fit: the pair tables hold %d entries, 2^31 or more" % off)
    t = RoboticFitTables()
    t.n, t.batch = n, b
    t.idx, t.tables, t.dir = _HostDevice(mb, device), _HostDevice(np.concatenate(parts), device), _HostDevice(entries, device)
    return t


def _robotic_fit_args(features, tabs, order, params, who):
    if not isinstance(tabs, RoboticFitTables):
        raise ValueError("%s: tabs must be a RoboticFitTables (ops.robotic_fit_tables)" % who)
    features = _check(features, "features")
    if features.dim() != 2:
        raise ValueError("%s: features must be [N, D], got %s" % (who, tuple(features.shape)))
    n, d = int(features.shape[0]), int(features.shape[1])
    n_par = int(params.numel())
    if n_par % (d + 1):
        raise ValueError("%s: %d parameters are no Linear(%d, S) with its bias" % (who, n_par, d))
    s = n_par // (d + 1)
    if not robotic_supported(d, s, tabs.batch):
        raise ValueError("%s: %d features, state_dim %d and minibatches of %d are outside srlz_robotic_supported" % (who, d, s, tabs.batch))
    if not isinstance(order, _HostDevice):
        order = _HostDevice(np.asarray(order).reshape(-1), features.device)
    for t in (tabs.idx, tabs.tables, tabs.dir, order):
        if t.device.device != features.device:
            raise ValueError("%s: the tables live on %s, the features on %s" % (who, t.device.device, features.device))
    return features, n, d, s, order


def _robotic_buffer(t, name, dtype, numel, device, who, exact=False):
    if not (torch.is_tensor(t) and t.dtype == dtype and t.device == device and t.is_contiguous()
            and (t.numel() == numel if exact else t.numel() >= numel)):
        raise ValueError("%s: %s must be a contiguous %s device tensor of %s%d elements on %s"
                         % (who, name, dtype, "" if exact else "at least ", numel, device))


def robotic_order(ids, device):
    """A list of minibatch ids (an epoch's order, or the validation minibatches), uploaded without blocking."""
    return _HostDevice(np.asarray(ids).reshape(-1), device)


def robotic_fit(features, tabs, order, params, m, v, t0, lr, running, step_terms=None, last_grad=None, betas=(0.9, 0.999), eps=1e-8):
    """len(order) consecutive Adam steps of the linear state map under the four robotic priors in ONE launch of srlz_robotic_fit:
    step s trains on minibatch order[s] of tabs.  No autograd: the kernel owns the backward.  features fp32 [N, D] on the device;
    params / m / v: float32 [S * D + S] in state_dict order, updated in place; t0: the Adam steps already taken; running float64
    [4] is added to (the four terms of every step); step_terms: float64 [>= 4 * steps] or None; last_grad: float32 [n_params] or
    None."""
    features, n, d, s, order = _robotic_fit_args(features, tabs, order, params, "robotic_fit")
    dev, n_par, steps = features.device, int(params.numel()), int(order.host.numel())
    for t, name in ((params, "params"), (m, "m"), (v, "v")):
        _robotic_buffer(t, name, torch.float32, n_par, dev, "robotic_fit", exact=True)
    _robotic_buffer(running, "running", torch.float64, 4, dev, "robotic_fit", exact=True)
    if step_terms is not None:
        _robotic_buffer(step_terms, "step_terms", torch.float64, 4 * steps, dev, "robotic_fit")
    if last_grad is not None:
        _robotic_buffer(last_grad, "last_grad", torch.float32, n_par, dev, "robotic_fit", exact=True)
    C.robotic_fit(ptr(features), n, d, s, ptr(tabs.idx.device), tabs.idx.host_ptr(), tabs.n, tabs.batch, ptr(tabs.tables.device),
                  int(tabs.tables.host.numel()), ptr(tabs.dir.device), tabs.dir.host_ptr(), ptr(order.device), order.host_ptr(), steps,
                  ptr(params), ptr(m), ptr(v), int(t0), float(lr), float(betas[0]), float(betas[1]), float(eps), ptr(running),
                  ptr(step_terms), ptr(last_grad), stream())


_ROBOTIC_TICKET = {}


def robotic_eval(features, tabs, order, params, running, workspace=None):
    """The four terms of the listed minibatches in ONE launch of srlz_robotic_eval, added to running float64 [4] in list order;
    params are only read.  workspace: a contiguous uint8 device tensor of at least srlz_robotic_eval_workspace(len(order)) bytes,
    made here when None."""
    features, n, d, s, order = _robotic_fit_args(features, tabs, order, params, "robotic_eval")
    dev, count = features.device, int(order.host.numel())
    _robotic_buffer(params, "params", torch.float32, int(params.numel()), dev, "robotic_eval", exact=True)
    _robotic_buffer(running, "running", torch.float64, 4, dev, "robotic_eval", exact=True)
    ticket = _ROBOTIC_TICKET.get(dev.index)
    if ticket is None:
        ticket = _ROBOTIC_TICKET[dev.index] = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(C.robotic_eval_workspace(count))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    else:
        _robotic_buffer(workspace, "workspace", torch.uint8, nbytes, dev, "robotic_eval")
    C.robotic_eval(ptr(features), n, d, s, ptr(tabs.idx.device), tabs.idx.host_ptr(), tabs.n, tabs.batch, ptr(tabs.tables.device),
                   int(tabs.tables.host.numel()), ptr(tabs.dir.device), tabs.dir.host_ptr(), ptr(order.device), order.host_ptr(), count,
                   ptr(params), ptr(running), ptr(workspace), workspace.numel(), ptr(ticket), stream())
