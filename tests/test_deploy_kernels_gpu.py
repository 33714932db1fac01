"""csrc/infer.hip on the GPU: each block kind (conv + eval BatchNorm + ReLU + MaxPool 3x3 s2 in ONE launch) against an fp64
restatement in torch-CPU double (conv2d, affine, relu, max_pool2d: deploy_util.ref_block).

Shapes: the smallest at which the kernel can go wrong — odd and rectangular maps, a truncated last window under pool pad 1, pooled maps
of 1 x 2, and per kind one case whose pooled map spans MORE THAN ONE WORKGROUP TILE in both directions, sized from the kernel's own tile
edge T = srlz_infer_tile() (a workgroup owns T x T pooled outputs): pooled (T + 1) x (T + 2).
Inputs: gamma with negative entries, channels whose pre-activation is negative everywhere, running variances over two decades, a
sentinel tail behind every output.
Bound: the project's bound for outputs, 1e-4 of the output's scale; the measured maximum is printed (DESIGN.md 3.13 quotes it)."""
import ctypes

import numpy as np
import pytest
import torch

import deploy_util as du

pytestmark = pytest.mark.gpu

BOUND = 1e-4
SENTINEL = 1234.5
TAIL = 64
DEAD = (5, 37)  # channels whose pre-activation is negative everywhere (beta far below anything the convolution reaches)


def _bn(layer):
    g, b, m, v = du.bn_formula(layer)
    b = b.clone()
    for c in DEAD:
        b[c] = -1.0e4
    return g, b, m, v


def _weights(kind, c_in, seed):
    k = du.GEO[kind][0]
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((64, c_in, k, k), generator=gen) * (1.0 / np.sqrt(c_in * k * k))


class Block(object):
    """One block kind on the device: packed weights and the BatchNorm record, made once."""

    def __init__(self, kind, c_in, seed=0):
        from srlz import _cabi as C, ops
        self.C, self.ops, self.kind, self.c_in = C, ops, kind, c_in
        self.dev = torch.device("cuda", 0)
        self.w = _weights(kind, c_in, seed + 10 * kind + c_in)
        self.wpack = ops.infer_pack(self.w.to(self.dev), kind)
        g, b, m, v = [t.to(self.dev) for t in _bn(kind)]
        self.bnp = torch.empty(256, dtype=torch.float32, device=self.dev)
        C.bn_eval_params(C.ptr(g), C.ptr(b), C.ptr(m), C.ptr(v), du.BN_EPS, C.ptr(self.bnp), C.stream())
        rec = self.bnp.cpu()
        self.scale, self.shift = rec[128:192].clone(), rec[192:256].clone()
        self.lut = ops.norm_lut(self.dev) if kind == 0 else None

    def run(self, x_dev, n, hi, wi, strides=None, pool_pad=None, out_nchw=False):
        """-> (pooled as [n,64,hp,wp] on the CPU, the sentinel tail)"""
        ops = self.ops
        pool_pad = du.POOL_PAD[self.kind] if pool_pad is None else pool_pad
        d = ops.infer_desc(self.kind, n, self.c_in, hi, wi, strides, pool_pad, out_nchw)
        assert ops.infer_supported(d)
        _, _, hp, wp = ops.infer_out_dims(d)
        numel = n * 64 * hp * wp
        out = torch.full((numel + TAIL,), SENTINEL, dtype=torch.float32, device=self.dev)
        ops.infer_block(x_dev, self.wpack, self.bnp, out, d, lut=self.lut)
        torch.cuda.synchronize()
        host = out.cpu()
        body = host[:numel].view(n, 64, hp, wp) if out_nchw else host[:numel].view(n, hp, wp, 64).permute(0, 3, 1, 2)
        return body.contiguous(), host[numel:]


@pytest.fixture(scope="module")
def blocks():
    assert torch.cuda.is_available()
    return {(0, 3): Block(0, 3), (0, 6): Block(0, 6), (1, 64): Block(1, 64), (2, 64): Block(2, 64)}


def _check(tag, got, tail, ref):
    assert torch.equal(tail, torch.full_like(tail, SENTINEL)), "%s: wrote behind its output" % tag
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = (got.double() - ref).abs().max().item() / ref.abs().max().item()
    print("%s: max |err| / max |ref| = %.3e (pooled %s)" % (tag, err, tuple(ref.shape)))
    assert err <= BOUND, (tag, err)
    for c in DEAD:
        assert float(got[:, c].abs().max()) == 0.0, (tag, c)
    assert float(got.min()) >= 0.0


def _in_sizes():
    from srlz import _cabi as C
    t = C.infer_tile()
    # pooled (t + 1) x (t + 2) under pool pad 1: hc = 2 hp - 1, and the 7x7 stride-2 convolution gives hc from hi = 2 hc - 1
    return 2 * (2 * (t + 1) - 1) - 1, 2 * (2 * (t + 2) - 1) - 1


@pytest.mark.parametrize("c,n,h,w", [(3, 1, 12, 20), (3, 1, 20, 12), (6, 3, 17, 23), (3, 2, None, None)])
def test_block_in_against_fp64_both_byte_layouts(blocks, c, n, h, w):
    """Frames of h x w (H x W); the convolution sees the reference's [N,C,W,H] tensor.  (None, None): the multi-tile case."""
    if h is None:
        w, h = _in_sizes()
    b = blocks[(0, c)]
    fr = du.frames_nhwc(n, h, w, c)
    planar = du.to_planar(fr)  # [N,C,W,H]
    hi, wi = w, h
    lut = b.lut.cpu().double()
    x = torch.stack([lut[ch % 3][torch.from_numpy(planar[:, ch].astype(np.int64))] for ch in range(c)], 1)
    ref = du.ref_block(x, b.w, b.scale, b.shift, 0, 1)
    assert ref.shape[2:] == (du.out_dims(0, hi, wi, 1)[2], du.out_dims(0, hi, wi, 1)[3])
    got_p, tail_p = b.run(torch.from_numpy(planar).to(b.dev), n, hi, wi, (c * hi * wi, hi * wi, wi, 1))
    got_c, tail_c = b.run(torch.from_numpy(fr).to(b.dev), n, hi, wi, (h * w * c, 1, c, w * c))
    _check("in C=%d N=%d %dx%d planar" % (c, n, h, w), got_p, tail_p, ref)
    _check("in C=%d N=%d %dx%d nhwc" % (c, n, h, w), got_c, tail_c, ref)
    assert torch.equal(got_p, got_c), "the two byte layouts of the same pixels must give the same bits"
    again, _ = b.run(torch.from_numpy(fr).to(b.dev), n, hi, wi, (h * w * c, 1, c, w * c))
    assert torch.equal(again, got_c), "two runs must be bit-identical"


def _c64_sizes(kind):
    from srlz import _cabi as C
    t = C.infer_tile()
    hc, wc = 2 * (t + 1) + 1, 2 * (t + 2) + 1  # pooled (t + 1) x (t + 2) under pool pad 0
    return (hc, wc) if kind == 1 else (2 * hc - 1, 2 * wc - 1)


@pytest.mark.parametrize("kind,n,hi,wi,out_nchw", [(1, 1, 5, 7, False), (1, 3, 9, 13, False), (1, 2, None, None, False),
                                                   (2, 1, 7, 11, False), (2, 2, 27, 27, True), (2, 2, None, None, True)])
def test_block_c64_against_fp64(blocks, kind, n, hi, wi, out_nchw):
    if hi is None:
        hi, wi = _c64_sizes(kind)
    b = blocks[(kind, 64)]
    gen = torch.Generator().manual_seed(100 * kind + n + hi)
    x = torch.randn((n, 64, hi, wi), generator=gen)
    ref = du.ref_block(x, b.w, b.scale, b.shift, kind, 0)
    if (kind, hi, wi) == (1, 5, 7):
        assert ref.shape[2:] == (2, 3)
    if (kind, hi, wi) == (2, 7, 11):
        assert ref.shape[2:] == (1, 2)
    if (kind, hi, wi) == (2, 27, 27):
        assert ref.shape[2:] == (6, 6)
    x_dev = x.permute(0, 2, 3, 1).contiguous().to(b.dev)
    got, tail = b.run(x_dev, n, hi, wi, None, 0, out_nchw)
    _check("kind %d N=%d %dx%d nchw=%d" % (kind, n, hi, wi, out_nchw), got, tail, ref)
    again, _ = b.run(x_dev, n, hi, wi, None, 0, out_nchw)
    assert torch.equal(again, got), "two runs must be bit-identical"


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_rows_of_a_batch_equal_the_frames_run_alone(blocks, kind):
    """Row i of an N = 5 call has the bits of frame i in an N = 1 call (the sum order depends on neither N nor the tiling)."""
    n = 5
    if kind == 0:
        b, c, h, w = blocks[(0, 3)], 3, 17, 23
        x = torch.from_numpy(du.frames_nhwc(n, h, w, c)).to(b.dev)
        hi, wi = w, h
        strides = (h * w * c, 1, c, w * c)
    else:
        b, hi, wi, strides = blocks[(kind, 64)], 11, 13, None
        x = torch.randn((n, hi, wi, 64), generator=torch.Generator().manual_seed(7 + kind)).to(b.dev)
    whole, _ = b.run(x, n, hi, wi, strides)
    for i in range(n):
        one, _ = b.run(x[i:i + 1].contiguous(), 1, hi, wi, strides)
        assert torch.equal(one[0], whole[i]), (kind, i)


def test_a_rejected_descriptor_returns_the_code_and_launches_nothing(blocks):
    from srlz import _cabi as C, ops
    b = blocks[(1, 64)]
    x = torch.zeros((1, 9, 9, 64), device=b.dev)
    out = torch.full((4096,), SENTINEL, dtype=torch.float32, device=b.dev)
    bad = [ops.infer_desc(1, 1, 64, 9, 9, strides=(9 * 9 * 64, 1, 9 * 64, 32)),  # not the contiguous NHWC strides
           ops.infer_desc(1, 1, 64, 2, 9),                                         # the pooled map would be empty
           ops.infer_desc(1, 1, 32, 9, 9),                                         # c_in
           ops.infer_desc(7, 1, 64, 9, 9)]                                         # unknown kind
    for d in bad:
        assert not ops.infer_supported(d)
        rc = C._lib.srlz_infer_block(C.ptr(x), None, C.ptr(b.wpack), C.ptr(b.bnp), C.ptr(out), ctypes.byref(d), C.stream())
        assert rc == -1 and "infer_block" in C.error_text()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((4096,), SENTINEL))
