"""csrc/infer_dec.hip on the GPU: each layer kind of the eval-mode decoder against an fp64 restatement in torch-CPU double
(conv_transpose2d, affine, relu: decode_util.ref_block / ref_out) and the byte expression in numpy (decode_util.bytes_expr).

Shapes: the smallest at which the kernels can go wrong — a 1 x 1 map (every output a border), odd and rectangular maps both ways,
and per kind maps whose cell grid spans MORE THAN ONE WORKGROUP TILE in both directions, sized from srlz_infer_dec_tile(kind) (the
cell grid of an hi x wi map is (hi + 1) x (wi + 1): T x (T + 1) is 2 x 2 tiles with one row and two columns in the second).
Inputs: gamma with negative entries, two channels whose pre-activation is negative everywhere, running variances over two decades,
a sentinel tail behind every output; one out-layer case with biases of +3 and -3 so that both ends of the clip are hit.
Bound for floats: the project's bound for outputs, 1e-4 of the output's scale; the measured maximum is printed (DESIGN.md 3.14
quotes it).  Bytes: exactly the numpy expression on the kernel's OWN fp32 output."""
import ctypes

import numpy as np
import pytest
import torch

import decode_util as dd
import deploy_util as du

pytestmark = pytest.mark.gpu

BOUND = 1e-4
SENTINEL = 1234.5
SENTINEL_U8 = 0xA5
TAIL = 64
DEAD = (5, 37)  # channels whose pre-activation is negative everywhere (beta far below anything the convolution reaches)
FIRST, MID, OUT = 0, 1, 2


class Layer(object):
    """One layer kind on the device: packed weights, bias and (blocks) the BatchNorm record, made once."""

    def __init__(self, kind, c_out, bias=None):
        from srlz import _cabi as C, ops
        self.C, self.ops, self.kind, self.c_out = C, ops, kind, c_out
        self.dev = torch.device("cuda", 0)
        k = 4 if kind == OUT else 3
        gen = torch.Generator().manual_seed(50 + 10 * kind + c_out)
        self.w = torch.randn((64, c_out, k, k), generator=gen) * (2.0 / np.sqrt(64 * k * k))
        self.b = 0.1 * torch.randn((c_out,), generator=gen) if bias is None else torch.tensor(bias, dtype=torch.float32)
        self.wpack = ops.infer_dec_pack(self.w.to(self.dev), kind)
        self.b_dev = self.b.to(self.dev)
        self.bnp = None
        if kind != OUT:
            g, b, m, v = du.bn_formula(3 + kind)
            b = b.clone()
            for c in DEAD:
                b[c] = -1.0e4
            self.bnp = torch.empty(256, dtype=torch.float32, device=self.dev)
            on_dev = [t.to(self.dev) for t in (g, b, m, v)]  # (kept alive until the launch has read them)
            C.bn_eval_params(*[C.ptr(t) for t in on_dev], du.BN_EPS, C.ptr(self.bnp), C.stream())
            rec = self.bnp.cpu()
            self.scale, self.shift = rec[128:192].clone(), rec[192:256].clone()

    def dev_input(self, x):
        """x [N,64,hi,wi] on the CPU -> the layout the kind reads, on the device."""
        return (x if self.kind == FIRST else x.permute(0, 2, 3, 1)).contiguous().to(self.dev)

    def run(self, x_dev, n, hi, wi):
        """fp32 output as [n,c_out,ho,wo] on the CPU (blocks write NHWC, the out layer the decode tensor), and the sentinel tail."""
        ops = self.ops
        d = ops.infer_dec_desc(self.kind, n, hi, wi, c_out=self.c_out)
        assert ops.infer_dec_supported(d)
        ho, wo = ops.infer_dec_out_dims(d)
        numel = n * self.c_out * ho * wo
        out = torch.full((numel + TAIL,), SENTINEL, dtype=torch.float32, device=self.dev)
        if self.kind == OUT:
            ops.infer_dec_out(x_dev, self.wpack, self.b_dev, out, d)
        else:
            ops.infer_dec_block(x_dev, self.wpack, self.b_dev, self.bnp, out, d)
        torch.cuda.synchronize()
        host = out.cpu()
        body = host[:numel].view(n, self.c_out, ho, wo) if self.kind == OUT else host[:numel].view(n, ho, wo, 64).permute(0, 3, 1, 2)
        return body.contiguous(), host[numel:]

    def run_bytes(self, x_dev, n, hi, wi, layout, bgr):
        """uint8 picture in `layout` ("planar" [n,C,W,H] / "nhwc" [n,H,W,C]) on the CPU, and the sentinel tail."""
        ops, c = self.ops, self.c_out
        ho, wo = 2 * hi + 2, 2 * wi + 2  # decode tensor [n,C,W = ho,H = wo]
        strides = (wo * ho * c, 1, c, ho * c) if layout == "nhwc" else (c * ho * wo, ho * wo, wo, 1)
        d = ops.infer_dec_desc(OUT, n, hi, wi, c_out=c, out_u8=True, bgr=bgr, out_strides=strides)
        assert ops.infer_dec_supported(d) and ops.infer_dec_out_dims(d) == (ho, wo)
        numel = n * c * ho * wo
        out = torch.full((numel + TAIL,), SENTINEL_U8, dtype=torch.uint8, device=self.dev)
        ops.infer_dec_out(x_dev, self.wpack, self.b_dev, out, d)
        torch.cuda.synchronize()
        host = out.cpu()
        body = host[:numel].view((n, wo, ho, c) if layout == "nhwc" else (n, c, ho, wo))
        return body.numpy().copy(), host[numel:]


@pytest.fixture(scope="module")
def layers():
    assert torch.cuda.is_available()
    return {(FIRST, 64): Layer(FIRST, 64), (MID, 64): Layer(MID, 64), (OUT, 3): Layer(OUT, 3), (OUT, 6): Layer(OUT, 6),
            "clip": Layer(OUT, 3, bias=[3.0, -3.0, 0.05])}


def _x(n, hi, wi, seed):
    return torch.randn((n, 64, hi, wi), generator=torch.Generator().manual_seed(seed))


def _check(tag, got, tail, ref, block):
    assert torch.equal(tail, torch.full_like(tail, SENTINEL)), "%s: wrote behind its output" % tag
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = (got.double() - ref).abs().max().item() / ref.abs().max().item()
    print("%s: max |err| / max |ref| = %.3e (output %s)" % (tag, err, tuple(ref.shape)))
    assert err <= BOUND, (tag, err)
    if block:
        for c in DEAD:
            assert float(got[:, c].abs().max()) == 0.0, (tag, c)
        assert float(got.min()) >= 0.0 and float(got.max()) > 0.0


def _tile(kind):
    from srlz import _cabi as C
    t = C.infer_dec_tile(kind)
    assert t >= 1
    return t


@pytest.mark.parametrize("n,hi,wi", [(3, 1, 1), (3, 2, 3), (1, 6, 6)])
def test_block_first_against_fp64(layers, n, hi, wi):
    la = layers[(FIRST, 64)]
    x = _x(n, hi, wi, 11 * hi + wi)
    ref = dd.ref_block(x, la.w, la.b, la.scale, la.shift)
    assert ref.shape[2:] == (2 * hi + 1, 2 * wi + 1)
    got, tail = la.run(la.dev_input(x), n, hi, wi)
    _check("first N=%d %dx%d" % (n, hi, wi), got, tail, ref, True)
    again, _ = la.run(la.dev_input(x), n, hi, wi)
    assert torch.equal(again, got), "two runs must be bit-identical"


@pytest.mark.parametrize("n,hi,wi", [(2, 1, 1), (1, 3, 2), (2, 2, 3), (1, "T", "T+1"), (2, "T+1", "T+2"), (1, "T+2", "T+1")])
def test_block_mid_against_fp64(layers, n, hi, wi):
    t = _tile(MID)
    size = {"T": t, "T+1": t + 1, "T+2": t + 2}
    hi, wi = size.get(hi, hi), size.get(wi, wi)
    la = layers[(MID, 64)]
    x = _x(n, hi, wi, 100 + 13 * hi + wi)
    ref = dd.ref_block(x, la.w, la.b, la.scale, la.shift)
    got, tail = la.run(la.dev_input(x), n, hi, wi)
    _check("mid N=%d %dx%d" % (n, hi, wi), got, tail, ref, True)
    again, _ = la.run(la.dev_input(x), n, hi, wi)
    assert torch.equal(again, got), "two runs must be bit-identical"


@pytest.mark.parametrize("c", [3, 6])
@pytest.mark.parametrize("n,hi,wi", [(2, 1, 1), (2, 5, 7), (1, 7, 5), (1, "T", "T+1")])
def test_out_layer_floats_and_bytes(layers, c, n, hi, wi):
    """Floats against fp64; bytes of both layouts, bgr on and off, exactly the expression on the kernel's own floats."""
    t = _tile(OUT)
    size = {"T": t, "T+1": t + 1}
    hi, wi = size.get(hi, hi), size.get(wi, wi)
    la = layers[(OUT, c)]
    x = _x(n, hi, wi, 200 + 17 * hi + wi + c)
    ref = dd.ref_out(x, la.w, la.b)
    assert ref.shape[1:] == (c, 2 * hi + 2, 2 * wi + 2)
    x_dev = la.dev_input(x)
    got, tail = la.run(x_dev, n, hi, wi)
    _check("out C=%d N=%d %dx%d" % (c, n, hi, wi), got, tail, ref, False)
    again, _ = la.run(x_dev, n, hi, wi)
    assert torch.equal(again, got), "two runs must be bit-identical"
    for bgr in (False, True):
        planar, tail_p = la.run_bytes(x_dev, n, hi, wi, "planar", bgr)
        nhwc, tail_c = la.run_bytes(x_dev, n, hi, wi, "nhwc", bgr)
        assert (tail_p == SENTINEL_U8).all() and (tail_c == SENTINEL_U8).all(), "wrote behind its picture"
        assert np.array_equal(planar, dd.bytes_expr(got.numpy(), "planar", bgr)), (c, bgr)
        assert np.array_equal(nhwc, dd.bytes_expr(got.numpy(), "nhwc", bgr)), (c, bgr)
        assert np.array_equal(nhwc, planar.transpose(0, 3, 2, 1)), "the two byte layouts must hold the same bytes"
        again_b, _ = la.run_bytes(x_dev, n, hi, wi, "nhwc", bgr)
        assert np.array_equal(again_b, nhwc)
    assert planar.std() > 5.0  # (a picture, not a flat field)


def test_out_layer_bytes_hit_both_ends_of_the_clip(layers):
    la = layers["clip"]
    n, hi, wi = 1, 5, 7
    x = 0.1 * _x(n, hi, wi, 77)  # (the layer's output then stays within a few tenths of its bias)
    x_dev = la.dev_input(x)
    got, tail = la.run(x_dev, n, hi, wi)
    _check("out clip", got, tail, dd.ref_out(x, la.w, la.b), False)
    planar, _ = la.run_bytes(x_dev, n, hi, wi, "planar", False)
    assert np.array_equal(planar, dd.bytes_expr(got.numpy()))
    assert (planar[:, 0] == 255).all() and (planar[:, 1] == 0).all()  # +3 and -3: beyond 1 and below 0 after deNormalize
    assert 0 < planar[:, 2].min() and planar[:, 2].max() < 255
    nan = x.clone()
    nan[0, 0, 2, 3] = float("nan")
    got_n, _ = la.run(la.dev_input(nan), n, hi, wi)
    by_n, _ = la.run_bytes(la.dev_input(nan), n, hi, wi, "planar", False)
    assert torch.isnan(got_n).any() and np.array_equal(by_n, dd.bytes_expr(got_n.numpy()))  # NaN gives 0
    assert (by_n[np.isnan(got_n.numpy())] == 0).all()


@pytest.mark.parametrize("kind", [FIRST, MID, OUT])
def test_rows_of_a_batch_equal_the_states_run_alone(layers, kind):
    """Row i of an N = 5 call has the bits of input i in an N = 1 call (the sum order depends on neither N nor the tiling)."""
    n, t = 5, _tile(kind)
    la = layers[(kind, 3 if kind == OUT else 64)]
    hi, wi = t + 1, t + 2
    x = _x(n, hi, wi, 300 + kind)
    whole, _ = la.run(la.dev_input(x), n, hi, wi)
    if kind == OUT:
        whole_b, _ = la.run_bytes(la.dev_input(x), n, hi, wi, "nhwc", True)
    for i in range(n):
        one, _ = la.run(la.dev_input(x[i:i + 1]), 1, hi, wi)
        assert torch.equal(one[0], whole[i]), (kind, i)
        if kind == OUT:
            one_b, _ = la.run_bytes(la.dev_input(x[i:i + 1]), 1, hi, wi, "nhwc", True)
            assert np.array_equal(one_b[0], whole_b[i]), i


def test_rejected_descriptors_return_the_code_and_launch_nothing(layers):
    from srlz import _cabi as C, ops
    mid, out3 = layers[(MID, 64)], layers[(OUT, 3)]
    x = torch.zeros((1, 6, 6, 64), device=mid.dev)
    out = torch.full((65536,), SENTINEL, dtype=torch.float32, device=mid.dev)
    bad_block = [ops.infer_dec_desc(MID, 1, 6, 6, in_strides=(64 * 36, 36, 6, 1)),  # not the contiguous NHWC strides
                 ops.infer_dec_desc(MID, 1, 0, 6),                                   # an empty map
                 ops.infer_dec_desc(MID, 1, 6, 6, c_in=32), ops.infer_dec_desc(MID, 1, 6, 6, c_out=3),
                 ops.infer_dec_desc(7, 1, 6, 6),                                     # unknown kind
                 ops.infer_dec_desc(OUT, 1, 6, 6)]                                   # a kind of the other entry point
    for d in bad_block:
        rc = C._lib.srlz_infer_dec_block(C.ptr(x), C.ptr(mid.wpack), C.ptr(mid.b_dev), C.ptr(mid.bnp), C.ptr(out), ctypes.byref(d),
                                         C.stream())
        assert rc == -1 and "infer_dec_block" in C.error_text()
    bad_out = [ops.infer_dec_desc(OUT, 1, 6, 6, c_out=4),
               ops.infer_dec_desc(OUT, 1, 6, 6, out_u8=True, out_strides=(1, 1, 1, 1)),  # elements share a byte
               ops.infer_dec_desc(OUT, 1, 6, 6, in_strides=(64 * 36, 36, 6, 1)),
               ops.infer_dec_desc(MID, 1, 6, 6)]
    for d in bad_out:
        rc = C._lib.srlz_infer_dec_out(C.ptr(x), C.ptr(out3.wpack), C.ptr(out3.b_dev), C.ptr(out), ctypes.byref(d), C.stream())
        assert rc == -1 and "infer_dec_out" in C.error_text()
    for d in bad_block[:5] + bad_out[:3]:
        assert not ops.infer_dec_supported(d)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((65536,), SENTINEL))
