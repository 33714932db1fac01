"""Kernel-level parity (GPU) for the frozen ResNet-18 trunk and the EmbeddingNet head of `--multi-view --losses triplet`: every
entry point that only that route uses, by name, against fp64 torch-CPU functional ops on the same seeded inputs.

 A  srlz_convn_fwd (+ srlz_convn_pack_weights / srlz_convn_fwd_tiles / srlz_convn_packed_floats) per layer against fp64 F.conv2d:
    every element of y, the per-tile statistics partials per BatchNorm group and block of 64 output channels, with and without the
    fused relu(scale * x + shift) operand; bit-identity of two runs, of stats = NULL, and of a groups = G launch with G launches.
 B  srlz_bn_finalize_chunks / srlz_bn_eval_params_chunks: all four quarters of every [group][block][256] record, the running
    statistics after the groups' momentum updates in order, num_batches_tracked — with random, negative and zero affine parameters.
 C  srlz_bn_add_relu (both forms) and srlz_avgpool_nhwc.
 D  srlz_prelu_fwd / srlz_prelu_bwd and srlz_triplet_fwd / srlz_triplet_bwd against fp64 autograd.
 E  the whole trunk (hotpath.resnet18_forward, EmbeddingNet.forward / getStates) on a state whose BatchNorm layers are NOT the
    (weight 1, bias 0, mean 0, var 1) of a fresh module, and the SRLZ_RESNET18_WEIGHTS route.
 F  descriptors that every entry point must refuse before it launches anything.

Tolerances: bit-for-bit claims use torch.equal; fp32 against fp64 uses 1e-4 of the reference's largest magnitude (BASELINE.json
north_star, as tests/test_kernels_gpu.py).  For every convolution shape and for the whole trunk the same operation in fp32 torch-CPU
is also compared with fp64 and printed next to the GPU's error: a case counts only if that fp32 reference alone stays within
2.5e-5, a quarter of the ceiling.  Measured figures: profiles/NOTES.md.

Shapes refused by design: none of section A's.  The degenerate 1 x 1 and 2 x 2 maps build a grid program (the virtual grid is never
narrower than two columns) and are checked like every other shape.
"""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4        # BASELINE.json north_star
REF_CAP = 2.5e-5  # the fp32 CPU reference's own error against fp64 may use a quarter of TOL
EPS, MOMENTUM = 1e-5, 0.1  # nn.BatchNorm2d defaults (srlz.ops.BN_EPS / BN_MOMENTUM)
NAN = float("nan")


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = ref.abs().max().item()
    return (got - ref).abs().max().item() / max(scale, 1e-30)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    assert torch.cuda.is_available()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return _cabi


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def affine_records(groups, chunks, gen):
    """[groups][chunks][256] records as a consumer of (scale, shift) sees them: different per group, block and channel, one scale in
    five negative, two per record exactly 0; the (mean, invstd) quarters are NaN — nothing downstream may read them."""
    rec = torch.full((groups, chunks, 256), NAN)
    scale = torch.rand(groups, chunks, 64, generator=gen) + 0.5
    scale = torch.where(torch.rand(groups, chunks, 64, generator=gen) < 0.2, -scale, scale)
    for g in range(groups):
        for c in range(chunks):
            scale[g, c, torch.randperm(64, generator=gen)[:2]] = 0.0
    rec[:, :, 128:192] = scale
    rec[:, :, 192:] = 0.3 * torch.randn(groups, chunks, 64, generator=gen)
    return rec


def scale_shift(rec, g):
    """Per-channel (scale, shift) of group g as [1, C, 1, 1] fp64."""
    return (rec[g, :, 128:192].reshape(1, -1, 1, 1).double(), rec[g, :, 192:].reshape(1, -1, 1, 1).double())


# ---------------------------------------------------------------------------------------------------------------------------------
# A. srlz_convn_fwd per layer
# ---------------------------------------------------------------------------------------------------------------------------------
# (cin, cout, k, stride, hi, wi, n, groups)
RESNET = [(64, 128, 3, 2, 56, 56, 3, 1), (128, 128, 3, 1, 28, 28, 3, 1), (64, 128, 1, 2, 56, 56, 3, 1),
          (128, 256, 3, 2, 28, 28, 3, 1), (256, 256, 3, 1, 14, 14, 3, 1), (128, 256, 1, 2, 28, 28, 3, 1),
          (256, 512, 3, 2, 14, 14, 3, 1), (512, 512, 3, 1, 7, 7, 3, 1), (256, 512, 1, 2, 14, 14, 3, 1)]
EDGES = [
    (512, 512, 3, 2, 7, 7, 3, 1), (256, 512, 1, 2, 7, 7, 3, 1),        # odd side under stride 2: 7 -> 4
    (128, 256, 3, 2, 13, 13, 2, 1), (128, 256, 1, 2, 13, 13, 2, 1),    # 13 -> 7
    (128, 128, 3, 1, 5, 9, 2, 1), (128, 128, 3, 1, 9, 5, 2, 1),        # not square: a swapped h / w shows
    (128, 256, 3, 2, 13, 7, 2, 1), (128, 256, 1, 2, 13, 7, 2, 1), (64, 128, 3, 2, 6, 11, 2, 1), (64, 128, 1, 2, 6, 11, 2, 1),
    (256, 256, 3, 1, 14, 14, 1, 1),                                     # n = 1
    (128, 128, 3, 1, 7, 7, 5, 1),                                       # 5 x 64 grid positions: the third tile is half empty
    (128, 128, 3, 1, 1, 1, 4, 1), (128, 256, 3, 2, 1, 1, 4, 1), (128, 256, 1, 2, 1, 1, 4, 1),   # 1 x 1 maps
    (128, 128, 3, 1, 2, 2, 3, 1), (128, 256, 3, 2, 2, 2, 3, 1), (128, 256, 1, 2, 2, 2, 3, 1),   # 2 x 2 maps
    (128, 64, 3, 1, 9, 9, 2, 1), (256, 64, 1, 2, 9, 9, 2, 1),          # cout < cin
    (64, 64, 3, 2, 56, 56, 2, 1), (64, 64, 1, 2, 56, 56, 2, 1),        # 64 -> 64 outside the hot path's own 64 -> 64 stride-1 kernels
    (128, 128, 3, 1, 14, 14, 4, 2), (64, 128, 3, 2, 28, 28, 6, 3), (128, 256, 1, 2, 14, 14, 6, 3), (256, 512, 3, 2, 7, 5, 6, 6),
    (512, 512, 3, 1, 7, 7, 12, 6),                                      # BatchNorm groups
    (64, 128, 3, 2, 56, 56, 64, 2),                                     # 422 tiles: not a multiple of 8 on the XCD walk
]


def convn_desc(C, cin, cout, k, s, hi, wi, n, groups):
    p = 1 if k == 3 else 0
    ho, wo = (hi + 2 * p - k) // s + 1, (wi + 2 * p - k) // s + 1
    return C.ConvNDesc(n, hi, wi, ho, wo, cin, cout, k, s, p, groups), p, ho, wo


def convn_pack(C, w, d):
    wd = w.to(DEV)
    pk = nans(C.convn_packed_floats(d))
    C.convn_pack_weights(C.ptr(wd), C.ptr(pk), d, C.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(pk).all()  # every slot of the packed copy is written (the 1 x 1 kernel's eight other taps as zeros)
    return pk


def convn_launch(C, xd, pk, bnp, d, cout, want_stats=True):
    y = nans(d.n, d.ho, d.wo, cout)
    tiles = C.convn_fwd_tiles(d)
    assert tiles > 0
    stats = nans(cout // 64, tiles, 128) if want_stats else None
    C.convn_fwd(C.ptr(xd), C.ptr(pk), C.ptr(y), C.ptr(stats), C.ptr(bnp), d, C.stream())
    torch.cuda.synchronize()
    return y, stats, tiles


def _case_id(c):
    return "%dto%d_k%ds%d_%dx%d_n%d_g%d" % c


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("case", RESNET + EDGES, ids=_case_id)
def test_convn_fwd_per_layer(C, case, fused):
    cin, cout, k, s, hi, wi, n, G = case
    d, p, ho, wo = convn_desc(C, *case)
    npg = n // G
    gen = torch.Generator().manual_seed(1000 * cin + 100 * k + 10 * s + hi + 3 * wi + n + (7 if fused else 0))
    x = torch.randn(n, cin, hi, wi, generator=gen) + 0.5
    w = torch.randn(cout, cin, k, k, generator=gen) / float(np.sqrt(cin * k * k))
    rec = affine_records(G, cin // 64, gen) if fused else None

    # fp64 reference per group, and the same in fp32 (the reference's own error)
    yr, y32 = [], []
    for g in range(G):
        xg = x[g * npg:(g + 1) * npg]
        a64, a32 = xg.double(), xg
        if fused:
            sc, sh = scale_shift(rec, g)
            a64, a32 = F.relu(a64 * sc + sh), F.relu(a32 * sc.float() + sh.float())
        yr.append(F.conv2d(a64, w.double(), None, s, p))
        y32.append(F.conv2d(a32, w, None, s, p))
    yr, y32 = torch.cat(yr), torch.cat(y32)
    assert tuple(yr.shape) == (n, cout, ho, wo)
    e_ref = rel_err(y32, yr)

    xd = nhwc(x).to(DEV)
    pk = convn_pack(C, w, d)
    bnp = rec.to(DEV) if fused else None
    y, stats, tiles = convn_launch(C, xd, pk, bnp, d, cout)
    assert tiles % G == 0
    tpg = tiles // G
    if n == 64:
        assert tiles % 8 != 0
    e_y = rel_err(nchw(y), yr)
    # statistics partials: per group and block of 64 output channels, sum and sum of squares over that group's tiles
    e_s = e_q = 0.0
    for g in range(G):
        flat = yr[g * npg:(g + 1) * npg].permute(1, 0, 2, 3).reshape(cout, -1)
        for co in range(cout // 64):
            part = stats[co, g * tpg:(g + 1) * tpg].double().sum(0).cpu()
            e_s = max(e_s, rel_err(part[:64], flat[co * 64:(co + 1) * 64].sum(1)))
            e_q = max(e_q, rel_err(part[64:], (flat[co * 64:(co + 1) * 64] ** 2).sum(1)))
    print("A %s %s: y %.2e (fp32 reference %.2e) sum %.2e sumsq %.2e, %d tiles"
          % (_case_id(case), "fused" if fused else "plain", e_y, e_ref, e_s, e_q, tiles))
    assert e_ref <= REF_CAP, e_ref
    assert torch.isfinite(y).all() and torch.isfinite(stats).all()
    assert e_y < TOL, e_y
    assert e_s < TOL and e_q < TOL, (e_s, e_q)

    # two runs are the same bits; so is a run that asks for no statistics
    y2, stats2, _ = convn_launch(C, xd, pk, bnp, d, cout)
    assert torch.equal(y2, y) and torch.equal(stats2, stats)
    y3, _, _ = convn_launch(C, xd, pk, bnp, d, cout, want_stats=False)
    assert torch.equal(y3, y)
    # a groups = G launch is G launches of one group each, bit for bit
    if G > 1:
        d1, _, _, _ = convn_desc(C, cin, cout, k, s, hi, wi, npg, 1)
        for g in range(G):
            yg, sg, t1 = convn_launch(C, xd[g * npg:(g + 1) * npg], pk, bnp[g] if fused else None, d1, cout)
            assert t1 == tpg
            assert torch.equal(yg, y[g * npg:(g + 1) * npg]), g
            assert torch.equal(sg, stats[:, g * tpg:(g + 1) * tpg]), g


def test_convn_pack_weights_layout_is_independent_of_the_map(C):
    """The packed copy depends on (cin, cout, k) only — hotpath._packed keeps one per module whatever the batch — and
    srlz_convn_packed_floats is cin/64 * cout/64 * 9 * 4096."""
    gen = torch.Generator().manual_seed(5)
    for k, s in ((3, 1), (1, 2)):
        w = torch.randn(256, 128, k, k, generator=gen)
        da = convn_desc(C, 128, 256, k, s, 14, 14, 3, 1)[0]
        db = convn_desc(C, 128, 256, k, s, 5, 9, 6, 3)[0]
        assert C.convn_packed_floats(da) == C.convn_packed_floats(db) == 2 * 4 * 9 * 4096
        pa, pb = convn_pack(C, w, da), convn_pack(C, w, db)
        assert torch.equal(pa, pb)
        # a permutation of the weights (3 x 3), or of the weights and 8 x as many zeros (1 x 1)
        got = torch.sort(pa.cpu().abs())[0]
        want = torch.sort(torch.cat([w.reshape(-1).abs(), torch.zeros(pa.numel() - w.numel())]))[0]
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. BatchNorm records for C > 64
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_affine(ch, gen):
    """The recipe of section E for one BatchNorm: weight U(0.5, 1.5) with one sign in ten flipped and two channels exactly 0,
    bias 0.3 N(0, 1), running_mean 0.5 N(0, 1), running_var U(0.5, 1.5)."""
    weight = torch.rand(ch, generator=gen) + 0.5
    weight = torch.where(torch.rand(ch, generator=gen) < 0.1, -weight, weight)
    weight[torch.randperm(ch, generator=gen)[:2]] = 0.0
    bias = 0.3 * torch.randn(ch, generator=gen)
    mean = 0.5 * torch.randn(ch, generator=gen)
    var = torch.rand(ch, generator=gen) + 0.5
    return weight, bias, mean, var


def check_records(bnp, mean, invstd, gamma, beta, chunks):
    """bnp [chunks][256] (one group) against per-channel fp64 mean / invstd: all four quarters."""
    got = bnp.reshape(chunks, 4, 64).double().cpu()
    scale = gamma.double() * invstd
    want = torch.stack([mean, invstd, scale, beta.double() - mean * scale]).reshape(4, chunks, 64).permute(1, 0, 2)
    assert torch.isfinite(got).all()
    return max(rel_err(got[:, q], want[:, q]) for q in range(4))


@pytest.mark.parametrize("tiny", [False, True], ids=["count50", "count2"])
@pytest.mark.parametrize("groups", [1, 2, 6])
@pytest.mark.parametrize("chunks", [1, 2, 4, 8])
def test_bn_finalize_chunks(C, chunks, groups, tiny):
    """Train mode, on the partials of a real srlz_convn_fwd launch.  count2: two 1 x 1 images per group (n * ho * wo = 2) — the
    unbiased-variance factor count / (count - 1) is 2; the second image is -0.5 x the first, so that no channel's variance is a
    difference of nearly equal fp32 sums (var / mean-square = 0.9 for every channel)."""
    cout, G = 64 * chunks, groups
    hi, npg = (1, 2) if tiny else (9, 2)
    case = (64, cout, 3, 2, hi, hi, npg * G, G)
    d, p, ho, wo = convn_desc(C, *case)
    count = npg * ho * wo
    assert count == (2 if tiny else 50)
    gen = torch.Generator().manual_seed(31 * chunks + 7 * groups + int(tiny))
    x = torch.randn(npg * G, 64, hi, hi, generator=gen)
    if tiny:
        x[1::2] = -0.5 * x[0::2]
    w = torch.randn(cout, 64, 3, 3, generator=gen) / 24.0
    gamma, beta, rm0, rv0 = bn_affine(cout, gen)
    yr = F.conv2d(x.double(), w.double(), None, 2, 1)

    y, stats, tiles = convn_launch(C, nhwc(x).to(DEV), convn_pack(C, w, d), None, d, cout)
    gd, bd, rm, rv = gamma.to(DEV), beta.to(DEV), rm0.to(DEV), rv0.to(DEV)
    tick = torch.tensor([5], dtype=torch.int64, device=DEV)
    bnp = nans(G, chunks, 256)
    nbytes = C.bn_finalize_chunks_workspace(chunks, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    C.bn_finalize_chunks(C.ptr(stats), tiles, chunks, G, count, C.ptr(gd), C.ptr(bd), EPS, MOMENTUM, C.ptr(rm), C.ptr(rv), C.ptr(tick),
                         C.ptr(bnp), C.ptr(ws), nbytes, C.stream())
    torch.cuda.synchronize()

    # reference: G sequential F.batch_norm(training=True) calls in fp64 on the running statistics
    rm_r, rv_r = rm0.double(), rv0.double()
    worst = 0.0
    for g in range(G):
        yg = yr[g * npg:(g + 1) * npg]
        F.batch_norm(yg, rm_r, rv_r, gamma.double(), beta.double(), True, MOMENTUM, EPS)
        mean = yg.mean((0, 2, 3))
        invstd = 1.0 / torch.sqrt(yg.var((0, 2, 3), unbiased=False) + EPS)
        worst = max(worst, check_records(bnp[g], mean, invstd, gamma, beta, chunks))
    e_rm, e_rv = rel_err(rm, rm_r), rel_err(rv, rv_r)
    print("B finalize chunks=%d groups=%d count=%d: records %.2e running_mean %.2e running_var %.2e" % (chunks, G, count, worst, e_rm, e_rv))
    assert worst < TOL and e_rm < TOL and e_rv < TOL, (worst, e_rm, e_rv)
    assert int(tick) == 5 + G

    # the batched launch is G single-group launches in order, bit for bit (records, running statistics, counter)
    if G > 1:
        rm1, rv1 = rm0.to(DEV), rv0.to(DEV)
        tick1 = torch.tensor([5], dtype=torch.int64, device=DEV)
        tpg = tiles // G
        nb1 = C.bn_finalize_chunks_workspace(chunks, 1)
        for g in range(G):
            one = nans(chunks, 256)
            sg = stats[:, g * tpg:(g + 1) * tpg].contiguous()
            C.bn_finalize_chunks(C.ptr(sg), tpg, chunks, 1, count, C.ptr(gd), C.ptr(bd), EPS, MOMENTUM, C.ptr(rm1), C.ptr(rv1),
                                 C.ptr(tick1), C.ptr(one), C.ptr(ws), nb1, C.stream())
            torch.cuda.synchronize()
            assert torch.equal(one, bnp[g]), g
        assert torch.equal(rm1, rm) and torch.equal(rv1, rv) and int(tick1) == 5 + G


@pytest.mark.parametrize("chunks", [1, 2, 4, 8])
def test_bn_eval_params_chunks(C, chunks):
    ch = 64 * chunks
    gen = torch.Generator().manual_seed(77 + chunks)
    gamma, beta, rm0, rv0 = bn_affine(ch, gen)
    gd, bd, rm, rv = gamma.to(DEV), beta.to(DEV), rm0.to(DEV), rv0.to(DEV)
    bnp = nans(chunks, 256)
    C.bn_eval_params_chunks(C.ptr(gd), C.ptr(bd), C.ptr(rm), C.ptr(rv), EPS, chunks, C.ptr(bnp), C.stream())
    torch.cuda.synchronize()
    invstd = 1.0 / torch.sqrt(rv0.double() + EPS)
    e = check_records(bnp, rm0.double(), invstd, gamma, beta, chunks)
    print("B eval chunks=%d: records %.2e" % (chunks, e))
    assert e < TOL
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)  # eval mode moves nothing
    # what the hot path builds from it: the same record for every group, [groups][chunks][256]; nothing moves, no tick
    from srlz import hotpath
    bn = torch.nn.BatchNorm2d(ch)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    bn = bn.to(DEV).eval()
    for groups in (1, 2, 6):
        r = hotpath._bn_record(bn, None, 0, 0, False, torch.device(DEV, torch.cuda.current_device()), groups)
        assert torch.equal(r.reshape(groups, chunks, 256), bnp.expand(groups, chunks, 256))
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean.cpu(), rm0)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. srlz_bn_add_relu, srlz_avgpool_nhwc
# ---------------------------------------------------------------------------------------------------------------------------------
# 36 000 pixels: 576 000 .. 4 608 000 float4 elements, more than 8 workgroups of 256 threads per CU can hold at once on any CDNA part
# (2048 x 256 = 524 288 on 256 CUs): the grid-stride loop goes round.  3 pixels: one per group.
@pytest.mark.parametrize("pixels", [36000, 3], ids=["wrap", "tiny"])
@pytest.mark.parametrize("downsample", [True, False], ids=["b_bnp", "identity"])
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("chunks", [1, 2, 8])
def test_bn_add_relu(C, chunks, groups, downsample, pixels):
    ch, G = 64 * chunks, groups
    if pixels > 3:
        assert pixels * chunks * 16 > 8 * C.device_cus() * 256
    gen = torch.Generator().manual_seed(13 * chunks + groups + 2 * int(downsample) + pixels)
    a = torch.randn(pixels, ch, generator=gen)
    b = torch.randn(pixels, ch, generator=gen)
    ra = affine_records(G, chunks, gen)
    rb = affine_records(G, chunks, gen) if downsample else None
    per = pixels // G
    ref = []
    for g in range(G):
        sa, ha = (t.reshape(1, ch) for t in scale_shift(ra, g))
        z = a[g * per:(g + 1) * per].double() * sa + ha
        bg = b[g * per:(g + 1) * per].double()
        if downsample:
            sb, hb = (t.reshape(1, ch) for t in scale_shift(rb, g))
            bg = bg * sb + hb
        ref.append(F.relu(z + bg))
    ref = torch.cat(ref)
    ad, bd, rad = a.to(DEV), b.to(DEV), ra.to(DEV)
    rbd = rb.to(DEV) if downsample else None
    out = nans(pixels, ch)
    C.bn_add_relu(C.ptr(ad), C.ptr(rad), C.ptr(bd), C.ptr(rbd), C.ptr(out), pixels, chunks, G, C.stream())
    torch.cuda.synchronize()
    e = rel_err(out, ref)
    print("C bn_add_relu chunks=%d groups=%d %s pixels=%d: %.2e" % (chunks, G, "b_bnp" if downsample else "identity", pixels, e))
    assert torch.isfinite(out).all()
    assert e < TOL, e


@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("c", [64, 512])
@pytest.mark.parametrize("hw", [1, 16, 49])
def test_avgpool_nhwc(C, hw, c, n):
    gen = torch.Generator().manual_seed(hw + c + n)
    x = torch.randn(n, hw, c, generator=gen) + 0.25
    xd = x.to(DEV)
    out = nans(n, c)
    C.avgpool_nhwc(C.ptr(xd), C.ptr(out), n, hw, c, C.stream())
    torch.cuda.synchronize()
    e = rel_err(out, x.double().mean(1))
    print("C avgpool hw=%d c=%d n=%d: %.2e" % (hw, c, n, e))
    assert e < TOL, e


# ---------------------------------------------------------------------------------------------------------------------------------
# D. head kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def prelu_inputs(n, gen):
    x = torch.randn(n, generator=gen)
    x[torch.rand(n, generator=gen) < 0.15] = 0.0  # exact zeros: the x <= 0 side of the subgradient, as torch
    if n == 1:
        x[0] = -0.75
    elif n >= 4:
        x[0], x[1], x[n - 1] = 0.0, -0.0, 0.0
    return x, torch.randn(n, generator=gen)


def prelu_reference(x, slope, dy):
    xr = x.double().requires_grad_(True)
    sr = torch.tensor([slope], dtype=torch.float64, requires_grad=True)
    yr = F.prelu(xr, sr)
    yr.backward(dy.double())
    return yr.detach(), xr.grad, sr.grad


@pytest.mark.parametrize("slope", [0.25, 0.0, -0.5])
@pytest.mark.parametrize("n", [1, 63, 128, 896, 1000, 32768])
def test_prelu_c_abi(C, n, slope):
    gen = torch.Generator().manual_seed(1000 + n + int(100 * slope))
    x, dy = prelu_inputs(n, gen)
    yr, dxr, dsr = prelu_reference(x, slope, dy)
    xd, dyd = x.to(DEV), dy.to(DEV)
    sd = torch.tensor([slope], dtype=torch.float32, device=DEV)
    y, dx, ds = nans(n), nans(n), nans(1)
    C.prelu_fwd(C.ptr(xd), C.ptr(sd), C.ptr(y), n, C.stream())
    C.prelu_bwd(C.ptr(xd), C.ptr(sd), C.ptr(dyd), C.ptr(dx), C.ptr(ds), n, C.stream())
    torch.cuda.synchronize()
    e = (rel_err(y, yr), rel_err(dx, dxr), rel_err(ds, dsr))
    print("D prelu n=%d slope=%g: y %.2e dx %.2e dslope %.2e" % ((n, slope) + e))
    assert max(e) < TOL, e
    # the subgradient at exact zeros is the slope's side (torch: x > 0 ? g : a * g)
    z = x == 0
    assert torch.equal(dx.cpu()[z], (slope * dy.double()[z]).float())


@pytest.mark.parametrize("slope", [0.25, 0.0, -0.5])
@pytest.mark.parametrize("B", [1, 7, 256])
def test_prelu_autograd_function(C, B, slope):
    """ops.PReLUFn on the head's [B, 128] tensor (n = 128 B)."""
    from srlz import ops
    gen = torch.Generator().manual_seed(2000 + B + int(100 * slope))
    x, dy = prelu_inputs(128 * B, gen)
    yr, dxr, dsr = prelu_reference(x, slope, dy)
    xd = x.reshape(B, 128).to(DEV).requires_grad_(True)
    sd = torch.nn.Parameter(torch.tensor([slope], dtype=torch.float32, device=DEV))
    y = ops.PReLUFn.apply(xd, sd)
    y.backward(dy.reshape(B, 128).to(DEV))
    torch.cuda.synchronize()
    e = (rel_err(y.reshape(-1), yr), rel_err(xd.grad.reshape(-1), dxr), rel_err(sd.grad, dsr))
    print("D PReLUFn B=%d slope=%g: y %.2e dx %.2e dslope %.2e" % ((B, slope) + e))
    assert max(e) < TOL, e


def triplet_inputs(B, S, mode, alpha, gen):
    """Rows whose hinge argument |s-p|^2 - |s-n|^2 + alpha is far from 0 on the chosen side (at least 0.3 |s-p|^2 + 0.5), so that the
    fp32 kernel and the fp64 reference take the same branch: the negative is the anchor displaced along the same direction as the
    positive, by 0.5 of the distance (active) or by 1.5 of it plus a margin (inactive)."""
    s = torch.randn(B, S, generator=gen)
    u = torch.randn(B, S, generator=gen)
    u = u / u.norm(dim=1, keepdim=True)
    r = 1.0 + torch.rand(B, 1, generator=gen)                   # |s - p|
    if mode == "mixed":
        active = torch.rand(B, 1, generator=gen) < 0.6
        active[0] = True
        if B > 1:
            active[B - 1] = False
    else:
        active = torch.full((B, 1), mode == "active", dtype=torch.bool)
    rn = torch.where(active, 0.5 * r, 1.5 * r + 1.0)            # |s - n|
    p = s + r * u
    v = torch.randn(B, S, generator=gen)
    v = v / v.norm(dim=1, keepdim=True)
    n = s + rn * (u if S == 1 else v)
    arg = (s - p).double().pow(2).sum(1) - (s - n).double().pow(2).sum(1) + alpha
    assert bool(((arg > 0.5) == active.reshape(-1)).all()) and bool((arg.abs() > 0.5).all())
    return s, p, n, active.reshape(-1)


@pytest.mark.parametrize("alpha", [0.0, 0.2])
@pytest.mark.parametrize("mode", ["mixed", "inactive", "active"])
@pytest.mark.parametrize("S", [1, 3, 128, 200])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1000])
def test_triplet_fwd_bwd(C, B, S, mode, alpha):
    from oracle import torch_twin as T
    gen = torch.Generator().manual_seed(B * 1000 + S + int(10 * alpha) + len(mode))
    s, p, n, active = triplet_inputs(B, S, mode, alpha, gen)
    up = -1.75  # upstream gradient
    sr, pr, nr = (t.double().requires_grad_(True) for t in (s, p, n))
    lr = T.triplet_loss(sr, pr, nr, alpha)
    (up * lr).backward()
    sd, pd, nd = s.to(DEV), p.to(DEV), n.to(DEV)
    g = torch.tensor([up], dtype=torch.float32, device=DEV)
    out, hinge = nans(1), nans(B)
    ds, dp, dn = nans(B, S), nans(B, S), nans(B, S)
    C.triplet_fwd(C.ptr(sd), C.ptr(pd), C.ptr(nd), B, S, alpha, C.ptr(out), C.ptr(hinge), C.stream())
    C.triplet_bwd(C.ptr(sd), C.ptr(pd), C.ptr(nd), C.ptr(hinge), C.ptr(g), B, S, C.ptr(ds), C.ptr(dp), C.ptr(dn), C.stream())
    torch.cuda.synchronize()
    assert torch.equal(hinge.cpu(), active.float())
    if mode == "inactive":
        assert float(lr.detach()) == 0.0 and float(out) == 0.0
        for t in (ds, dp, dn):
            assert torch.equal(t.cpu(), torch.zeros(B, S))
        return
    e = (rel_err(out, lr.detach().reshape(1)), rel_err(ds, sr.grad), rel_err(dp, pr.grad), rel_err(dn, nr.grad))
    print("D triplet B=%d S=%d %s alpha=%g: loss %.2e ds %.2e dp %.2e dn %.2e" % ((B, S, mode, alpha) + e))
    assert max(e) < TOL, e
    off = ~active
    for t in (ds, dp, dn):  # rows behind an inactive hinge carry exactly no gradient
        assert torch.equal(t.cpu()[off], torch.zeros(int(off.sum()), S))


def test_triplet_autograd_function(C):
    """ops.TripletLossFn under autograd with an upstream gradient other than 1, as losses.tripletLoss calls it."""
    from oracle import torch_twin as T
    from srlz import ops
    gen = torch.Generator().manual_seed(9)
    s, p, n, _ = triplet_inputs(257, 16, "mixed", 0.2, gen)
    sr, pr, nr = (t.double().requires_grad_(True) for t in (s, p, n))
    (3.0 * T.triplet_loss(sr, pr, nr, 0.2)).backward()
    sd, pd, nd = (t.to(DEV).requires_grad_(True) for t in (s, p, n))
    (3.0 * ops.TripletLossFn.apply(sd, pd, nd, 0.2)).backward()
    torch.cuda.synchronize()
    e = (rel_err(sd.grad, sr.grad), rel_err(pd.grad, pr.grad), rel_err(nd.grad, nr.grad))
    assert max(e) < TOL, e


# ---------------------------------------------------------------------------------------------------------------------------------
# E. the whole trunk on a state with non-trivial BatchNorm layers
# ---------------------------------------------------------------------------------------------------------------------------------
def randomise_batchnorm(module, seed):
    """Overwrite every BatchNorm2d under `module` (CPU) with bn_affine's recipe, one generator for all of them in module order."""
    gen = torch.Generator().manual_seed(seed)
    count = 0
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                weight, bias, mean, var = bn_affine(m.num_features, gen)
                m.weight.copy_(weight); m.bias.copy_(bias); m.running_mean.copy_(mean); m.running_var.copy_(var)
                count += 1
    return count


def as_fp64(sd):
    return OrderedDict((k, v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in sd.items())


def as_fp32(sd):
    return OrderedDict((k, v.detach().cpu().clone()) for k, v in sd.items())


def build_realistic(seed):
    from test_triplet_gpu import _build
    model = _build()
    assert randomise_batchnorm(model.model.conv_layers, seed) == 20
    return model


def compare_state(after, ref, tag):
    """Every running statistic against the fp64 oracle's (1e-4 of its largest magnitude), every counter exactly."""
    worst = 0.0
    for k, r in ref.items():
        if "running_" in k:
            e = rel_err(after[k], r)
            worst = max(worst, e)
            assert e < TOL, (tag, k, e)
        elif "num_batches_tracked" in k:
            assert int(after[k]) == int(r), (tag, k, int(after[k]), int(r))
    return worst


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("training", [True, False], ids=["train_bn", "eval_bn"])
def test_trunk_with_realistic_batchnorm(C, training, seed):
    from oracle import torch_twin as T
    from srlz import hotpath
    from test_triplet_gpu import _views
    model = build_realistic(seed)
    init = as_fp32(model.state_dict())
    obs, _ = _views(3, 11 + seed)
    x = obs[:, :3].contiguous()

    sd64, sd32 = as_fp64(init), as_fp32(init)
    ref_feat = T.resnet18_features(sd64, x.double(), training)
    feat32 = T.resnet18_features(sd32, x, training)
    e_ref = rel_err(feat32, ref_feat)
    e_ref_run = max(rel_err(sd32[k], sd64[k]) for k in sd64 if "running_" in k)
    ref_emb = T.embedding_forward(as_fp64(init), x.double(), training)

    model = model.to(DEV)
    model.train(training)
    trunk = model.model.conv_layers
    feat = hotpath.resnet18_forward(trunk, x.to(DEV), training)
    torch.cuda.synchronize()
    e_feat = rel_err(feat, ref_feat)
    e_run = compare_state(model.state_dict(), sd64, "trunk")
    for k in sd64:
        if "num_batches_tracked" in k and "conv_layers" in k:
            assert int(sd64[k]) == (1 if training else 0), k
    model.load_state_dict(init)
    emb = model.model(x.to(DEV))
    torch.cuda.synchronize()
    e_emb = rel_err(emb, ref_emb)
    print("E trunk %s seed=%d: features %.2e (fp32 oracle %.2e) running statistics %.2e (fp32 oracle %.2e) embedding %.2e"
          % ("train" if training else "eval", seed, e_feat, e_ref, e_run, e_ref_run, e_emb))
    assert e_ref <= REF_CAP and e_ref_run <= REF_CAP, (e_ref, e_ref_run)
    assert not feat.requires_grad
    assert e_feat < TOL and e_emb < TOL, (e_feat, e_emb)
    if not training:  # getStates = the first view only
        st = model.getStates(obs.to(DEV))
        torch.cuda.synchronize()
        assert rel_err(st, ref_emb) < TOL


@pytest.mark.parametrize("training", [True, False], ids=["train_bn", "eval_bn"])
def test_trunk_three_groups_are_three_calls(C, training):
    """groups = 3 on the realistic state: bit-identical to three separate calls (features, running statistics, counters), and both
    equal to the fp64 oracle called three times in order."""
    from oracle import torch_twin as T
    from srlz import hotpath
    from test_triplet_gpu import _views
    model = build_realistic(3)
    init = as_fp32(model.state_dict())
    obs, _ = _views(2, 29)
    views = [obs[:, 3 * i:3 * i + 3].contiguous() for i in range(3)]
    sd64 = as_fp64(init)
    ref = torch.cat([T.resnet18_features(sd64, v.double(), training) for v in views])

    model = model.to(DEV)
    model.train(training)
    trunk = model.model.conv_layers
    sep = torch.cat([hotpath.resnet18_forward(trunk, v.to(DEV), training) for v in views])
    torch.cuda.synchronize()
    after_sep = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(init)
    one = hotpath.resnet18_forward(trunk, torch.cat(views).to(DEV), training, groups=3)
    torch.cuda.synchronize()
    after_one = model.state_dict()
    assert torch.equal(one, sep)
    for k in init:
        assert torch.equal(after_one[k], after_sep[k]), k
        if "num_batches_tracked" in k and "conv_layers" in k:
            assert int(after_one[k]) == (3 if training else 0), k
    e_feat = rel_err(one, ref)
    e_run = compare_state(after_one, sd64, "groups3")
    print("E trunk groups=3 %s: features %.2e running statistics %.2e" % ("train" if training else "eval", e_feat, e_run))
    assert e_feat < TOL, e_feat


def test_resnet18_weights_file_route(C, tmp_path, monkeypatch):
    """SRLZ_RESNET18_WEIGHTS: a torchvision-keyed resnet18 state dict (with its 1000-class fc) is what the trunk holds, frozen, and
    eval-mode getStates is the fp64 oracle's on that very dict."""
    from models.triplet import ResNet18Trunk
    from oracle import torch_twin as T
    from test_triplet_gpu import _build, _views
    torch.manual_seed(41)
    donor = ResNet18Trunk()
    assert randomise_batchnorm(donor, 4) == 20
    file_sd = as_fp32(donor.state_dict())
    assert tuple(file_sd["fc.weight"].shape) == (1000, 512) and "layer4.1.bn2.running_var" in file_sd
    path = str(tmp_path / "resnet18.pth")
    torch.save(file_sd, path)
    monkeypatch.setenv("SRLZ_RESNET18_WEIGHTS", path)
    model = _build(seed=6)  # another seed: nothing of the donor's can come from the initialisation
    trunk = model.model.conv_layers
    got = trunk.state_dict()
    n_checked = 0
    for k, v in file_sd.items():
        if k.startswith("fc."):
            continue
        assert torch.equal(got[k], v), k
        n_checked += 1
    assert n_checked == 120  # 20 convolutions + 20 BatchNorm layers of 5 tensors
    assert tuple(trunk.fc.weight.shape) == (128, 512)  # the 1000-class layer is replaced by the embedding's
    for name, prm in trunk.named_parameters():
        assert prm.requires_grad == name.startswith("fc."), name
    assert all(prm.requires_grad for prm in model.model.fc.parameters())

    # the oracle's state: the FILE's trunk tensors under the product's key names + the model's own head
    sd = as_fp64(model.state_dict())
    for k, v in file_sd.items():
        if not k.startswith("fc."):
            sd["model.conv_layers." + k] = v.double() if v.is_floating_point() else v.clone()
    obs, _ = _views(3, 17)
    ref = T.get_states(sd, obs.double(), "triplet")
    sd32 = OrderedDict((k, v.float() if v.is_floating_point() else v.clone()) for k, v in sd.items())
    e_ref = rel_err(T.get_states(sd32, obs, "triplet"), ref)
    model = model.to(DEV)
    model.eval()
    with torch.no_grad():
        st = model.getStates(obs.to(DEV))
    torch.cuda.synchronize()
    e = rel_err(st, ref)
    print("E weights file route: getStates %.2e (fp32 oracle %.2e)" % (e, e_ref))
    assert e_ref <= REF_CAP, e_ref
    assert e < TOL, e
    after = model.state_dict()
    for k, v in file_sd.items():  # eval mode: nothing moved
        if not k.startswith("fc."):
            assert torch.equal(after["model.conv_layers." + k].cpu(), v), k


# ---------------------------------------------------------------------------------------------------------------------------------
# F. rejections that must not launch
# ---------------------------------------------------------------------------------------------------------------------------------
BAD_CONVN = {
    "cin192": dict(cin=192),            # a multiple of 64, not a power of two
    "cin1024": dict(cin=1024),
    "cin96": dict(cin=96),
    "cout96": dict(cout=96),
    "k5": dict(ksize=5, pad=2),
    "stride3": dict(stride=3, ho=3, wo=3),
    "k1_stride1": dict(ksize=1, pad=0, stride=1),
    "ho_inconsistent": dict(ho=6),
    "wo_inconsistent": dict(wo=8),
    "n_not_multiple_of_groups": dict(n=4, groups=3),
}


@pytest.mark.parametrize("what", sorted(BAD_CONVN))
def test_convn_refuses(C, what):
    """All four entry points agree on what a srlz_convn_desc may hold; a refused call writes nothing."""
    f = dict(n=4, hi=7, wi=7, ho=7, wo=7, cin=128, cout=128, ksize=3, stride=1, pad=1, groups=1)
    f.update(BAD_CONVN[what])
    d = C.ConvNDesc(f["n"], f["hi"], f["wi"], f["ho"], f["wo"], f["cin"], f["cout"], f["ksize"], f["stride"], f["pad"], f["groups"])
    assert C.convn_packed_floats(d) == 0
    assert C.convn_fwd_tiles(d) == -1
    # buffers sized generously for whatever the descriptor claims
    w = torch.zeros(1024 * 128 * 25, device=DEV)
    pk = nans(16 * 2 * 9 * 4096)
    x = torch.zeros(4 * 7 * 7 * 1024, device=DEV)
    y = nans(4 * 8 * 8 * 128)
    stats = nans(2 * 64 * 128)
    with pytest.raises(C.SrlzError):
        C.convn_pack_weights(C.ptr(w), C.ptr(pk), d, C.stream())
    with pytest.raises(C.SrlzError):
        C.convn_fwd(C.ptr(x), C.ptr(pk), C.ptr(y), C.ptr(stats), None, d, C.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(pk).all()) and bool(torch.isnan(y).all()) and bool(torch.isnan(stats).all())


def test_bn_entry_points_refuse(C):
    ch, chunks = 128, 2
    a, b = torch.zeros(10, ch, device=DEV), torch.zeros(10, ch, device=DEV)
    rec = torch.zeros(3, chunks, 256, device=DEV)
    out = nans(10, ch)
    with pytest.raises(C.SrlzError):  # 10 pixels do not split into 3 groups
        C.bn_add_relu(C.ptr(a), C.ptr(rec), C.ptr(b), None, C.ptr(out), 10, chunks, 3, C.stream())
    with pytest.raises(C.SrlzError):
        C.bn_add_relu(C.ptr(a), None, C.ptr(b), None, C.ptr(out), 9, chunks, 3, C.stream())
    stats = torch.zeros(chunks, 10, 128, device=DEV)
    gamma, beta, rm, rv = (torch.ones(ch, device=DEV) for _ in range(4))
    tick = torch.zeros(1, dtype=torch.int64, device=DEV)
    bnp = nans(3, chunks, 256)
    nbytes = C.bn_finalize_chunks_workspace(chunks, 3)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def finalize(tiles, groups, ws_bytes, n_chunks=chunks):
        C.bn_finalize_chunks(C.ptr(stats), tiles, n_chunks, groups, 50, C.ptr(gamma), C.ptr(beta), EPS, MOMENTUM, C.ptr(rm), C.ptr(rv),
                             C.ptr(tick), C.ptr(bnp), C.ptr(ws), ws_bytes, C.stream())
    with pytest.raises(C.SrlzError):  # 10 tiles do not split into 3 groups
        finalize(10, 3, nbytes)
    with pytest.raises(C.SrlzError):  # a workspace one byte short
        finalize(9, 3, nbytes - 1)
    with pytest.raises(C.SrlzError):
        finalize(0, 1, nbytes)
    with pytest.raises(C.SrlzError):  # more channel blocks than a 512-channel BatchNorm has
        finalize(9, 3, nbytes, n_chunks=9)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(bnp).all()) and int(tick) == 0
    assert bool((rm == 1).all()) and bool((rv == 1).all())
