"""conv64_scatter_pipe_kernel — the persistent, software-pipelined forward of ConvTranspose2d(64, 64, 3, stride 2) (reference
models/models.py:66-78) — against conv64_fwd_kernel<4, false>, bit for bit, in the output AND in the per-tile BatchNorm partials.

The reference kernel is reached without a switch: srlz_conv64_fwd on a few images at a time stays below the route's
tiles-per-group threshold.  A chunk of `c` images whose virtual grid (c * PH * PW positions) is a whole number of 128-position tiles
has exactly the tiles of the whole launch, so its statistics records are the whole launch's records, in place.  The route is asserted
through the host-only predicate before every launch.
"""
import os
import shutil
import sys

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
TM = 128


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    assert torch.cuda.is_available()
    return _cabi


def grid(h, w):
    """Virtual grid of a stride-2 ConvTranspose's forward (csrc/conv64.hip: build_program): one spare row and column."""
    return h + 1, w + 1


def chunk_images(h, w):
    """Fewest images whose grid positions fill whole tiles."""
    ph, pw = grid(h, w)
    c = 1
    while (c * ph * pw) % TM:
        c += 1
    return c


def desc(C, n, h, w, groups=1):
    return C.Conv64Desc(n, h, w, 2 * h + 1, 2 * w + 1, 3, 2, 0, 1, groups)


def smallest_routed(C, h, w, groups=1, limit=4096):
    for n in range(1, limit):
        if C.conv64_scatter_pipe_supported(desc(C, n * groups, h, w, groups), 0):
            return n
    return None


def make_bnp(g, groups, special=False):
    """BatchNorm records [groups][mean | invstd | scale | shift]; the kernels read scale and shift."""
    bnp = torch.randn(groups, 4, 64, generator=g)
    bnp[:, 2] = bnp[:, 2] * 0.5 + 1.0
    if special:
        bnp[:, 3, :] = bnp[:, 3, :].abs() + 0.1  # every shift positive: a row outside the tensor that landed as relu(shift) would show
        bnp[:, 2, 3] = 0.0      # scale 0: relu(shift) everywhere inside the tensor
        bnp[:, 3, 3] = 0.75
        bnp[:, 2, 7] = -1.25    # a negative scale
    return bnp.reshape(groups, 256).contiguous()


def run_whole(C, x, packs, bias, bnp, n, h, w, groups, want_route=1):
    d = desc(C, n, h, w, groups)
    assert C.conv64_scatter_pipe_supported(d, 0) == want_route
    tiles = C.conv64_fwd_tiles(d)
    y = torch.full((n, 2 * h + 1, 2 * w + 1, 64), float("nan"), device=DEV)
    stats = torch.full((tiles, 128), float("nan"), device=DEV)
    C.conv64_fwd(C.ptr(x), C.ptr(packs[0]), C.ptr(bias), C.ptr(y), C.ptr(stats), C.ptr(bnp), d, C.stream())
    torch.cuda.synchronize()
    return y, stats


def run_chunked(C, x, packs, bias, bnp, n, h, w, groups):
    """The same launch as conv64_fwd_kernel's: group by group, chunk_images at a time."""
    ph, pw = grid(h, w)
    c = chunk_images(h, w)
    ng = n // groups
    tpg = (ng * ph * pw + TM - 1) // TM
    y = torch.full((n, 2 * h + 1, 2 * w + 1, 64), float("nan"), device=DEV)
    stats = torch.full((groups * tpg, 128), float("nan"), device=DEV)
    for g in range(groups):
        for i0 in range(0, ng, c):
            m = min(c, ng - i0)
            d = desc(C, m, h, w, 1)
            assert C.conv64_scatter_pipe_supported(d, 0) == 0  # conv64_fwd_kernel
            t0 = g * tpg + i0 * ph * pw // TM
            a = g * ng + i0
            C.conv64_fwd(C.ptr(x[a:a + m]), C.ptr(packs[0]), C.ptr(bias), C.ptr(y[a:a + m]), C.ptr(stats[t0:]),
                         C.ptr(bnp[g]) if bnp is not None else None, d, C.stream())
    torch.cuda.synchronize()
    return y, stats


def inputs(C, seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, 64, generator=g).to(DEV)
    wt = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(DEV)
    bias = torch.randn(64, generator=g).to(DEV)
    packs = torch.empty(2, C.conv64_packed_floats(), device=DEV)
    C.conv64_pack_weights(C.ptr(wt), C.ptr(packs[0]), C.ptr(packs[1]), desc(C, n, h, w), C.stream())
    return g, x, wt, bias, packs


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_identical(C, n, h, w, groups, seed, variants=("fused+bias", "plain"), special=False):
    g, x, wt, bias, packs = inputs(C, seed, n, h, w)
    bnp = make_bnp(g, groups, special).to(DEV)
    out = {}
    for v in variants:
        b, r = (bias, bnp) if v == "fused+bias" else (None, None) if v == "plain" else (None, bnp)
        y, st = run_whole(C, x, packs, b, r, n, h, w, groups)
        yr, sr = run_chunked(C, x, packs, b, r, n, h, w, groups)
        assert not torch.isnan(yr).any() and not torch.isnan(sr).any()
        assert same_bits(y, yr), "%s: output differs in %d elements" % (v, int((y != yr).sum()))
        assert same_bits(st, sr), "%s: statistics differ in %d elements" % (v, int((st != sr).sum()))
        out[v] = y
    return x, wt, bias, bnp, out


@pytest.mark.gpu
def test_prefetch_across_tiles_partial_last_tile_and_xcd_run_ends(C):
    """N = 48 at 55 x 55 -> 111 x 111 in two BatchNorm groups of 24: 2 x 588 = 1176 tiles, more than two per persistent workgroup on
    256 CUs, group boundary inside an XCD's run; with the fused operand and bias, and plain."""
    assert C.conv64_fwd_tiles(desc(C, 48, 55, 55, 2)) == 1176
    check_identical(C, 48, 55, 55, 2, seed=1)


LAYERS = [(27, 27), (13, 13)]  # ConvT3 and ConvT2 of the model (ConvT4 = 55 x 55 above; ConvT1 is below the threshold at any batch
# size the model trains at: test_refusals)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", LAYERS)
def test_layer_shapes_at_the_smallest_routed_batch(C, h, w):
    n = smallest_routed(C, h, w)
    assert n is not None and n > 1
    assert C.conv64_scatter_pipe_supported(desc(C, n - 1, h, w), 0) == 0
    check_identical(C, n, h, w, 1, seed=h)


@pytest.mark.gpu
def test_rectangular_map_and_unaligned_last_group(C):
    """20 x 27 -> 41 x 55, two groups of 57 images: 262 tiles per group (the last one partial), 524 tiles on 512 workgroups — the second
    group starts in the middle of an XCD's run and only some workgroups have a second tile."""
    n = 2 * max(57, smallest_routed(C, 20, 27, 2))
    check_identical(C, n, 20, 27, 2, seed=3)


@pytest.mark.gpu
def test_fused_operand_edge_cases(C):
    """A BatchNorm channel with scale 0, one with a negative scale, every shift positive: the spare row and column of the virtual grid
    and the rows before / behind the tensor must land as zeros, not as relu(shift) — bit for bit against conv64_fwd_kernel and against
    fp64 conv_transpose2d(relu(bn(x)))."""
    h = w = 27
    n = smallest_routed(C, h, w)
    x, wt, bias, bnp, out = check_identical(C, n, h, w, 1, seed=5, variants=("fused+bias", "fused"), special=True)
    sc, sh = bnp[0, 128:192].double().cpu(), bnp[0, 192:256].double().cpu()
    a = torch.relu(x.double().cpu() * sc + sh).permute(0, 3, 1, 2)
    assert float(a[:, 3].min()) == 0.75 and float(a[:, 3].max()) == 0.75
    ref = F.conv_transpose2d(a, wt.double().cpu(), bias.double().cpu(), stride=2).permute(0, 2, 3, 1)
    got = out["fused+bias"].double().cpu()
    assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max())  # fp32 chains of 576 products against fp64


@pytest.mark.gpu
def test_refusals(C):
    """Below the threshold, a gather program, a stride-1 program and every data gradient are refused by the predicate, and
    srlz_conv64_fwd computes them as before (fp64 torch, the tolerance of test_kernels_gpu.py::test_conv64_forward_backward)."""
    n27 = smallest_routed(C, 27, 27)
    assert C.conv64_scatter_pipe_supported(desc(C, n27, 27, 27), 1) == 0  # a data gradient
    assert C.conv64_scatter_pipe_supported(desc(C, 512, 6, 6, 2), 0) == 0  # ConvT1 at the benchmark's batch: 98 tiles per group
    cases = [C.Conv64Desc(8, 27, 27, 55, 55, 3, 2, 0, 1, 1),    # few tiles
             C.Conv64Desc(300, 27, 27, 14, 14, 3, 2, 1, 0, 1),  # gather (conv3)
             C.Conv64Desc(24, 56, 56, 56, 56, 3, 1, 1, 0, 1)]   # stride 1 (conv2)
    for d in cases:
        assert C.conv64_scatter_pipe_supported(d, 0) == 0 and C.conv64_scatter_pipe_supported(d, 1) == 0
        g = torch.Generator().manual_seed(d.n)
        x = torch.randn(d.n, 64, d.hi, d.wi, generator=g)
        wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05
        packs = torch.empty(2, C.conv64_packed_floats(), device=DEV)
        C.conv64_pack_weights(C.ptr(wt.to(DEV)), C.ptr(packs[0]), C.ptr(packs[1]), d, C.stream())
        y = torch.full((d.n, d.ho, d.wo, 64), float("nan"), device=DEV)
        stats = torch.empty(C.conv64_fwd_tiles(d), 128, device=DEV)
        C.conv64_fwd(C.ptr(x.permute(0, 2, 3, 1).contiguous().to(DEV)), C.ptr(packs[0]), None, C.ptr(y), C.ptr(stats), None, d, C.stream())
        torch.cuda.synchronize()
        ref = (F.conv_transpose2d(x.double(), wt.double(), None, stride=d.stride, padding=d.pad) if d.transposed else
               F.conv2d(x.double(), wt.double(), None, stride=d.stride, padding=d.pad)).permute(0, 2, 3, 1)
        assert float((y.double().cpu() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())


def test_isa_audit_scatter_pipe_kernel():
    """No spills (a scratch reload is a vector-memory load: waiting for it drains the prefetched rows) and no serialised stores in
    either instantiation; a whole tile's MFMAs unrolled (9 taps x 64)."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import isa_audit
    if not os.path.exists(isa_audit.HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    ks = list(isa_audit.kernels(isa_audit.disassemble(os.path.join(isa_audit.CSRC, "conv64_pipe.hip"))))
    names = isa_audit.demangle([k for k, _ in ks])
    seen = 0
    for (_, body), name in zip(ks, names):
        if not name.startswith("conv64_scatter_pipe_kernel"):
            continue
        seen += 1
        a = isa_audit.audit(body)
        assert a["store_wait_chain"] < 2, name
        assert a["scratch_reloads"] == 0, name
        assert not any(t.startswith("scratch_") for t in body), name
        assert a["mfma"] == 576, name
        # every store is a 16-byte buffer store without a branch of its own: 4 flushes x 8
        assert sum(t.startswith("buffer_store_dwordx4") for t in body) == 32, name
    assert seen == 2
