"""conv1's buffer staging of the image window (csrc/skinny.hip: image_request_buf) against the generic-pointer staging it replaces.

srlz_conv1_fwd(_u8) and srlz_conv1_bwd_weight_fused(_u8) take the buffer staging wherever srlz_conv1_buffer_staging_supported says
so; srlz_debug_conv1_*_generic run the same kernels on the generic staging.  The arithmetic is the same, so every output is compared
with torch.equal: y and the BatchNorm partial records of the forward, dW of the fused weight gradient — on floats and on uint8 frames.
The forward is also held to fp64 F.conv2d at the bar of tests/test_kernels_gpu.py::test_conv1 (2e-5).

Shapes (all C = 3), the smallest at which each path of the new code runs:
  64 x 64, N = 2      2 x 2 tiles per image: every tile is a border tile, no interior request
  96 x 96, N = 2      3 x 3 tiles: exactly one interior tile, surrounded by all eight kinds of border tile
  72 x 88, N = 4      two BatchNorm groups of npg = 2 images (a descriptor's n must be a multiple of its groups, so two groups of two
                      take N = 4, not 3), 36 x 44 map: partial last tile row and column, i.e. dropped epilogue stores and masked
                      statistics
  96 x 96, N = 64     576 tiles, more than the persistent workgroups: a next tile is requested under the MFMA loop, and the "no next
                      tile" branch is taken
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
TOL = 2e-5  # tests/test_kernels_gpu.py::test_conv1

# (himg, wimg, n, groups)
SHAPES = [(64, 64, 2, 1), (96, 96, 2, 1), (72, 88, 4, 2), (96, 96, 64, 1)]
WGRAD_SHAPES = [(96, 96, 2, 1, 1), (72, 88, 4, 2, 1), (96, 96, 2, 1, 0)]  # (+ training)


def ids(c):
    return "x".join(str(v) for v in c)


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    assert torch.cuda.is_available()
    return _cabi


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@functools.lru_cache(maxsize=None)
def inputs(H, W, n):
    """The frames as bytes, the weights, and the normalisation table's host twin — shared by every test of a shape, never modified."""
    rs = np.random.RandomState(H * 3 + W + n)
    u8 = torch.from_numpy(rs.randint(0, 256, (n, 3, H, W)).astype(np.uint8))
    w = torch.from_numpy(rs.randn(64, 3, 7, 7).astype(np.float32) * 0.1)
    return u8, w


@functools.lru_cache(maxsize=None)
def device_inputs(H, W, n):
    from srlz import _cabi as C
    u8, w = inputs(H, W, n)
    st = C.stream()
    u8d, wd = u8.to(DEV), w.to(DEV)
    lut = torch.full((3, 256), NAN, device=DEV)
    C.normalize_lut(C.ptr(lut), st)
    xd = torch.full((n, 3, H, W), NAN, device=DEV)
    C.normalize_u8_planar(C.ptr(u8d), C.ptr(lut), C.ptr(xd), n, 3, H * W, st)
    torch.cuda.synchronize()
    return u8d, wd, lut, xd


@functools.lru_cache(maxsize=None)
def reference(H, W, n):
    """fp64 F.conv2d of the normalised frames, NHWC."""
    _, w = inputs(H, W, n)
    x = device_inputs(H, W, n)[3].cpu()
    return F.conv2d(x.double(), w.double(), None, stride=2, padding=3).permute(0, 2, 3, 1).contiguous()


def desc(C, H, W, n, G):
    hf, wf = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return C.SkinnyDesc(n, 3, H, W, hf, wf, 0, G), hf, wf


@pytest.mark.parametrize("u8", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_forward_matches_generic_staging(C, case, u8):
    H, W, n, G = case
    d, hf, wf = desc(C, H, W, n, G)
    assert C.conv1_buffer_staging_supported(d) == 1
    tiles = C.skinny_tiles(d)
    assert tiles == n * ((hf + 15) // 16) * ((wf + 15) // 16)
    if n == 64:
        assert tiles > C.conv1_workgroups(d)  # a workgroup walks more than one tile
    u8d, wd, lut, xd = device_inputs(H, W, n)
    st = C.stream()
    y, stats = torch.full((n, hf, wf, 64), NAN, device=DEV), torch.full((tiles, 128), NAN, device=DEV)
    yg, sg = torch.full_like(y, NAN), torch.full_like(stats, NAN)
    if u8:
        C.conv1_fwd_u8(C.ptr(u8d), C.ptr(lut), C.ptr(wd), C.ptr(y), C.ptr(stats), d, st)
        C.debug_conv1_fwd_u8_generic(C.ptr(u8d), C.ptr(lut), C.ptr(wd), C.ptr(yg), C.ptr(sg), d, st)
    else:
        C.conv1_fwd(C.ptr(xd), C.ptr(wd), C.ptr(y), C.ptr(stats), d, st)
        C.debug_conv1_fwd_generic(C.ptr(xd), C.ptr(wd), C.ptr(yg), C.ptr(sg), d, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(yg).all()) and bool(torch.isfinite(sg).all())
    assert torch.equal(y, yg)
    assert torch.equal(stats, sg)
    e = rel_err(y, reference(H, W, n))
    print("conv1 forward %r %s: %.1e against fp64" % (case, "uint8" if u8 else "float", e))
    assert e < TOL


@pytest.mark.parametrize("u8", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("case", WGRAD_SHAPES, ids=ids)
def test_fused_weight_gradient_matches_generic_staging(C, case, u8):
    H, W, n, G, training = case
    d, hf, wf = desc(C, H, W, n, G)
    assert C.conv1_buffer_staging_supported(d) == 1
    hp, wp = (hf + 2 - 3) // 2 + 1, (wf + 2 - 3) // 2 + 1
    u8d, wd, lut, xd = device_inputs(H, W, n)
    st = C.stream()
    gen = torch.Generator().manual_seed(H + 7 * W + n)
    y = torch.randn(n, hf, wf, 64, generator=gen).to(DEV)
    bnp = torch.cat([torch.cat([torch.randn(64, generator=gen) * 0.1, torch.rand(64, generator=gen) + 0.5,
                                torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.1]) for _ in range(G)]).to(DEV)
    dpooled = torch.randn(n, hp, wp, 64, generator=gen).to(DEV)
    sums = (torch.randn(128 * G, generator=gen) * 10).to(DEV)
    pd = C.PoolDesc(n, hf, wf, hp, wp, 1, 0, G)
    pooled = torch.full((n, hp, wp, 64), NAN, device=DEV)
    arg = torch.full((n, hp, wp, 64), 0xEE, dtype=torch.uint8, device=DEV)
    C.bn_relu_pool_fwd(C.ptr(y), C.ptr(bnp), C.ptr(pooled), C.ptr(arg), pd, st)
    nb = C.skinny_bwd_weight_workspace(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw, dwg = torch.full((64, 3, 7, 7), NAN, device=DEV), torch.full((64, 3, 7, 7), NAN, device=DEV)
    if u8:
        C.conv1_bwd_weight_fused_u8(C.ptr(u8d), C.ptr(lut), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpooled), C.ptr(sums), training,
                                    C.ptr(dw), C.ptr(ws), nb, d, pd, st)
        C.debug_conv1_bwd_weight_fused_u8_generic(C.ptr(u8d), C.ptr(lut), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpooled), C.ptr(sums),
                                                  training, C.ptr(dwg), C.ptr(ws), nb, d, pd, st)
    else:
        C.conv1_bwd_weight_fused(C.ptr(xd), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpooled), C.ptr(sums), training, C.ptr(dw),
                                 C.ptr(ws), nb, d, pd, st)
        C.debug_conv1_bwd_weight_fused_generic(C.ptr(xd), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpooled), C.ptr(sums), training,
                                               C.ptr(dwg), C.ptr(ws), nb, d, pd, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dwg).all()) and float(dwg.abs().max()) > 0
    assert torch.equal(dw, dwg)
