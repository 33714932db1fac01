"""The persistent kernels of the training step PAST their first tile, chunk or job per workgroup.

Their grids are capped at one or two workgroups per CU and a workgroup carries state from one tile to the next — prefetched rows, an
LDS ring of source rows, tile-parity double buffers, accumulators, the BatchNorm group of the tile.  At the few images of the other
kernel-level tests every workgroup has exactly one tile, and the loop body behind the first iteration never runs.

Every case here finds its batch size by SEARCHING through the host-only queries of the C ABI (the plan of the weight gradient, the
tile and workgroup counts of the other kernels) and asserts the regime before it launches, so a device with another CU count still
tests the steady state.  Small maps, many images: the regime depends on grid positions, not on the image size.

Where the arithmetic allows it the comparison is EXACT: small integers (and halves) as inputs make every product and every partial
sum exact in fp32 in any order, so the result must equal the host's fp64 result bit for bit — the device of the integer-exact cases
of tests/test_linear_kernels_gpu.py.  The test asserts the property of the inputs that makes this so (sum |a| |b| < 2^24 granules).
Everything else keeps the bound of the kernel-level test of the same entry point in tests/test_kernels_gpu.py.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from fused_block_util import whole_block_backward, rel_err, nhwc, nchw

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = float(1 << 24)  # integers up to here are fp32 numbers
PARTIAL_BYTES = (9 * 64 * 64 + 64) * 4  # a workgroup's weight-gradient partial (nine taps of 64 x 64, the bias sums)
RING_S2, RING, GATHER, CHUNK = 0, 1, 2, 3
NAMES = ("ring_s2", "ring", "gather", "chunk")


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    assert torch.cuda.is_available()
    return _cabi


def out_size(hi, s, p, t):
    return (hi - 1) * s - 2 * p + 3 if t else (hi + 2 * p - 3) // s + 1


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# a) srlz_conv64_bwd_weight: the four routes
# ---------------------------------------------------------------------------------------------------------------------------------
def desc64(C, n, shape, groups):
    hi, wi, s, p, t = shape
    return C.Conv64Desc(n, hi, wi, out_size(hi, s, p, t), out_size(wi, s, p, t), 3, s, p, t, groups)


def wgrad_plan(C, d, has_x_bnp, has_dy_bn):
    """The plan srlz_conv64_bwd_weight launches from, with what follows from it: chunks per BatchNorm group (nch), workgroups per
    group launched (wpg) and available (gpg: the workspace holds one partial per workgroup of the whole grid)."""
    out = (ctypes.c_int * 4)()
    C.conv64_bwd_weight_plan(d, has_x_bnp, has_dy_bn, out)
    route, wgs, cpw, tk = out
    prog = (ctypes.c_int * 64)()
    assert C.conv64_debug_program(d, 0, prog, 64) > 0
    G = max(d.groups, 1)
    nch = (prog[0] * prog[1] * prog[2] + tk - 1) // tk  # images per group x PH x PW grid positions
    return {"route": route, "wgs": wgs, "cpw": cpw, "tk": tk, "nch": nch, "G": G, "wpg": wgs // G,
            "gpg": C.conv64_bwd_weight_workspace(d) // PARTIAL_BYTES // G, "positions": G * nch * tk}


def ragged(pl):
    """Not every workgroup takes the same number of chunks."""
    if pl["route"] in (RING_S2, RING):  # contiguous ranges: the group's last workgroup takes what is left, and some stay away
        return pl["nch"] % pl["cpw"] != 0 and pl["wpg"] < pl["gpg"]
    return (pl["nch"] * pl["G"]) % pl["wgs"] != 0  # strided over the grid


REGIMES = {
    "two chunks, ragged": lambda pl: pl["cpw"] == 2 and ragged(pl),
    # (the stride-2 ring walks chunks of 32 positions on a grid sized for chunks of 64: two per workgroup is its smallest launch, and
    # then on every workgroup of the grid — its first ragged launch has three)
    "three chunks, ragged": lambda pl: pl["cpw"] == 3 and ragged(pl),
    "five or more": lambda pl: pl["cpw"] >= 5,  # (the rings: 64 new rows per chunk into 246, or 184 at stride 2 — every slot rewritten by then)
    "steady": lambda pl: pl["cpw"] >= 2 and ragged(pl),
}


def search_wgrad(C, shape, groups, has_x_bnp, has_dy_bn, regime, limit=8192):
    for per in range(1, limit):
        d = desc64(C, per * groups, shape, groups)
        pl = wgrad_plan(C, d, has_x_bnp, has_dy_bn)
        if REGIMES[regime](pl):
            return d, pl
    raise AssertionError("no batch size below %d reaches '%s' on %r" % (limit, regime, shape))


def exact_bnp(g, groups):
    """BatchNorm records [groups][mean | invstd | scale | shift] whose fused operand relu(x * scale + shift) is exact in halves on
    integer x: every shift positive (a row outside the tensor that landed as relu(shift) would show), a zero scale, negative scales."""
    rec = torch.zeros(groups, 4, 64)
    rec[:, 1] = 1.0
    rec[:, 2] = torch.tensor([1.0, -1.0, 0.5, 2.0, 0.0])[torch.randint(0, 5, (groups, 64), generator=g)]
    rec[:, 3] = torch.randint(1, 5, (groups, 64), generator=g).float() * 0.5
    rec[:, 2, 3], rec[:, 3, 3] = 0.0, 1.5
    rec[:, 2, 7] = -1.0
    return rec.reshape(groups, 256).contiguous()


def wgrad_host(a, dy, shape):
    """fp64 weight gradient of the layer (reference layout: conv [co][ci][3][3], transposed [ci][co][3][3]); a, dy NCHW fp64."""
    _, _, s, p, t = shape
    w = torch.zeros(64, 64, 3, 3, dtype=torch.float64)
    return torch.ops.aten.convolution_backward(dy, a, w, None, [s, s], [p, p], [1, 1], bool(t), [0, 0], 1, [False, True, False])[1]


def launch_wgrad(C, d, x, dy, bnp, op=None):
    nbytes = C.conv64_bwd_weight_workspace(d)
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    dw = torch.full((64, 64, 3, 3), float("nan"), device=DEV)
    db = torch.full((64,), float("nan"), device=DEV)
    C.conv64_bwd_weight(C.ptr(x), C.ptr(dy), C.ptr(dw), C.ptr(db), C.ptr(bnp), op, C.ptr(ws), nbytes, d, C.stream())
    torch.cuda.synchronize()
    return dw, db


SQUARE = {RING: (9, 9, 1, 1, 0), RING_S2: (6, 6, 2, 0, 1), GATHER: (10, 10, 2, 1, 0), CHUNK: (9, 80, 1, 1, 0)}
RECT = {RING: (7, 12, 1, 1, 0), RING_S2: (4, 6, 2, 0, 1), GATHER: (8, 21, 2, 0, 0), CHUNK: (6, 75, 1, 1, 0)}
FIRST_RAGGED = {RING: "two chunks, ragged", RING_S2: "three chunks, ragged", GATHER: "two chunks, ragged", CHUNK: "two chunks, ragged"}
# (route, shape, groups, fused x_bnp, regime)
EXACT_CASES = []
for _r in (RING_S2, RING, GATHER, CHUNK):
    EXACT_CASES += [(_r, SQUARE[_r], 1, 0, FIRST_RAGGED[_r]), (_r, SQUARE[_r], 2, 0, "five or more"), (_r, RECT[_r], 2, 0, "steady")]
for _r in (RING_S2, RING):
    EXACT_CASES += [(_r, SQUARE[_r], 2, 1, "five or more"), (_r, RECT[_r], 1, 1, FIRST_RAGGED[_r])]
# the gather kernel has no fused operand: with x_bnp its shapes go to the chunk-at-a-time kernel (the stride-2 instantiation)
EXACT_CASES += [(CHUNK, SQUARE[GATHER], 2, 1, "five or more"), (CHUNK, RECT[GATHER], 1, 1, "two chunks, ragged")]


@pytest.mark.parametrize("route,shape,groups,fused,regime", EXACT_CASES,
                         ids=["%s-%dx%d-g%d-%s-%s" % (NAMES[c[0]], c[1][0], c[1][1], c[2], "bnp" if c[3] else "plain", c[4].split(",")[0].replace(" ", "_"))
                              for c in EXACT_CASES])
def test_conv64_weight_gradient_routes_integer_exact(C, route, shape, groups, fused, regime):
    """x holds integers in [-4, 4], dy integers in [-2, 2], the fused operand has scales in {1, -1, 0.5, 2, 0} and shifts in halves:
    dw and db equal the fp64 result bit for bit, whichever workgroup summed which chunk in which order, and twice in a row."""
    d, pl = search_wgrad(C, shape, groups, fused, 0, regime)
    assert pl["route"] == route, "%r runs as %s" % (shape, NAMES[pl["route"]])
    if fused and shape in (SQUARE[GATHER], RECT[GATHER]):
        assert wgrad_plan(C, d, 0, 0)["route"] == GATHER  # (the same launch without x_bnp is the gather kernel's)
    print("%s %r groups %d: n = %d, %d chunks of %d per group on %d of %d workgroups, %d per workgroup, %d positions"
          % (NAMES[route], shape, groups, d.n, pl["nch"], pl["tk"], pl["wpg"], pl["gpg"], pl["cpw"], pl["positions"]))
    assert REGIMES[regime](pl) and pl["positions"] <= 300000
    g = torch.Generator().manual_seed(1000 * route + 10 * shape[0] + groups + fused)
    x = ints(g, (d.n, 64, d.hi, d.wi), -4, 4)
    dy = ints(g, (d.n, 64, d.ho, d.wo), -2, 2)
    bnp = exact_bnp(g, groups) if fused else None
    a = x.double()
    if fused:
        rec = bnp.view(groups, 4, 64).double()
        a = torch.relu(a.view(groups, -1, 64, d.hi, d.wi) * rec[:, 2].view(groups, 1, 64, 1, 1) + rec[:, 3].view(groups, 1, 64, 1, 1))
        a = a.view(d.n, 64, d.hi, d.wi)
        assert float(a[:, 3].min()) == 1.5 and float(a[:, 3].max()) == 1.5
    granule = 0.5 if fused else 1.0
    # exactness is a property of the inputs: no partial sum of any output element, in any order, leaves the fp32 integers
    bound = float(wgrad_host(a.abs(), dy.double().abs(), shape).max()) / granule
    assert bound < EXACT and float(dy.abs().sum((0, 2, 3)).max()) < EXACT, bound
    ref_dw, ref_db = wgrad_host(a, dy.double(), shape), dy.double().sum((0, 2, 3))
    xd, dyd = nhwc(x).to(DEV), nhwc(dy).to(DEV)
    bd = bnp.to(DEV) if fused else None
    dw, db = launch_wgrad(C, d, xd, dyd, bd)
    wrong = int((dw.double().cpu() != ref_dw).sum())
    assert wrong == 0, "%d of 36864 weight-gradient elements differ, worst by %g (bound %g granules)" % (
        wrong, float((dw.double().cpu() - ref_dw).abs().max()), bound)
    assert torch.equal(db.double().cpu(), ref_db)
    dw2, db2 = launch_wgrad(C, d, xd, dyd, bd)
    assert same_bits(dw2, dw) and same_bits(db2, db)


@pytest.mark.parametrize("shape,training", [((13, 13, 2, 0, 1), 1), ((9, 9, 1, 1, 0), 0)])
def test_conv64_weight_gradient_chunk_route_with_the_rebuilt_gradient(C, shape, training):
    """dy_bn: the gradient is rebuilt from (dA, y) while the chunk is staged, which only the chunk-at-a-time kernel does (both of its
    instantiations here), in two BatchNorm groups with five or more chunks per workgroup.  Not exact — compared with the fp64 weight
    gradient of the fp64 rebuilt gradient at the 5e-5 of test_kernels_gpu.py::test_fused_bn_backward_operand.  The ReLU decisions are
    kept out of the comparison by construction: y, scale and shift are dyadic, so bn(y) is exact in fp32 and never 0."""
    groups = 2
    assert wgrad_plan(C, desc64(C, 64, shape, groups), 0, 0)["route"] != CHUNK  # (without dy_bn a ring kernel takes these shapes)
    d, pl = search_wgrad(C, shape, groups, 0, 1, "five or more")
    assert pl["route"] == CHUNK and pl["cpw"] >= 5 and pl["positions"] <= 300000
    per, count = d.n // groups, (d.n // groups) * d.ho * d.wo
    g = torch.Generator().manual_seed(31 + shape[0])
    x = torch.randn(d.n, 64, d.hi, d.wi, generator=g)
    da = torch.randn(d.n, 64, d.ho, d.wo, generator=g)
    y = ints(g, (d.n, 64, d.ho, d.wo), -8, 8) / 4
    rec = torch.empty(groups, 4, 64)
    rec[:, 0], rec[:, 1] = torch.randn(groups, 64, generator=g) * 0.1, torch.rand(groups, 64, generator=g) + 0.5
    rec[:, 2] = torch.tensor([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5])[torch.randint(0, 6, (groups, 64), generator=g)]
    rec[:, 3] = (2 * torch.randint(-8, 8, (groups, 64), generator=g).float() + 1) / 16  # odd sixteenths: y * scale is an even number of them
    sums = torch.randn(groups, 128, generator=g) * count ** 0.5
    r64, s64 = rec.double(), sums.double()

    def col(v):
        return v.view(groups, 1, 64, 1, 1)
    y5, da5 = y.double().view(groups, per, 64, d.ho, d.wo), da.double().view(groups, per, 64, d.ho, d.wo)
    z = y5 * col(r64[:, 2]) + col(r64[:, 3])
    assert float(z.abs().min()) >= 1.0 / 16
    dy = col(r64[:, 2]) * da5 * (z > 0)
    if training:  # include/srlz.h: scale * (dA [bn(y) > 0] - sums[c] / count - xhat sums[64 + c] / count)
        dy = dy - col(r64[:, 2]) * (col(s64[:, :64]) / count + (y5 - col(r64[:, 0])) * col(r64[:, 1]) * col(s64[:, 64:]) / count)
    dy = dy.view(d.n, 64, d.ho, d.wo)
    ref_dw, ref_db = wgrad_host(x.double(), dy, shape), dy.sum((0, 2, 3))
    xd, dad, yd, recd, sumd = nhwc(x).to(DEV), nhwc(da).to(DEV), nhwc(y).to(DEV), rec.reshape(-1).to(DEV), sums.reshape(-1).to(DEV)
    op = C.BnBwdOperand(yd.data_ptr(), recd.data_ptr(), sumd.data_ptr(), count, training, None)
    dw, db = launch_wgrad(C, d, xd, dad, None, op)
    e_dw, e_db = rel_err(dw, ref_dw), rel_err(db, ref_db)
    print("chunk route with dy_bn %r training %d: n = %d, cpw %d; dw %.2e db %.2e" % (shape, training, d.n, pl["cpw"], e_dw, e_db))
    assert e_dw < 5e-5 and e_db < 5e-5
    dw2, db2 = launch_wgrad(C, d, xd, dad, None, op)
    assert same_bits(dw2, dw) and same_bits(db2, db)


# ---------------------------------------------------------------------------------------------------------------------------------
# b) srlz_conv64_bwd_fused: several tiles per workgroup, a BatchNorm group boundary inside a workgroup's walk
# ---------------------------------------------------------------------------------------------------------------------------------
def fused_regime(C, d):
    """(tiles, workgroups, tiles per group, positions per group) and whether this batch is the regime asked for."""
    G = max(d.groups, 1)
    tiles, grid = C.conv64_bwd_data_tiles(d), C.conv64_bwd_fused_workgroups(d)
    prog = (ctypes.c_int * 64)()
    assert C.conv64_debug_program(d, 1, prog, 64) > 0
    q = prog[0] * prog[1] * prog[2]  # grid positions of one BatchNorm group; a tile is 128 of them
    tpg = tiles // G
    ok = (C.conv64_bwd_fused_supported(d) == 1 and tiles >= 2 * grid + 8 and tiles % 8 != 0 and q % 128 != 0 and tiles == G * tpg
          and tpg % (grid // 8) != 0)
    return ok, (tiles, grid, tpg, q)


@pytest.mark.parametrize("hi,training,zero_gamma", [(13, 1, False), (13, 0, False), (6, 1, True)])
def test_conv64_bwd_fused_beyond_one_tile_per_workgroup(C, hi, training, zero_gamma):
    """Two BatchNorm groups, at least two tiles and a piece for every workgroup: the cross-tile prefetch, the row-info double buffer,
    the next tile's first weight slab behind the closing barrier, the XCD run ends (tiles % 8 != 0), a partial last tile per group,
    consecutive tiles of one workgroup in different groups (tiles per group no multiple of the run length), weight-gradient and
    bias accumulators carried over tiles.  Every check of test_conv64_bwd_fused_whole_block_backward (dx bit for bit against the
    two-launch path; dx, dw, db against fp64 autograd at 1e-4), and both BatchNorm-backward sums of the input's BatchNorm against
    fp64 at the same 1e-4."""
    groups, ho = 2, 2 * hi + 1
    for per in range(1, 8192):
        d = C.Conv64Desc(per * groups, hi, hi, ho, ho, 3, 2, 0, 1, groups)
        ok, info = fused_regime(C, d)
        if ok:
            break
    else:
        raise AssertionError("no batch size reaches the steady state")
    print("bwd_fused %dx%d: n = %d, %d tiles on %d workgroups, %d per group of %d positions" % ((hi, hi, d.n) + info))

    def regime(dd):
        assert (dd.n, dd.hi, dd.groups) == (d.n, hi, groups) and fused_regime(C, dd)[0]
    r = whole_block_backward(C, d.n, hi, groups, training, zero_gamma, regime=regime)
    # the two sums of the BatchNorm + ReLU that produced the layer's input, sum dA [bn(x) > 0] and sum dA [bn(x) > 0] xhat, in fp64
    per = d.n // groups
    want = []
    for gi in range(groups):
        xs, dA = r["x"][gi * per:(gi + 1) * per].double(), r["dx_ref"][gi * per:(gi + 1) * per]
        sc, sh = r["recs64"][gi]
        mean, inv = r["xrecs"][gi][:64].double().view(1, 64, 1, 1), r["xrecs"][gi][64:128].double().view(1, 64, 1, 1)
        dz = dA * ((xs * sc + sh) > 0)
        want.append(torch.cat((dz.sum((0, 2, 3)), (dz * (xs - mean) * inv).sum((0, 2, 3)))))
    want = torch.stack(want)
    got = r["sums"].view(groups, 128).double().cpu()
    errs = [float((got[:, k:k + 64] - want[:, k:k + 64]).abs().max() / want[:, k:k + 64].abs().max()) for k in (0, 64)]
    print("bwd_fused %dx%d: BatchNorm-backward sums against fp64: %.2e %.2e; dw %.2e" % (hi, hi, errs[0], errs[1], rel_err(r["dw"], r["dw_ref"])))
    assert max(errs) < 1e-4, errs


# ---------------------------------------------------------------------------------------------------------------------------------
# c) conv1: skinny_conv_kernel<7, 3> and skinny_wgrad_kernel<7, 3> prefetching the next tile under the current one
# ---------------------------------------------------------------------------------------------------------------------------------
H1, HF1 = 64, 32  # a 64 x 64 image: a 32 x 32 map, four tiles of 16 x 16


def search_conv1(C, c, groups=2, spare=3):
    for per in range(1, 8192):
        d = C.SkinnyDesc(per * groups, c, H1, H1, HF1, HF1, 0, groups)
        tiles, grid = C.skinny_tiles(d), C.conv1_workgroups(d)
        if tiles >= 2 * grid + spare:
            assert tiles == 4 * d.n and 0 < grid < tiles
            return d, tiles, grid
    raise AssertionError("no batch size reaches the steady state")


@pytest.fixture(scope="module", params=[3, 6])
def conv1_exact(request, C):
    """Integer images and weights in {-1, 0, 1}, integer gradients in [-2, 2]; the fp64 results, computed once."""
    c = request.param
    d, tiles, grid = search_conv1(C, c)
    print("conv1 C = %d: n = %d, %d tiles on %d workgroups" % (c, d.n, tiles, grid))
    g = torch.Generator().manual_seed(40 + c)
    x, w = ints(g, (d.n, c, H1, H1), -1, 1), ints(g, (64, c, 7, 7), -1, 1)
    dy = ints(g, (d.n, 64, HF1, HF1), -2, 2)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, stride=2, padding=3)
    yr.backward(dy.double())
    return {"d": d, "c": c, "x": x, "w": w, "dy": dy, "y": yr.detach(), "dx": xr.grad, "dw": wr.grad}


def tile_sums(y_nchw):
    """[tiles][sum | sum of squares] per 16 x 16 tile of a 32 x 32 map, tiles in (image, tile row, tile column) order."""
    n = y_nchw.shape[0]
    t = y_nchw.permute(0, 2, 3, 1).reshape(n, 2, 16, 2, 16, 64)
    return torch.cat((t.sum((2, 4)), (t * t).sum((2, 4))), dim=-1).reshape(n * 4, 128)


def test_conv1_forward_integer_exact_float_and_byte_frames(C, conv1_exact):
    """y and the per-tile statistics records equal the host's; the uint8 + table form of the same launch (its table holding the
    integers -1, 0, 1 and, separately, the loader's normalisation) gives the float form's bits."""
    from srlz import ops
    e = conv1_exact
    d, c = e["d"], e["c"]
    ref_stats = tile_sums(e["y"])
    assert float(ref_stats.abs().max()) < EXACT  # the sums of a tile stay fp32 integers in any order
    xd, wd = e["x"].to(DEV), e["w"].to(DEV)

    def fwd(img, lut, w):
        y = torch.full((d.n, HF1, HF1, 64), float("nan"), device=DEV)
        stats = torch.full((C.skinny_tiles(d), 128), float("nan"), device=DEV)
        if lut is None:
            C.conv1_fwd(C.ptr(img), C.ptr(w), C.ptr(y), C.ptr(stats), d, C.stream())
        else:
            C.conv1_fwd_u8(C.ptr(img), C.ptr(lut), C.ptr(w), C.ptr(y), C.ptr(stats), d, C.stream())
        torch.cuda.synchronize()
        return y, stats
    y, stats = fwd(xd, None, wd)
    assert torch.equal(nchw(y).double().cpu(), e["y"]) and torch.equal(stats.double().cpu(), ref_stats)
    # bytes 0, 1, 2 through a table that maps them to -1, 0, 1: the same integers
    lut = torch.zeros(3, 256, device=DEV)
    lut[:, 1], lut[:, 0] = 0.0, -1.0
    lut[:, 2] = 1.0
    x8 = (e["x"] + 1).to(torch.uint8).to(DEV)
    y8, stats8 = fwd(x8, lut, wd)
    assert same_bits(y8, y) and same_bits(stats8, stats)
    # random bytes through the loader's normalisation and random weights: bit for bit against the float form (test_u8_frames_gpu.py)
    g = torch.Generator().manual_seed(7 + c)
    f8 = torch.randint(0, 256, (d.n, c, H1, H1), generator=g).to(torch.uint8).to(DEV)
    wf = (torch.randn(64, c, 7, 7, generator=g) * 0.1).to(DEV)
    ya, sa = fwd(ops.frames_as_float(f8), None, wf)
    yb, sb = fwd(f8, ops.norm_lut(torch.device(DEV, torch.cuda.current_device())), wf)
    assert torch.isfinite(ya).all() and torch.isfinite(sa).all() and same_bits(yb, ya) and same_bits(sb, sa)


def test_conv1_weight_and_data_gradient_integer_exact(C, conv1_exact):
    e = conv1_exact
    d, c = e["d"], e["c"]
    # no sum of |x| |dy| over the positions, hence no partial sum in any order, leaves the fp32 integers
    assert d.n * HF1 * HF1 * float(e["x"].abs().max()) * float(e["dy"].abs().max()) < EXACT and float(e["dw"].abs().max()) > 0
    xd, wd, dyd = e["x"].to(DEV), e["w"].to(DEV), nhwc(e["dy"]).to(DEV)
    nbytes = C.skinny_bwd_weight_workspace(d)
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
        dw = torch.full((64, c, 7, 7), float("nan"), device=DEV)
        C.conv1_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw), C.ptr(ws), nbytes, d, C.stream())
        dx = torch.full((d.n, c, H1, H1), float("nan"), device=DEV)
        C.conv1_bwd_data(C.ptr(dyd), C.ptr(wd), C.ptr(dx), d, C.stream())
        torch.cuda.synchronize()
        outs.append((dw, dx))
    assert torch.equal(outs[0][0].double().cpu(), e["dw"])
    assert torch.equal(outs[0][1].double().cpu(), e["dx"])
    assert same_bits(outs[1][0], outs[0][0]) and same_bits(outs[1][1], outs[0][1])


@pytest.mark.parametrize("c", [3, 6])
def test_conv1_pool_fused_weight_gradient_in_the_steady_state(C, c):
    """skinny_wgrad_kernel<7, 3, true>, the variant the step runs: conv1 -> BatchNorm (training, two groups) -> ReLU -> MaxPool(3, 2, 1)
    through ops.EncInFn against fp64 autograd at the 5e-5 of test_kernels_gpu.py::test_encoder_input_block_fused_backward.  At this
    many elements two correct evaluations do disagree on a few ReLU and arg-max decisions, so the incoming gradient is zeroed where
    the fp64 evaluation is within 1e-4 of a tie (the winner against the runner-up of its window, or against 0): there either decision
    multiplies a zero."""
    from srlz import ops
    groups = 2
    d, tiles, grid = search_conv1(C, c, groups)
    n, per = d.n, d.n // groups
    g = torch.Generator().manual_seed(7 * c + 1)
    x = torch.randn(n, c, H1, H1, generator=g)
    w = torch.randn(64, c, 7, 7, generator=g) * 0.1
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    hp = (HF1 + 2 - 3) // 2 + 1
    dp = torch.randn(n, 64, hp, hp, generator=g)
    wr, gr, br = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    yr = F.conv2d(x.double(), wr, None, stride=2, padding=3)
    zr = torch.cat([F.batch_norm(yr[gi * per:(gi + 1) * per], None, None, gr, br, True, 0.1, 1e-5) for gi in range(groups)])
    pr = F.max_pool2d(F.relu(zr), 3, 2, 1)
    with torch.no_grad():  # the winner of every window against its runner-up and against the ReLU's threshold
        gaps = []
        for gi in range(groups):
            win = F.unfold(F.relu(zr[gi * per:(gi + 1) * per]).reshape(-1, 1, HF1, HF1), 3, padding=1, stride=2)  # [images x 64, 9, windows]
            top = win.topk(2, dim=1).values
            gaps.append((top[:, 0] - top[:, 1]).view(per, 64, hp, hp))
        zmax = F.max_pool2d(zr, 3, 2, 1)
        tie = (zmax.abs() < 1e-4) | ((zmax > 0) & (torch.cat(gaps) < 1e-4))
        dp = torch.where(tie, torch.zeros(()), dp)
    print("conv1 pool-fused wgrad C = %d: n = %d, %d tiles on %d workgroups, %d of %d pooled gradients zeroed at ties"
          % (c, n, tiles, grid, int(tie.sum()), tie.numel()))
    pr.backward(dp.double())
    xd = x.to(DEV)
    wd, gd, bd = (t.to(DEV).requires_grad_(True) for t in (w, gamma, beta))
    rmd, rvd = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    with ops.batch_groups(groups):
        pooled, y = ops.EncInFn.apply(xd, wd, gd, bd, rmd, rvd, True, 1, None)
        assert rel_err(nchw(y), yr) < 2e-5 and rel_err(nchw(pooled), pr) < 2e-5
        pooled.backward(nhwc(dp).to(DEV))
    torch.cuda.synchronize()
    errs = rel_err(wd.grad, wr.grad), rel_err(gd.grad, gr.grad), rel_err(bd.grad, br.grad)
    print("conv1 pool-fused wgrad C = %d: dw %.2e dgamma %.2e dbeta %.2e" % ((c,) + errs))
    assert max(errs) < 5e-5, errs


# ---------------------------------------------------------------------------------------------------------------------------------
# d) the last ConvTranspose, output-stationary: waves that take a second job next to waves that do not
# ---------------------------------------------------------------------------------------------------------------------------------
OS_CASES = [(3, 5, 37), (6, 57, 5)]  # (C, hf, wf): three strips of 16 columns; three strips of 28 rows


def search_os(C, c, hf, wf, groups=2):
    himg, wimg = 2 * hf + 2, 2 * wf + 2
    for per in range(1, 8192):
        d = C.SkinnyDesc(per * groups, c, himg, wimg, hf, wf, 1, groups)
        plans = []
        for backward in (0, 1):
            out = (ctypes.c_int * 2)()
            C.convT_out_os_plan(d, backward, out)
            plans.append((out[0], out[1]))
        # a second job for some waves of a workgroup and not for the others, forward and backward
        if all(jobs > 4 * grid + 4 and jobs % 4 != 0 for jobs, grid in plans):
            return d, plans
    raise AssertionError("no batch size reaches the steady state")


def os_inputs(C, c, hf, wf, seed, image=(1.3, 0.2)):
    """image: (spread, mean) of the image-side tensor — a target of the loss, or a gradient (zero mean, as a gradient of the step is:
    the bound on the bias gradient below is a few ulps of a sum of zero-mean terms)."""
    d, plans = search_os(C, c, hf, wf)
    print("convT_out C = %d %dx%d: n = %d, forward %d jobs on %d workgroups, backward %d on %d" % ((c, hf, wf, d.n) + plans[0] + plans[1]))
    g = torch.Generator().manual_seed(seed)
    n, groups = d.n, 2
    x = (torch.randn(n, hf, wf, 64, generator=g) * 1.2 + 0.1).to(DEV)
    w = (torch.randn(64, c, 4, 4, generator=g) * 0.1).to(DEV)
    b = torch.randn(c, generator=g).to(DEV)
    img = (torch.randn(n, c, d.himg, d.wimg, generator=g) * image[0] + image[1]).to(DEV)
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    recs = []
    for gi in range(groups):
        xg = x[gi * (n // groups):(gi + 1) * (n // groups)].double().cpu()
        m, v = xg.mean((0, 1, 2)), xg.var((0, 1, 2), unbiased=False)
        inv = 1.0 / torch.sqrt(v + 1e-5)
        recs.append(torch.cat((m, inv, gamma.double() * inv, beta.double() - m * gamma.double() * inv)).float())
    xs = nchw(x).double().cpu()
    half = n // groups
    act = torch.cat([torch.relu(xs[gi * half:(gi + 1) * half] * recs[gi][128:192].double().view(1, 64, 1, 1) +
                                recs[gi][192:].double().view(1, 64, 1, 1)) for gi in range(groups)])
    return d, x, w, b, img, torch.cat(recs).to(DEV), act


@pytest.mark.parametrize("c,hf,wf", OS_CASES)
def test_convT_out_forward_with_and_without_the_loss_beyond_one_job_per_wave(C, c, hf, wf):
    """srlz_convT_out_fwd against fp64 at test_convT_out's 2e-5, and srlz_convT_out_fwd_loss as in
    test_convT_out_forward_with_the_loss_in_its_epilogue: the error is dec - target and the reconstruction srlz_convT_out_fwd's bit
    for bit, with or without the reconstruction stored; the per-frame loss sums against fp64 at 1e-5."""
    d, x, w, b, tgt, bnp, act = os_inputs(C, c, hf, wf, 5 * hf + c)
    st = C.stream()
    dec0 = torch.full((d.n, c, d.himg, d.wimg), float("nan"), device=DEV)
    C.convT_out_fwd(C.ptr(x), C.ptr(w), C.ptr(b), C.ptr(dec0), C.ptr(bnp), d, st)
    err, dec1, err2 = (torch.full_like(dec0, float("nan")) for _ in range(3))
    nwg = C.convT_out_fwd_loss_workgroups(d)
    part, part2 = (torch.full((2 * nwg,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    C.convT_out_fwd_loss(C.ptr(x), C.ptr(w), C.ptr(b), C.ptr(tgt), C.ptr(err), C.ptr(dec1), C.ptr(bnp), C.ptr(part), d, st)
    C.convT_out_fwd_loss(C.ptr(x), C.ptr(w), C.ptr(b), C.ptr(tgt), C.ptr(err2), None, C.ptr(bnp), C.ptr(part2), d, st)
    per = dec0.numel() // 2
    sums, comb = torch.empty(2, device=DEV), torch.empty((), device=DEV)
    C.pair_loss_finalize(C.ptr(part), nwg, per, 1, C.ptr(sums), C.ptr(comb), st)
    torch.cuda.synchronize()
    ref = F.conv_transpose2d(act, w.double().cpu(), b.double().cpu(), stride=2)
    e = rel_err(dec0, ref)
    print("convT_out forward C = %d %dx%d: %.2e" % (c, hf, wf, e))
    assert e < 2e-5
    assert same_bits(dec1, dec0) and same_bits(err, dec0 - tgt) and same_bits(err2, err) and torch.equal(part2, part)
    sq = ((ref - tgt.double().cpu()) ** 2).reshape(2, -1).sum(1)
    assert rel_err(sums, sq) < 1e-5
    expect = sq[0] / per + sq[1] / per
    assert abs(float(comb) - float(expect)) <= 1e-5 * abs(float(expect))


@pytest.mark.parametrize("c,hf,wf", OS_CASES)
def test_convT_out_backward_fused_and_two_launches_beyond_one_job_per_wave(C, c, hf, wf):
    """The checks of test_convT_out_bwd_fused_matches_the_two_launches: dA, the BatchNorm-backward sums, dw and db of
    srlz_convT_out_bwd_fused against srlz_convT_out_bwd_data + srlz_convT_out_bwd_weight and against fp64 autograd, at its bounds;
    a second launch bit for bit."""
    groups = 2
    d, x_raw, w, _, dimg, bnp, act = os_inputs(C, c, hf, wf, 71 + hf, image=(1.0, 0.0))
    n = d.n
    assert C.convT_out_bwd_fused_supported(d) == 1
    st = C.stream()
    nb = C.bn_bwd_workspace(0)
    wsb = torch.empty(nb, dtype=torch.uint8, device=DEV)
    da0 = torch.full((n, hf, wf, 64), float("nan"), device=DEV)
    p0 = torch.full((C.skinny_tiles(d), 128), float("nan"), device=DEV)
    C.convT_out_bwd_data(C.ptr(dimg), C.ptr(w), C.ptr(da0), C.ptr(x_raw), C.ptr(bnp), C.ptr(p0), d, st)
    n0 = C.skinny_bwd_weight_workspace(d)
    ws0 = torch.empty(n0, dtype=torch.uint8, device=DEV)
    dw0, db0 = torch.full((64, c, 4, 4), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)
    C.convT_out_bwd_weight(C.ptr(x_raw), C.ptr(dimg), C.ptr(dw0), C.ptr(db0), C.ptr(bnp), C.ptr(ws0), n0, d, st)
    n1 = C.convT_out_bwd_fused_workspace(d)
    runs = []
    for _ in range(2):
        da = torch.full((n, hf, wf, 64), float("nan"), device=DEV)
        p = torch.full((C.convT_out_bwd_fused_tiles(d), 128), float("nan"), device=DEV)
        ws1 = torch.full((n1 // 4,), float("nan"), device=DEV)
        dw, db = torch.full((64, c, 4, 4), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)
        C.convT_out_bwd_fused(C.ptr(dimg), C.ptr(w), C.ptr(da), C.ptr(x_raw), C.ptr(bnp), C.ptr(p), C.ptr(dw), C.ptr(db), C.ptr(ws1), n1,
                              None, 1.0, 1.0, d, st)
        runs.append((da, p, dw, db))
    (da1, p1, dw1, db1), second = runs
    out = [[torch.empty(k, device=DEV) for k in (128 * groups, 64, 64)] for _ in range(2)]
    for p, o in ((p0, out[0]), (p1, out[1])):
        C.bn_bwd_finalize_partials(C.ptr(p), p.shape[0], groups, C.ptr(o[0]), C.ptr(o[1]), C.ptr(o[2]), C.ptr(wsb), nb, st)
    torch.cuda.synchronize()
    assert torch.isfinite(da1).all() and torch.isfinite(p1).all() and rel_err(da1, da0) < 5e-6
    for a_, b_ in zip(second, runs[0]):
        assert same_bits(a_, b_)
    for a_, b_ in zip(out[0], out[1]):
        assert rel_err(b_, a_) < 2e-5
    assert rel_err(dw1, dw0) < 2e-5
    ref = dimg.double().sum((0, 2, 3)).cpu()
    tol = 3e-6 * (n * d.himg * d.wimg) ** 0.5  # unit-variance data: a few fp32 ulps of the typical |sum|
    assert float((db0.double().cpu() - ref).abs().max()) <= tol and float((db1.double().cpu() - ref).abs().max()) <= tol
    wr = w.double().cpu().requires_grad_(True)
    a = act.requires_grad_(True)
    F.conv_transpose2d(a, wr, None, stride=2).backward(dimg.double().cpu())
    errs = rel_err(nchw(da1), a.grad), rel_err(dw1, wr.grad), rel_err(nchw(da0), a.grad), rel_err(dw0, wr.grad)
    print("convT_out backward C = %d %dx%d: fused dA %.2e dw %.2e, two launches dA %.2e dw %.2e" % ((c, hf, wf) + errs))
    assert max(errs) < 2e-5, errs
