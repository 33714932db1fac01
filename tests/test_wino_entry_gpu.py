"""The Winograd conv2 kernels (csrc/wino.hip) entry by entry (GPU): every srlz_conv64_wino_* entry point called by name, at the
smallest shapes at which each edge of the kernels exists (FWD_SHAPES / WGRAD_SHAPES of tests/wino_util.py, sized from
srlz_device_cus() where they depend on it): a single ragged tile, tiles across images, a patch row that is no power of two, a patch row
longer than a tile, G * tpg = 9, and 56 x 56 in two groups with the smallest even n at which workgroups take a second tile and, for
some, that tile lies in the other BatchNorm group (the persistent path with grp2 != grp, fused operand and pooled-block sums included).

Every case first asserts srlz_conv64_wino_tiles, srlz_conv64_wino_bwd_data_rows and srlz_conv64_wino_bwd_weight_workspace against the
rules restated in wino_util.py, so a case cannot quietly test another tiling or split.  Outputs are NaN before the call and sit between
NaN guards that must come back untouched; operands (x, dy, pooled, pool_y, the argmax bytes, the packed weights, the records, the bias)
sit between NaN guards too — in front of x as long as the (W + 1) pixels the input resource starts before the tensor — so a load that
runs on, or a resource that is too long, shows as NaN; workspaces are pre-filled with a NaN payload no sum can have and are followed by a
sentinel tail.

Two references per case (wino_util.py):
  * integer-exact: operands uniform integers of [-2, 2] (fused records: scale of {-2 .. 2}, shift of [-3, 3]).  B^T, A^T and A dY A^T
    only add and subtract, G g G^T adds and halves, every MFMA is fp32: every transform value, product and partial sum is a dyadic
    rational far below 2^24 (asserted by the operand makers), so the kernels must return the fp64 convolution, its gradients and the
    per-tile sums exactly, in any accumulation order ("exactly": equal as numbers and NaN-free; the sign of a zero is not held);
  * random operands against fp64 element by element, with the derived bounds of wino_util.py's docstring.

Largest error / bound seen on an MI355X (256 CUs: n = 22 for the 56 x 56 shape, 540 tiles on 512 workgroups; weight-gradient grids
16, 16, 16, 16, 48 and 512 with 1, 1, 2, 6, 5 and 9 stages per slice and 7, 6, 0, 0, 4 and 16 empty slices), printed by every case
as a "RATIO" line:
    fwd            y 0.017, records 0.020
    fwd (x_bnp)    y 0.019, records 0.020
    bwd_data       dx 0.017
    bwd_weight     dw 0.145 (4 x 4, n = 1: four patches, where T_WGRAD is more than half of the bound; 0.0008 at 56 x 56)
The fp32 emulation of test_wino_host_cpu.py sits at the same figures (0.008 - 0.020 and 0.171): the kernels are as accurate as their
roundings have to be, and none is near 1.  Every integer case is exact.
"""
import functools

import numpy as np
import pytest
import torch

import wino_util as wu
from test_kernels_gpu import C, DEV  # noqa: F401  (C: the module-scoped fixture of the kernel tests)
from test_rect_kernels_gpu import tiles_wino
from test_update_path_gpu import GUARD, NAN, same_bits

pytestmark = pytest.mark.gpu

WS_SENTINEL = 0x7FC0BEEF  # a NaN with a payload: no sum of finite numbers has these bits
BAD_DESC, WORKSPACE = -1, -2


def lead(w):
    """Guard floats around a [n, h, w, 64] tensor: more than the (w + 1) pixels the input resource starts in front of it."""
    return (w + 2) * 64


class Buf:
    """A device tensor between two guards (NaN; bytes of 255 for uint8).  Without `src` the payload is NaN / 255 too: an output."""

    def __init__(self, shape, guard=GUARD, src=None, dtype=torch.float32):
        self.g, self.n = guard, int(np.prod(shape))
        self.fill = 255 if dtype == torch.uint8 else NAN
        self.whole = torch.full((2 * guard + self.n,), self.fill, dtype=dtype, device=DEV)
        self.view = self.whole[guard:guard + self.n].view(tuple(shape))
        if src is not None:
            self.view.copy_(torch.from_numpy(np.array(src)))  # (a writable copy: the cached inputs are read-only)
        assert self.view.data_ptr() % 16 == 0

    def _is_fill(self, t):
        return bool((t == 255).all()) if self.fill == 255 else bool(torch.isnan(t).all())

    def guards_intact(self):
        return self._is_fill(self.whole[:self.g]) and self._is_fill(self.whole[self.g + self.n:])

    def untouched(self):
        return self._is_fill(self.whole)

    def result(self):
        """The payload on the host; the guards in front of it and behind it must be intact."""
        assert self.guards_intact(), "written outside the output"
        return self.view.cpu().numpy()


class Workspace:
    """`nbytes` of workspace filled with WS_SENTINEL and GUARD more words behind it."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.nbytes = nbytes
        self.whole = torch.full((nbytes // 4 + GUARD,), WS_SENTINEL, dtype=torch.int32, device=DEV)

    def tail_intact(self):
        return bool((self.whole[self.nbytes // 4:] == WS_SENTINEL).all())

    def untouched(self):
        return bool((self.whole == WS_SENTINEL).all())


def ptr_of(C, v):
    return C.ptr(v.view if isinstance(v, Buf) else v.whole if isinstance(v, Workspace) else v)


def conv_desc(C, n, h, w, groups):
    return C.Conv64Desc(n, h, w, h, w, 3, 1, 1, 0, groups)


def assert_queries(C, h, w, n, groups):
    """The library's tiling and split of this shape are the restated ones -> (descriptor, forward plan, weight-gradient plan)."""
    d = conv_desc(C, n, h, w, groups)
    P, Wp = wu.fwd_plan(n, h, w, groups), wu.wgrad_plan(n, h, w, C.device_cus())
    assert C.conv64_wino_supported(d) == 1
    assert C.conv64_wino_tiles(d) == P["tiles"]
    assert C.conv64_wino_bwd_data_rows(d) == P["rows"]
    assert C.conv64_wino_bwd_weight_workspace(d) == Wp["workspace"]
    return d, P, Wp


def equal_values(got, want):
    """got (device fp32) equals want (numpy fp64, exactly representable) element by element, NaN-free."""
    w32 = want.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want)
    return tuple(got.shape) == want.shape and bool((got == torch.from_numpy(w32).to(DEV)).all())


@functools.lru_cache(maxsize=None)
def dev_weights(kind):
    """(w, bias, packed forward, packed data gradient) on the device, all between NaN guards; the packs by srlz_conv64_wino_pack_weights."""
    from srlz import _cabi
    wt, b = wu.weights(kind)
    w, bias = Buf(wt.shape, src=wt), Buf(b.shape, src=b)
    uf, ub = Buf((wu.PACKED,)), Buf((wu.PACKED,))
    assert _cabi.conv64_wino_packed_floats() == wu.PACKED
    _cabi.conv64_wino_pack_weights(_cabi.ptr(w.view), _cabi.ptr(uf.view), _cabi.ptr(ub.view), _cabi.stream())
    torch.cuda.synchronize()
    assert uf.guards_intact() and ub.guards_intact() and not bool(torch.isnan(uf.view).any() | torch.isnan(ub.view).any())
    return w, bias, uf, ub


@functools.lru_cache(maxsize=4)
def dev_operands(kind, h, w, n, groups):
    d = wu.operands(kind, h, w, n, groups)
    return {"x": Buf(d["x"].shape, lead(w), d["x"]), "dy": Buf(d["dy"].shape, lead(w), d["dy"]), "recs": Buf(d["recs"].shape, src=d["recs"])}


def records_of(y, groups):
    """[G * tpg, 128] fp64: per tile the sums of y and of y^2 (y [n, h, w, 64] fp64)."""
    return np.concatenate([wu.tile_sums(y, groups), wu.tile_sums(y * y, groups)], axis=2).reshape(-1, 128)


def run_fwd(C, d, P, x, up, bias, recs, want_stats):
    shape = (d.n, d.hi, d.wi, 64)
    y, st = Buf(shape, lead(d.wi)), (Buf((P["tiles"], 128)) if want_stats else None)
    C.conv64_wino_fwd(C.ptr(x.view), C.ptr(up.view), ptr_of(C, bias) if bias else None, C.ptr(y.view), ptr_of(C, st) if st else None,
                      ptr_of(C, recs) if recs else None, d, C.stream())
    torch.cuda.synchronize()
    assert y.guards_intact() and (st is None or st.guards_intact())
    return y, st


def run_bwd_data(C, d, dy, ub):
    dx = Buf((d.n, d.hi, d.wi, 64), lead(d.wi))
    C.conv64_wino_bwd_data(C.ptr(dy.view), C.ptr(ub.view), C.ptr(dx.view), d, C.stream())
    torch.cuda.synchronize()
    assert dx.guards_intact()
    return dx


def run_bwd_weight(C, d, Wp, x, dy):
    """-> (dw, the workgroups' partials [grid, 8 * 4096] on the host); the workspace is written exactly over its own bytes."""
    ws, dw = Workspace(Wp["workspace"]), Buf((64, 64, 3, 3))
    C.conv64_wino_bwd_weight(C.ptr(x.view), C.ptr(dy.view), C.ptr(dw.view), C.ptr(ws.whole), ws.nbytes, d, C.stream())
    torch.cuda.synchronize()
    assert dw.guards_intact() and ws.tail_intact()
    own = ws.whole[:ws.nbytes // 4]
    assert bool((own != WS_SENTINEL).all()), "a word of the workspace the entry point owns was not written"
    part = own[:Wp["grid"] * 8 * 4096].view(torch.float32).view(Wp["grid"], 8 * 4096).cpu().numpy()
    return dw, part


def assert_split(Wp, part):
    """The workgroups of the empty slices (the last ones) and no others left a partial of zeros: the split is the restated one."""
    used = Wp["slices"] - Wp["empty"]
    for b in range(Wp["grid"]):
        s, _ = wu.slice_of_workgroup(b, Wp["grid"])
        assert bool((part[b] == 0).all()) == (s >= used), (b, s, used)


# ---- 1. the pack --------------------------------------------------------------------------------------------------------------------
def test_pack_weights(C):
    """Weights ((co * 64 + ci) * 9 + 3 ky + kx) / 2 — every entry distinct, every transform value exact — packed in both directions equal
    the restated layout bit for bit over all 4 * WN_CHUNK floats; a NULL direction leaves its buffer alone."""
    co, ci, ky, kx = np.meshgrid(np.arange(64), np.arange(64), np.arange(3), np.arange(3), indexing="ij")
    wt = (((co * 64 + ci) * 9 + 3 * ky + kx) / 2).astype(np.float32)
    w = Buf(wt.shape, src=wt)
    assert C.conv64_wino_packed_floats() == wu.PACKED == 4 * wu.WN_CHUNK
    for dirs in ((True, True), (True, False), (False, True)):
        outs = [Buf((wu.PACKED,)), Buf((wu.PACKED,))]
        C.conv64_wino_pack_weights(C.ptr(w.view), *[C.ptr(o.view) if on else None for o, on in zip(outs, dirs)], C.stream())
        torch.cuda.synchronize()
        for bwd, (o, on) in enumerate(zip(outs, dirs)):
            if on:
                assert same_bits(torch.from_numpy(o.result()), wu.pack_ref(wt, bool(bwd)).astype(np.float32)), ("direction", bwd)
            else:
                assert o.untouched()
    none = C._lib.srlz_conv64_wino_pack_weights(C.ptr(w.view), None, None, C.stream())
    assert none == -4
    assert w.guards_intact()


# ---- 2. integer-exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wu.FWD_SHAPES, ids=wu.shape_id)
def test_fwd_exact(C, shape):
    """srlz_conv64_wino_fwd with and without bias, statistics and the fused operand: y is the fp64 convolution of the integers, every
    record the fp64 sums over its tile's patches, the second launch bit-identical."""
    h, w, n, groups = wu.resolve(shape, C.device_cus())
    d, P, _ = assert_queries(C, h, w, n, groups)
    ops, r = dev_operands("int", h, w, n, groups), wu.conv_refs("int", h, w, n, groups)
    _, bias, uf, _ = dev_weights("int")
    b64 = wu.weights("int")[1].astype(np.float64)
    assert np.array_equal(np.broadcast_to(tiles_wino(n, h, w, groups, P["tpg"]).numpy(), (n, h, w)), wu.tile_of_pixel(n, h, w, groups, P["tpg"]))
    for fused in (False, True):
        for with_bias in (False, True):
            ref = r["y_fused" if fused else "y"] + (b64 if with_bias else 0.0)
            rec_ref = records_of(ref, groups)
            for want_stats in (False, True):
                name = "fused=%d bias=%d stats=%d" % (fused, with_bias, want_stats)
                first = None
                for _ in range(2):
                    y, st = run_fwd(C, d, P, ops["x"], uf, bias if with_bias else None, ops["recs"] if fused else None, want_stats)
                    assert equal_values(y.view, ref), name
                    if st is not None:
                        assert equal_values(st.view, rec_ref), name
                    if first is not None:
                        assert torch.equal(first[0].view(torch.int32), y.view.view(torch.int32)), name
                        assert st is None or torch.equal(first[1].view(torch.int32), st.view.view(torch.int32)), name
                    first = (y.view, st.view if st is not None else None)
    assert all(v.guards_intact() for v in ops.values())


@pytest.mark.parametrize("shape", wu.FWD_SHAPES, ids=wu.shape_id)
def test_bwd_data_exact(C, shape):
    h, w, n, groups = wu.resolve(shape, C.device_cus())
    d, P, _ = assert_queries(C, h, w, n, groups)
    ops, r = dev_operands("int", h, w, n, groups), wu.conv_refs("int", h, w, n, groups)
    ub = dev_weights("int")[3]
    dx = run_bwd_data(C, d, ops["dy"], ub)
    assert equal_values(dx.view, r["dx"])
    dx2 = run_bwd_data(C, d, ops["dy"], ub)
    assert torch.equal(dx.view.view(torch.int32), dx2.view.view(torch.int32))


@pytest.mark.parametrize("shape", wu.WGRAD_SHAPES, ids=wu.shape_id)
def test_bwd_weight_exact(C, shape):
    """srlz_conv64_wino_bwd_weight on integers is fp64 autograd's dW exactly, with the grid, the stages per slice and the empty slices of
    the restated plan (the table of wino_util.py at 256 and at 8 CUs); every workgroup's partial is the exact sum over its own slice."""
    h, w, n = wu.resolve(shape, C.device_cus())
    G = wu.wgrad_groups(shape)
    d, _, Wp = assert_queries(C, h, w, n, G)
    cus = C.device_cus()
    if cus in wu.WGRAD_PLANS:
        assert (Wp["grid"], Wp["spw"], Wp["empty"]) == wu.WGRAD_PLANS[cus][wu.WGRAD_SHAPES.index(shape)]
    print("PLAN wgrad %s: %d CUs, grid %d, %d stages, spw %d, %d empty slices" % (wu.shape_id(shape), cus, Wp["grid"], Wp["stages"], Wp["spw"],
                                                                                   Wp["empty"]))
    ops, r = dev_operands("int", h, w, n, G), wu.conv_refs("int", h, w, n, G)
    wu.assert_wgrad_exact(wu.operands("int", h, w, n, G), Wp["spw"])
    dw, part = run_bwd_weight(C, d, Wp, ops["x"], ops["dy"])
    assert equal_values(dw.view, r["dw"])
    assert_split(Wp, part)
    host = wu.operands("int", h, w, n, G)
    assert np.array_equal(part.astype(np.float64).reshape(Wp["grid"], 8, 64, 64), wu.wgrad_partials(host["x"], host["dy"], Wp)), \
        "a workgroup's partial is not the sum over its slice"
    dw2, part2 = run_bwd_weight(C, d, Wp, ops["x"], ops["dy"])
    assert torch.equal(dw.view.view(torch.int32), dw2.view.view(torch.int32)) and np.array_equal(part.view(np.int32), part2.view(np.int32))


# ---- 3. the pooled block's sums, exact -------------------------------------------------------------------------------------------------
POOL_CASES = [(4, 4, 1, 1, 1), (6, 10, 3, 3, 0), (6, 10, 3, 3, 1), (8, 8, 4, 2, 0), (56, 56, 0, 2, 1)]


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "%dx%d-n%s-g%d-pad%d" % (c[0], c[1], c[2] or "big", c[3], c[4]))
def test_bwd_data_pool_sums_exact(C, case):
    """srlz_conv64_wino_bwd_data_pool_sums on integers: dx is srlz_conv64_wino_bwd_data's; each of the tpg tile records is the fp64
    (sum dA masked, sum dA * xhat) of its tile, with exact zeros at the zero-scale channels, whose sums arrive in the 64 cold records;
    per group all tpg + 64 records add up to the fp64 sums.  pooled and argmax are the project's own bn_relu_pool forward of pool_y."""
    hp, wp, n, groups, pad = case
    n = n or wu.big_n(C.device_cus())
    d, P, _ = assert_queries(C, hp, wp, n, groups)
    p = wu.pool_operands(hp, wp, n, groups, pad)
    h, w, recs = p["h"], p["w"], p["recs"]
    pool_y, bnp = Buf(p["pool_y"].shape, lead(w), p["pool_y"]), Buf(recs.shape, src=recs)
    pooled, arg = Buf((n, hp, wp, 64), lead(wp)), Buf((n, hp, wp, 64), lead(wp), dtype=torch.uint8)
    pd = C.PoolDesc(n, h, w, hp, wp, pad, 0, groups)
    C.bn_relu_pool_fwd(C.ptr(pool_y.view), C.ptr(bnp.view), C.ptr(pooled.view), C.ptr(arg.view), pd, C.stream())
    torch.cuda.synchronize()
    z = wu.pool_forward(p["pool_y"], recs, groups, pad)
    assert pooled.guards_intact() and arg.guards_intact() and equal_values(pooled.view, z)
    ops, ub = dev_operands("int", hp, wp, n, groups), dev_weights("int")[3]
    da = wu.conv_refs("int", hp, wp, n, groups)["dx"]
    dz, dzx = wu.pool_sum_values(da, arg.view.cpu().numpy(), p["pool_y"], recs, groups, pad)
    zero = wu.zero_scale(recs)
    assert zero.sum(1).tolist() == [2] * groups
    wu.assert_pool_exact(da, z, recs, groups)
    ref = np.concatenate([wu.tile_sums(dz, groups), wu.tile_sums(dzx, groups)], axis=2)          # [G, tpg, 128]
    total = ref.sum(1)
    hot = ref * np.tile(~zero, (1, 2))[:, None, :]
    assert np.abs(total[np.tile(zero, (1, 2))]).max() > 0 and np.abs(hot).max() > 0  # (both kinds of record carry a signal)
    first = None
    for _ in range(2):
        dx, part = Buf((n, hp, wp, 64), lead(wp)), Buf((P["rows"], 128))
        C.conv64_wino_bwd_data_pool_sums(C.ptr(ops["dy"].view), C.ptr(ub.view), C.ptr(dx.view), C.ptr(pooled.view), C.ptr(bnp.view),
                                         C.ptr(pool_y.view), C.ptr(arg.view), pd, C.ptr(part.view), d, C.stream())
        torch.cuda.synchronize()
        assert equal_values(dx.view, da)
        got = part.result().astype(np.float64).reshape(groups, P["tpg"] + wu.ZBLOCKS, 128)
        assert not np.isnan(got).any()
        assert np.array_equal(got[:, :P["tpg"]], hot), "tile records"
        cold = got[:, P["tpg"]:].sum(1)
        assert np.array_equal(cold, total * np.tile(zero, (1, 2))), "cold records"
        assert np.array_equal(got.sum(1), total)
        if first is not None:
            assert torch.equal(first[0].view(torch.int32), dx.view.view(torch.int32))
            assert torch.equal(first[1].view(torch.int32), part.view.view(torch.int32))
        first = (dx.view, part.view)
    plain = run_bwd_data(C, d, ops["dy"], ub)
    assert torch.equal(plain.view.view(torch.int32), first[0].view(torch.int32))
    assert pool_y.guards_intact() and bnp.guards_intact() and pooled.guards_intact() and arg.guards_intact()


# ---- 4. random operands against fp64, element by element -----------------------------------------------------------------------------
def ratio(name, got, ref, bnd):
    v = wu.worst_ratio(got, ref, bnd)
    print("RATIO %s %.4f" % (name, v))
    assert v <= 1.0, (name, v)
    return v


def check_records(name, st, y, groups):
    """The records against the sums of the kernel's own output."""
    y = y.astype(np.float64)
    got = st.result().astype(np.float64)
    ratio(name, got, records_of(y, groups), wu.bound_records(records_of(np.abs(y), groups)))


@pytest.mark.parametrize("shape", wu.FWD_SHAPES, ids=wu.shape_id)
def test_fwd_and_bwd_data_random(C, shape):
    h, w, n, groups = wu.resolve(shape, C.device_cus())
    d, P, _ = assert_queries(C, h, w, n, groups)
    ops, r = dev_operands("rnd", h, w, n, groups), wu.conv_refs("rnd", h, w, n, groups)
    _, bias, uf, ub = dev_weights("rnd")
    b = wu.weights("rnd")[1]
    sid = wu.shape_id(shape)
    y, st = run_fwd(C, d, P, ops["x"], uf, bias, None, True)
    yh = y.result()
    ratio("fwd:y %s" % sid, yh, r["y"] + b.astype(np.float64), wu.bound_fwd(r["m_x"] + np.abs(b).astype(np.float64)))
    check_records("fwd:records %s" % sid, st, yh, groups)
    y, st = run_fwd(C, d, P, ops["x"], uf, None, ops["recs"], True)
    yh = y.result()
    ratio("fwd(x_bnp):y %s" % sid, yh, r["y_fused"], wu.bound_fwd(r["m_act"]))
    check_records("fwd(x_bnp):records %s" % sid, st, yh, groups)
    dx = run_bwd_data(C, d, ops["dy"], ub)
    ratio("bwd_data:dx %s" % sid, dx.result(), r["dx"], wu.bound_fwd(r["m_dy"]))
    assert all(v.guards_intact() for v in ops.values())


@pytest.mark.parametrize("shape", wu.WGRAD_SHAPES, ids=wu.shape_id)
def test_bwd_weight_random(C, shape):
    h, w, n = wu.resolve(shape, C.device_cus())
    G = wu.wgrad_groups(shape)
    d, _, Wp = assert_queries(C, h, w, n, G)
    ops, host = dev_operands("rnd", h, w, n, G), wu.operands("rnd", h, w, n, G)
    dw, part = run_bwd_weight(C, d, Wp, ops["x"], ops["dy"])
    assert_split(Wp, part)
    ratio("bwd_weight:dw %s grid=%d spw=%d" % (wu.shape_id(shape), Wp["grid"], Wp["spw"]), dw.result(),
          wu.conv_refs("rnd", h, w, n, G)["dw"], wu.bound_wgrad(wu.wgrad_mag(host["x"], host["dy"]), Wp["spw"]))


# ---- 5. guards and refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(C):
    """A short workspace (SRLZ_ERR_WORKSPACE), an odd axis, n % groups != 0 and a pool descriptor that is not the layer's input
    (SRLZ_ERR_BAD_DESC): the documented code, and not a byte of an output or workspace changed."""
    L, st = C._lib, C.stream()
    h, w, n, groups = 8, 8, 4, 2
    ops = dev_operands("int", h, w, n, groups)
    _, bias, uf, ub = dev_weights("int")
    good = conv_desc(C, n, h, w, groups)
    nb = C.conv64_wino_bwd_weight_workspace(good)
    out, stats, dw, ws = Buf((n, h, w, 64), lead(w)), Buf((wu.fwd_plan(n, h, w, groups)["rows"], 128)), Buf((64, 64, 3, 3)), Workspace(nb)
    p = wu.pool_operands(h, w, n, groups, 1)
    pool_y, bnp = Buf(p["pool_y"].shape, lead(p["w"]), p["pool_y"]), Buf(p["recs"].shape, src=p["recs"])
    pooled, arg = Buf((n, h, w, 64), lead(w)), Buf((n, h, w, 64), lead(w), dtype=torch.uint8)
    pd = C.PoolDesc(n, p["h"], p["w"], h, w, 1, 0, groups)
    C.bn_relu_pool_fwd(C.ptr(pool_y.view), C.ptr(bnp.view), C.ptr(pooled.view), C.ptr(arg.view), pd, st)
    torch.cuda.synchronize()

    def clean():
        torch.cuda.synchronize()
        return out.untouched() and stats.untouched() and dw.untouched() and ws.untouched()

    def pool_sums(pdesc, desc):
        return L.srlz_conv64_wino_bwd_data_pool_sums(C.ptr(ops["dy"].view), C.ptr(ub.view), C.ptr(out.view), C.ptr(pooled.view), C.ptr(bnp.view),
                                                     C.ptr(pool_y.view), C.ptr(arg.view), pdesc, C.ptr(stats.view), desc, st)

    assert L.srlz_conv64_wino_bwd_weight(C.ptr(ops["x"].view), C.ptr(ops["dy"].view), C.ptr(dw.view), C.ptr(ws.whole), nb - 1, good, st) == WORKSPACE
    assert L.srlz_conv64_wino_bwd_weight(C.ptr(ops["x"].view), C.ptr(ops["dy"].view), C.ptr(dw.view), C.ptr(ws.whole), 0, good, st) == WORKSPACE
    assert clean()
    bad = [C.Conv64Desc(n, 7, 8, 7, 8, 3, 1, 1, 0, groups), C.Conv64Desc(n, 8, 7, 8, 7, 3, 1, 1, 0, groups),   # an odd axis, either one
           C.Conv64Desc(3, h, w, h, w, 3, 1, 1, 0, 2),                                                         # n % groups != 0
           C.Conv64Desc(n, 2, 8, 2, 8, 3, 1, 1, 0, groups)]                                                    # an axis below 4
    for desc in bad:
        assert C.conv64_wino_supported(desc) == 0 and C.conv64_wino_tiles(desc) == -1 and C.conv64_wino_bwd_data_rows(desc) == -1
        assert C.conv64_wino_bwd_weight_workspace(desc) == 0
        assert L.srlz_conv64_wino_fwd(C.ptr(ops["x"].view), C.ptr(uf.view), C.ptr(bias.view), C.ptr(out.view), C.ptr(stats.view), None, desc,
                                      st) == BAD_DESC
        assert L.srlz_conv64_wino_bwd_data(C.ptr(ops["dy"].view), C.ptr(ub.view), C.ptr(out.view), desc, st) == BAD_DESC
        assert L.srlz_conv64_wino_bwd_weight(C.ptr(ops["x"].view), C.ptr(ops["dy"].view), C.ptr(dw.view), C.ptr(ws.whole), nb, desc, st) == BAD_DESC
        assert pool_sums(pd, desc) == BAD_DESC
        assert clean()
    # pool descriptors that do not describe this layer's input: another height, another width, another batch, NCHW output, other groups
    for pdesc in (C.PoolDesc(n, p["h"], p["w"], h + 2, w, 1, 0, groups), C.PoolDesc(n, p["h"], p["w"], h, w - 2, 1, 0, groups),
                  C.PoolDesc(n - 2, p["h"], p["w"], h, w, 1, 0, groups), C.PoolDesc(n, p["h"], p["w"], h, w, 1, 1, groups),
                  C.PoolDesc(n, p["h"], p["w"], h, w, 1, 0, 1)):
        assert pool_sums(pdesc, good) == BAD_DESC
        assert clean()
    # and the same arguments with the right descriptors run
    assert pool_sums(pd, good) == 0
    assert L.srlz_conv64_wino_bwd_weight(C.ptr(ops["x"].view), C.ptr(ops["dy"].view), C.ptr(dw.view), C.ptr(ws.whole), nb, good, st) == 0
    torch.cuda.synchronize()
    assert equal_values(out.view, wu.conv_refs("int", h, w, n, groups)["dx"]) and equal_values(dw.view, wu.conv_refs("int", h, w, n, groups)["dw"])
    assert out.guards_intact() and stats.guards_intact() and dw.guards_intact() and ws.tail_intact()


# ---- 6. through srlz.ops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_conv64_fn_exact(C, with_bias):
    """The Conv64Fn node that _conv64_forward serves on the Winograd route, on the integers of 6 x 10 in three groups: y, the records,
    dx, dw and db exact (without a bias the weight gradient is srlz_conv64_wino_bwd_weight's, with one the direct kernel's)."""
    from srlz import ops
    h, w, n, groups = 6, 10, 3, 3
    host, r, (wt, b) = wu.operands("int", h, w, n, groups), wu.conv_refs("int", h, w, n, groups), wu.weights("int")
    assert C.conv64_wino_supported(ops.conv64_desc(n, h, w, 1, 1, 0, groups)) == 1

    def leaf(a):
        return torch.from_numpy(np.array(a)).to(DEV).requires_grad_(True)

    x, wd, bd = leaf(host["x"]), leaf(wt), (leaf(b) if with_bias else None)
    with ops.batch_groups(groups):
        y, stats = ops.Conv64Fn.apply(x, wd, bd, 1, 1, 0, True, None)
    y.backward(torch.from_numpy(np.array(host["dy"])).to(DEV))
    torch.cuda.synchronize()
    ref = r["y"] + (b.astype(np.float64) if with_bias else 0.0)
    assert equal_values(y.detach(), ref)
    assert equal_values(stats.detach(), records_of(ref, groups))
    assert equal_values(x.grad, r["dx"]) and equal_values(wd.grad, r["dw"])
    if with_bias:
        assert equal_values(bd.grad, host["dy"].astype(np.float64).sum((0, 1, 2)))

