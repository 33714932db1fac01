"""tests/wino_util.py against itself and against plain integer arithmetic (no GPU): what tests/test_wino_entry_gpu.py relies on.

  * the fp32 emulation of csrc/wino.hip's algorithm on small-integer operands returns the integer convolution, its data gradient and its
    weight gradient bit for bit — so a kernel that does not has a wrong term, not a rounding;
  * on the random operands of the GPU file the emulation's error stays below half of the derived element bounds (printed): a bound the
    reference's own restatement fills would prove nothing about the kernel;
  * the plan restatement gives the grid, the stages per slice and the empty slices the GPU file's cases are chosen for, at 256 CUs and
    at 8;
  * every integer case satisfies its exactness conditions (the 56 x 56 shape at both sizes, the pooled block included), the pack layout
    is a bijection, the workgroups' restated weight-gradient partials add up to the gradient, the pooled block's reference sums are
    autograd's, and fma32 is the correctly rounded fp32 fma;
  * the checks notice a wrong kernel: the emulation with an 11-bit patch operand exceeds the element bound, one transform value off by
    one is an exact mismatch.
"""
import numpy as np
import pytest

import wino_util as wu

CUS = (256, 8)
SMALL_FWD = wu.FWD_SHAPES[:-1]


def test_transform_matrices_compute_the_convolution():
    """Y = A^T [(G g G^T) .* (B^T d B)] A in fp64 is the 3 x 3 correlation of one patch; dW = G^T [(A dY A^T) .* (B^T d B)] G its weight
    gradient."""
    rs = np.random.RandomState(0)
    g, d, dy = rs.randint(-4, 5, size=(3, 3)), rs.randint(-4, 5, size=(4, 4)), rs.randint(-4, 5, size=(2, 2))
    y = wu.AT @ ((wu.G @ g @ wu.G.T) * (wu.BT @ d @ wu.BT.T)) @ wu.AT.T
    want = np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(2)] for i in range(2)])
    assert np.array_equal(y, want)
    dw = wu.G.T @ ((wu.AT.T @ dy @ wu.AT) * (wu.BT @ d @ wu.BT.T)) @ wu.G
    want = np.array([[(d[a:a + 2, b:b + 2] * dy).sum() for b in range(3)] for a in range(3)])
    assert np.array_equal(dw, want)


def test_pack_layout_is_a_bijection_and_the_fp32_pack_is_exact_on_half_integers():
    idx = wu.pack_layout(np.arange(64 * 64 * 16, dtype=np.float64).reshape(64, 64, 4, 4))
    assert np.array_equal(np.sort(idx), np.arange(wu.PACKED))
    # element [p][comp][g][m][e] holds U[m][16 p + 4 g + e][comp]
    p, comp, gq, m, e = 2, 7, 3, 41, 1
    assert idx[(((p * 16 + comp) * 4 + gq) * 64 + m) * 4 + e] == (m * 64 + 16 * p + 4 * gq + e) * 16 + comp
    co, ci, ky, kx = np.meshgrid(np.arange(64), np.arange(64), np.arange(3), np.arange(3), indexing="ij")
    w = (((co * 64 + ci) * 9 + 3 * ky + kx) / 2).astype(np.float32)
    for bwd in (False, True):
        g = wu.direction_weights(w, bwd)
        assert g[3, 5, 0, 1] == (w[5, 3, 2, 1] if bwd else w[3, 5, 0, 1])
        u64 = wu.transform_weights(g)
        assert np.array_equal(wu.transform_weights_f32(g).astype(np.float64), u64)
        assert len(np.unique(w)) == w.size and np.abs(u64 * 8).max() < wu.LIMIT and np.array_equal(u64 * 8, np.rint(u64 * 8))


def test_tile_map_and_tile_sums_agree():
    for h, w, n, groups in [(6, 10, 3, 3), (4, 68, 1, 1), (16, 20, 3, 3)]:
        P = wu.fwd_plan(n, h, w, groups)
        v = np.random.RandomState(h).randint(-9, 10, size=(n, h, w, 64)).astype(np.float64)
        tile = wu.tile_of_pixel(n, h, w, groups, P["tpg"])
        want = np.zeros((P["tiles"], 64))
        np.add.at(want, tile.reshape(-1), v.reshape(-1, 64))
        assert np.array_equal(wu.tile_sums(v, groups).reshape(-1, 64), want)


@pytest.mark.parametrize("cus", CUS)
def test_forward_tiles_and_runs(cus):
    """The tile counts of the table; every tile is taken exactly once; and the 56 x 56 shape is the smallest at which workgroups take a
    second tile and, for some, that tile lies in the other group."""
    for shape, tiles in zip(wu.FWD_SHAPES, wu.FWD_TILES):
        h, w, n, groups = wu.resolve(shape, cus)
        P = wu.fwd_plan(n, h, w, groups)
        if tiles is not None:
            assert P["tiles"] == tiles, shape
        grid = wu.launch_grid(P["tiles"], cus)
        runs = wu.tiles_of_workgroups(P["tiles"], grid)
        assert sorted(t for r in runs for t in r) == list(range(P["tiles"]))
        two = [r for r in runs if len(r) > 1]
        assert bool(two) == (shape[2] == 0), shape
        if shape[2] == 0:
            assert n == wu.BIG_N[cus] and P["tiles"] > 2 * cus + 8
            steps = [(a // P["tpg"], b // P["tpg"]) for r in two for a, b in zip(r, r[1:])]
            assert any(ga != gb for ga, gb in steps) and any(ga == gb for ga, gb in steps)
            assert wu.fwd_plan(n - 2, h, w, groups)["tiles"] <= 2 * cus + 8
    assert wu.fwd_plan(22, 56, 56, 2)["tpg"] == 270 and wu.fwd_plan(22, 56, 56, 2)["ppg"] % 32 == 16
    assert wu.fwd_plan(3, 16, 20, 3)["tiles"] & 7 == 1


@pytest.mark.parametrize("cus", CUS)
def test_weight_gradient_plans(cus):
    for shape, (grid, spw, empty) in zip(wu.WGRAD_SHAPES, wu.WGRAD_PLANS[cus]):
        h, w, n = wu.resolve(shape, cus)
        P = wu.wgrad_plan(n, h, w, cus)
        assert (P["grid"], P["spw"], P["empty"]) == (grid, spw, empty), (shape, P)
        assert P["workspace"] == grid * 8 * 4096 * 4 + 8 * 16 * 4096 * 8
        assert P["stages"] == wu.cdiv(n * (h // 2) * (w // 2), 8) and P["spw"] * (P["slices"] - P["empty"]) >= P["stages"]
        # every slice has both of its halves, once
        seen = sorted(wu.slice_of_workgroup(b, grid) for b in range(grid))
        assert seen == [(s, half) for s in range(P["slices"]) for half in (0, 1)]
    mid = wu.wgrad_plan(2, 40, 40, 256)
    assert 16 < mid["grid"] < 512 and mid["total"] == 800


def test_emulation_is_exact_on_integers():
    """Operands uniform in [-4, 4], n = 3, 10 x 14: forward (with bias), data gradient and weight gradient of the fp32 emulation equal
    the fp64 results bit for bit; the largest sum_ci |U||V| stays far below 2^22."""
    rs = np.random.RandomState(3)
    x, dy = (rs.randint(-4, 5, size=(3, 10, 14, 64)).astype(np.float32) for _ in range(2))
    w, b = rs.randint(-4, 5, size=(64, 64, 3, 3)).astype(np.float32), rs.randint(-4, 5, size=64).astype(np.float32)
    s = wu.chain_mag(x, w).max()
    print("largest sum_ci |U||V| %.2f" % s)
    assert 4 * s < wu.LIMIT
    assert np.array_equal(wu.emulate_conv(x, w, b).astype(np.float64), wu.conv64(x, w, b))
    dx, dw = wu.grads64(x, w, dy)
    assert np.array_equal(wu.emulate_conv(dy, wu.direction_weights(w, True)).astype(np.float64), dx)
    for spw in (1, 3, 14):
        assert np.array_equal(wu.emulate_wgrad(x, dy, spw).astype(np.float64), dw)


@pytest.mark.parametrize("shape", SMALL_FWD + [(56, 56, 0, 2)], ids=wu.shape_id)
def test_integer_cases_are_exact_and_emulated_exactly(shape):
    """Every integer case of the GPU file satisfies its exactness conditions (asserted inside conv_refs), and the emulation returns its
    references bit for bit (the 56 x 56 shape at its 8-CU size)."""
    h, w, n, groups = wu.resolve(shape, 8)
    d, r, (wt, b) = wu.operands("int", h, w, n, groups), wu.conv_refs("int", h, w, n, groups), wu.weights("int")
    assert np.array_equal(wu.emulate_conv(d["x"], wt, b).astype(np.float64), r["y"] + b.astype(np.float64))
    assert np.array_equal(wu.emulate_conv(d["act"], wt).astype(np.float64), r["y_fused"])
    assert np.array_equal(wu.emulate_conv(d["dy"], wu.direction_weights(wt, True)).astype(np.float64), r["dx"])


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("shape", wu.WGRAD_SHAPES, ids=wu.shape_id)
def test_integer_weight_gradient_cases_are_exact(shape, cus):
    h, w, n = wu.resolve(shape, cus)
    G = wu.wgrad_groups(shape)
    d = wu.operands("int", h, w, n, G)
    P = wu.wgrad_plan(n, h, w, cus)
    wu.assert_wgrad_exact(d, P["spw"])
    if n * h * w <= 2 * 56 * 56:
        assert np.array_equal(wu.emulate_wgrad(d["x"], d["dy"], P["spw"]).astype(np.float64), wu.conv_refs("int", h, w, n, G)["dw"])


@pytest.mark.parametrize("hp,wp,n,groups,pad", [(6, 10, 3, 3, 0), (6, 10, 3, 3, 1), (4, 4, 1, 1, 1)])
def test_pool_sum_reference_on_the_hosts_own_argmax(hp, wp, n, groups, pad):
    """pool_sum_values under the first-maximum argmax of the host's pooling: the masked gradient sums are those of fp64 autograd through
    max_pool2d(relu(bn(.)))."""
    import torch
    import torch.nn.functional as F
    p = wu.pool_operands(hp, wp, n, groups, pad)
    da = wu.operands("int", hp, wp, n, groups)["dy"]
    per = n // groups
    y = wu.nchw64(p["pool_y"]).requires_grad_(True)
    rec = torch.from_numpy(np.repeat(p["recs"].astype(np.float64), per, axis=0))[:, :, None, None]
    z = F.relu(y * rec[:, 128:192] + rec[:, 192:])
    pooled, idx = F.max_pool2d(z, 3, 2, pad, return_indices=True)
    assert np.array_equal(wu.nhwc_np(pooled), wu.pool_forward(p["pool_y"], p["recs"], groups, pad))
    iy, ix = idx // p["w"], idx % p["w"]
    ky = iy - (torch.arange(hp).view(1, 1, hp, 1) * 2 - pad)
    kx = ix - (torch.arange(wp).view(1, 1, 1, wp) * 2 - pad)
    arg = wu.nhwc_np(ky * 3 + kx).astype(np.uint8)
    dz, dzx = wu.pool_sum_values(da, arg, p["pool_y"], p["recs"], groups, pad)
    (gz,) = torch.autograd.grad(pooled, z, wu.nchw64(da))
    gz = wu.nhwc_np(gz * (z > 0))
    xhat = (p["pool_y"].astype(np.float64) - np.repeat(p["recs"][:, :64].astype(np.float64), per, axis=0)[:, None, None, :]) \
        * np.repeat(p["recs"][:, 64:128].astype(np.float64), per, axis=0)[:, None, None, :]
    for g in range(groups):
        sl = slice(g * per, (g + 1) * per)
        assert np.array_equal(dz[sl].sum((0, 1, 2)), gz[sl].sum((0, 1, 2)))
        assert np.array_equal(dzx[sl].sum((0, 1, 2)), (gz[sl] * xhat[sl]).sum((0, 1, 2)))
    assert wu.zero_scale(p["recs"]).sum(1).tolist() == [2] * groups


def test_the_256_cu_size_of_the_56x56_shape_is_exact():
    """n = 22: the exactness conditions of its forward, data-gradient and pooled-block cases (asserted by the makers)."""
    n = wu.big_n(256)
    r = wu.conv_refs("int", 56, 56, n, 2)
    p = wu.pool_operands(56, 56, n, 2, 1)
    wu.assert_pool_exact(r["dx"], wu.pool_forward(p["pool_y"], p["recs"], 2, 1), p["recs"], 2)
    print("largest sum_ci |U||V|: %r" % (r["smax"],))


def test_weight_gradient_partials_add_up_to_the_gradient():
    """wgrad_partials: the workgroups' exact partials, summed and taken through G^T . G, are fp64 autograd's dW (10 x 10, n = 5, at the
    8-CU plan and at a plan with empty slices)."""
    h, w, n = 10, 10, 5
    d, dw = wu.operands("int", h, w, n, 1), wu.conv_refs("int", h, w, n, 1)["dw"]
    for plan in (wu.wgrad_plan(n, h, w, 8), dict(wu.wgrad_plan(n, h, w, 8), grid=32, slices=16, spw=3)):
        part = wu.wgrad_partials(d["x"], d["dy"], plan)
        m = np.zeros((4, 4, 64, 64))
        for b in range(plan["grid"]):
            half = wu.slice_of_workgroup(b, plan["grid"])[1]
            m[:, 2 * half:2 * half + 2] += part[b].reshape(4, 2, 64, 64)
        assert np.array_equal(np.einsum("xa,xyCD,yb->CDab", wu.G, m, wu.G), dw)


@pytest.mark.parametrize("shape", [(4, 4, 1, 1), (6, 10, 3, 3), (16, 20, 3, 3)], ids=wu.shape_id)
def test_the_checks_notice_a_wrong_kernel(shape):
    """Deliberately wrong emulations: the patch operand rounded to 11 significant bits (what a reduced-precision matrix instruction would
    do) exceeds the element bound on random operands; one transform value of one patch off by one is an exact mismatch on integers."""
    h, w, n, groups = shape
    d, r, (wt, b) = wu.operands("rnd", h, w, n, groups), wu.conv_refs("rnd", h, w, n, groups), wu.weights("rnd")

    def short(v):
        m, e = np.frexp(v)
        return np.ldexp(np.rint(m * 2048) / 2048, e).astype(np.float32)

    ratio = wu.worst_ratio(wu.emulate_conv(d["x"], wt, b, spoil=short), r["y"] + b.astype(np.float64),
                           wu.bound_fwd(r["m_x"] + np.abs(b).astype(np.float64)))
    print("RATIO emulation with an 11-bit patch operand %s %.1f" % (wu.shape_id(shape), ratio))
    assert ratio > 1.0

    def off_by_one(v):
        v = v.copy()
        v[-1, -1, -1, 3, 3, 63] += 1
        return v

    di, ri, (wi, _) = wu.operands("int", h, w, n, groups), wu.conv_refs("int", h, w, n, groups), wu.weights("int")
    assert not np.array_equal(wu.emulate_conv(di["x"], wi, spoil=off_by_one).astype(np.float64), ri["y"])


def _ratios(shape, cus=8):
    h, w, n, groups = wu.resolve(shape, cus)
    d, r, (wt, b) = wu.operands("rnd", h, w, n, groups), wu.conv_refs("rnd", h, w, n, groups), wu.weights("rnd")
    out = {"fwd": wu.worst_ratio(wu.emulate_conv(d["x"], wt, b), r["y"] + b.astype(np.float64), wu.bound_fwd(r["m_x"] + np.abs(b).astype(np.float64))),
           "fused": wu.worst_ratio(wu.emulate_conv(d["act"], wt), r["y_fused"], wu.bound_fwd(r["m_act"])),
           "dgrad": wu.worst_ratio(wu.emulate_conv(d["dy"], wu.direction_weights(wt, True)), r["dx"], wu.bound_fwd(r["m_dy"]))}
    return out


@pytest.mark.parametrize("shape", wu.FWD_SHAPES, ids=wu.shape_id)
def test_emulation_sits_inside_the_forward_bounds(shape):
    out = _ratios(shape)
    print("RATIO emulation %s %s" % (wu.shape_id(shape), " ".join("%s %.4f" % kv for kv in sorted(out.items()))))
    assert max(out.values()) < 0.5, out


@pytest.mark.parametrize("shape", wu.WGRAD_SHAPES, ids=wu.shape_id)
def test_emulation_sits_inside_the_weight_gradient_bound(shape):
    for cus in CUS:
        h, w, n = wu.resolve(shape, cus)
        if n * h * w > 2 * 56 * 56:
            continue   # (the 256-CU size of the 56 x 56 shape: 17 248 outer products in numpy; its 8-CU size runs)
        G = wu.wgrad_groups(shape)
        d, spw = wu.operands("rnd", h, w, n, G), wu.wgrad_plan(n, h, w, cus)["spw"]
        ratio = wu.worst_ratio(wu.emulate_wgrad(d["x"], d["dy"], spw), wu.conv_refs("rnd", h, w, n, G)["dw"],
                               wu.bound_wgrad(wu.wgrad_mag(d["x"], d["dy"]), spw))
        print("RATIO emulation wgrad %s cus=%d spw=%d %.4f" % (wu.shape_id(shape), cus, spw, ratio))
        assert ratio < 0.5, ratio


def test_fma32_is_the_fp32_fma():
    """Against exact rational arithmetic on values chosen to sit on and next to fp32 rounding ties."""
    from fractions import Fraction
    rs = np.random.RandomState(1)
    a = rs.standard_normal(2000).astype(np.float32)
    b = rs.standard_normal(2000).astype(np.float32)
    c = rs.standard_normal(2000).astype(np.float32)
    a[:4], b[:4] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23)          # 1 + 2^-22 + 2^-46: just above a tie of the sum below
    c[:4] = np.float32([2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -30])
    got = wu.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))  # (float(Fraction) is correctly rounded to fp64; compare distances instead of trusting it)
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(abs(Fraction(float(v)) - exact) for v in cands)
        assert abs(Fraction(float(got[i])) - exact) == best, i
