"""srlz_dynfit_gram on the GPU, entry by entry through the C ABI: G = sum z zᵀ and C = sum z yᵀ over a list of transitions
(include/srlz.h), a sentinel tail behind G, C and the workspace.

Shapes.  S in {1, 3, 15, 16, 17, 33, 200} (below, on and above a 16-wide tile; several row tiles; more than one group of 8 tiles per
row tile), A in {1, 2, 6, 16, 17} (the one-hot block inside one tile, across two, P on and off a tile's edge), M in {1, 2, r - 1, r,
r + 1, 3 r + 5} with r = srlz_dynfit_chunk_rows(M, S, A) (= 32, one stage, for every M below 8193: asserted).  S decides the tiles
(grid.y), M the chunks (grid.x) and the rows of the last stage, and they meet nowhere in the kernel, so the cases pair every value of
each set with several of the others instead of walking the product; one more case, M = 8200, has two stages per chunk.
What is held:
  1  integers in [-8, 8]: every partial sum is an integer far below 2^53, so G and C equal numpy's int64 result bit for bit, G == G.T,
     a second call into fresh buffers leaves the same bits, the tails are untouched;
  2  floats, N(0, 1) scaled by 1e-2, 1, 1e2 per column, elementwise against numpy's fp64 Zᵀ Z and Zᵀ Y:
     |dev - ref| <= 2 M 2^-52 (|Z|ᵀ |Z|), likewise with |Y| — the first-order bound of ANY summation order (M 2^-53 relative to the
     sum of magnitudes), applied to both sides, with a factor 2 for the second-order terms and the FMA.  Derived, not measured;
  3  every refusal's code with nothing written;
  4  fit_forward's routes "gram" and "torch": equal weight64 on the integers, on the floats within 10 x numpy's own sensitivity to the
     summation order (the host solve on Zᵀ Z against the host solve on the Gram of the row-reversed Z), floor 1e-12 max |weight64|."""
import functools

import numpy as np
import pytest
import torch

import dynfit_util as du

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
TAIL = 64
R = 32

#         S    A   M            order
CASES = [(1, 1, 1, "sorted"),
         (1, 6, 3 * R + 5, "sorted"),
         (3, 2, 2, "sorted"),
         (3, 17, R, "sorted"),
         (15, 1, R + 1, "sorted"),
         (15, 16, R - 1, "sorted"),
         (16, 2, 3 * R + 5, "shuffled"),   # the list in non-monotone order
         (16, 17, 1, "sorted"),
         (17, 6, R, "sorted"),
         (17, 16, 2, "sorted"),
         (33, 1, R - 1, "sorted"),
         (33, 6, R + 1, "sorted"),
         (200, 6, 3 * R + 5, "sorted"),
         (200, 17, R + 1, "sorted"),
         (3, 2, 8200, "sorted")]           # beyond the list: chunks of two stages
IDS = ["S%d_A%d_M%d_%s" % c for c in CASES]
FLOAT_CASES = [(3, 2, 3 * R + 5), (17, 17, R + 1), (33, 6, 3 * R + 5), (200, 6, 3 * R + 5), (3, 2, 8200)]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def recording(s, a, m, order, kind):
    """(states fp32 [N,S], actions int32 [N], starts int32 [M]): the starts a strict subset of the frames with gaps in it (every
    ninth frame closes an episode and starts no transition, every fifth of the rest is left out)."""
    rs = np.random.RandomState(1000 * s + 10 * a + m % 997)
    n = 2 * m + 40
    if kind == "int":
        x = rs.randint(-8, 9, (n, s)).astype(np.float32)
    else:
        x = (rs.randn(n, s) * np.array([1e-2, 1.0, 1e2])[np.arange(s) % 3]).astype(np.float32)
    acts = rs.randint(0, a, n).astype(np.int32)
    frames = np.array([i for i in range(n - 1) if i % 9 != 8 and i % 5 != 3])
    starts = frames[:m].astype(np.int32)
    assert len(starts) == m and len(starts) < n - 1 and (m < 5 or (np.diff(starts) > 1).any())
    if order == "shuffled":
        starts = starts[rs.permutation(m)]
        assert (np.diff(starts) < 0).any()
    return x, acts, starts


def gram(x, acts, starts, a, raw=False, starts_host=None, ws_bytes=None, s_arg=None, a_arg=None):
    """One srlz_dynfit_gram call -> (G [P,P], C [P,S], status); the tails behind G, C and the workspace checked."""
    from srlz import _cabi as C_, ops
    import ctypes
    n, s = x.shape
    m, p = len(starts), s + a + 1
    dev = _dev()
    need = ops.dynfit_workspace(m, s, a)
    assert need > 0 and need % 8 == 0
    bufs = {"G": (p, p), "C": (p, s), "ws": (need // 8,)}
    dev_bufs = {q: torch.full((int(np.prod(shape)) + TAIL,), SENTINEL, dtype=torch.float64, device=dev) for q, shape in bufs.items()}
    d_x, d_a = torch.from_numpy(x).to(dev), torch.from_numpy(acts).to(dev)
    host = np.ascontiguousarray(starts if starts_host is None else starts_host, np.int32)
    d_st = torch.from_numpy(np.ascontiguousarray(starts, np.int32)).to(dev)
    args = [C_.ptr(d_x), C_.ptr(d_a), C_.ptr(d_st), ctypes.c_void_p(host.ctypes.data), n, m, s if s_arg is None else s_arg,
            a if a_arg is None else a_arg, C_.ptr(dev_bufs["G"]), C_.ptr(dev_bufs["C"]), C_.ptr(dev_bufs["ws"]),
            need if ws_bytes is None else ws_bytes, C_.stream()]
    status = C_._lib.srlz_dynfit_gram(*args) if raw else C_.dynfit_gram(*args)
    torch.cuda.synchronize()
    out = {}
    for q, shape in bufs.items():
        h = dev_bufs[q].cpu().numpy()
        assert (h[-TAIL:] == SENTINEL).all(), "%s: sentinel tail overwritten" % q
        out[q] = h[:-TAIL].reshape(shape).copy()
    return out["G"], out["C"], status, out["ws"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integers_match_numpy_int64_bit_for_bit(case):
    from srlz import ops
    s, a, m, order = case
    r = ops.dynfit_chunk_rows(m, s, a)
    assert (r == R and m in (1, 2, r - 1, r, r + 1, 3 * r + 5)) or (m == 8200 and r == 2 * R)
    x, acts, starts = recording(s, a, m, order, "int")
    z, y = du.design(x, acts, starts, a, np.int64)
    g_ref, c_ref = z.T @ z, z.T @ y
    G, C, status, _ = gram(x, acts, starts, a)
    assert status == 0
    np.testing.assert_array_equal(G, g_ref.astype(np.float64))
    np.testing.assert_array_equal(C, c_ref.astype(np.float64))
    np.testing.assert_array_equal(G, G.T)
    assert G[-1, -1] == m  # the constant column counts the transitions
    G2, C2, _, _ = gram(x, acts, starts, a)
    assert np.array_equal(G.view(np.uint64), G2.view(np.uint64)) and np.array_equal(C.view(np.uint64), C2.view(np.uint64))


@pytest.mark.parametrize("case", FLOAT_CASES, ids=["S%d_A%d_M%d" % c for c in FLOAT_CASES])
def test_floats_stay_inside_the_bound_of_any_summation_order(case):
    s, a, m = case
    x, acts, starts = recording(s, a, m, "sorted", "float")
    z, y = du.design(x, acts, starts, a)
    G, C, status, _ = gram(x, acts, starts, a)
    assert status == 0
    u = 2.0 * m * 2.0 ** -52
    worst = 0.0
    for got, ref, mag, q in ((G, z.T @ z, np.abs(z).T @ np.abs(z), "G"), (C, z.T @ y, np.abs(z).T @ np.abs(y), "C")):
        err, bound = np.abs(got - ref), u * mag
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print("%s S%d A%d M%d: largest |dev - ref| / bound = %.3e" % (q, s, a, m, ratio))
        assert (err <= bound).all(), "%s: largest ratio to the bound %.3e" % (q, ratio)
    np.testing.assert_array_equal(G, G.T)
    G2, C2, _, _ = gram(x, acts, starts, a)
    assert np.array_equal(G.view(np.uint64), G2.view(np.uint64)) and np.array_equal(C.view(np.uint64), C2.view(np.uint64))


def test_an_action_out_of_range_gives_a_zero_one_hot_block_on_the_device():
    s, a, m = 17, 6, R + 1
    x, acts, starts = recording(s, a, m, "sorted", "int")
    acts = acts.copy()
    acts[starts[3]], acts[starts[20]] = a, -1
    z, y = du.design(x, acts, starts, a, np.int64)  # (design compares the action with 0 .. A-1: no column answers)
    assert z[3, s:s + a].sum() == 0 and z[20, s:s + a].sum() == 0 and z[4, s:s + a].sum() == 1
    G, C, status, _ = gram(x, acts, starts, a)
    assert status == 0
    np.testing.assert_array_equal(G, (z.T @ z).astype(np.float64))
    np.testing.assert_array_equal(C, (z.T @ y).astype(np.float64))


def test_every_refusal_returns_its_code_and_writes_nothing():
    from srlz import _cabi as C_, ops
    BAD, WORKSPACE = -1, -2
    s, a, m = 17, 6, R + 1
    x, acts, starts = recording(s, a, m, "sorted", "int")
    n = x.shape[0]

    def refused(code, **kw):
        G, C, status, ws = gram(x, acts, starts, a, raw=True, **kw)
        assert status == code, (kw, status)
        assert C_.error_text(), kw
        assert (G == SENTINEL).all() and (C == SENTINEL).all() and (ws == SENTINEL).all(), kw  # nothing launched
    for bad in (n - 1, n, -1):  # the host table is what is checked: the device table stays the valid one
        host = starts.copy()
        host[m // 2] = bad
        refused(BAD, starts_host=host)
    refused(WORKSPACE, ws_bytes=ops.dynfit_workspace(m, s, a) - 1)
    refused(WORKSPACE, ws_bytes=0)
    refused(BAD, s_arg=513)
    refused(BAD, s_arg=0)
    refused(BAD, a_arg=65)
    refused(BAD, a_arg=0)
    with pytest.raises(C_.SrlzError, match="srlz_dynfit_supported"):
        ops.dynfit_gram(torch.zeros((4, 513), device=_dev()), torch.zeros(4, dtype=torch.int32, device=_dev()),
                        torch.zeros(1, dtype=torch.int32), 2)
    with pytest.raises(C_.SrlzError, match="host tensor"):
        ops.dynfit_gram(torch.zeros((4, 3), device=_dev()), torch.zeros(4, dtype=torch.int32, device=_dev()),
                        torch.zeros(1, dtype=torch.int32, device=_dev()), 2)
    with pytest.raises(C_.SrlzError, match="outside"):
        ops.dynfit_gram(torch.zeros((4, 3), device=_dev()), torch.zeros(4, dtype=torch.int32, device=_dev()),
                        torch.tensor([3], dtype=torch.int32), 2)


def _episodes(n, length):
    return (np.arange(n) % length) == 0


def test_routes_gram_and_torch_agree():
    from srlz import dynfit
    s, a, n = 8, 4, 480
    es = _episodes(n, 40)
    rs = np.random.RandomState(11)
    acts = rs.randint(0, a, n)
    # integers: the two routes hand the host solve the same bits
    xi = rs.randint(-8, 9, (n, s)).astype(np.float32)
    g = dynfit.fit_forward(xi, acts, es, route="gram")
    t = dynfit.fit_forward(torch.from_numpy(xi).to(_dev()), acts, es, route="torch")
    assert (g.route, t.route) == ("gram", "torch") and g.count == t.count == n - 12
    np.testing.assert_array_equal(g.gram, t.gram)
    np.testing.assert_array_equal(g.cross, t.cross)
    np.testing.assert_array_equal(g.weight64, t.weight64)
    np.testing.assert_array_equal(g.bias64, t.bias64)
    assert dynfit.fit_forward(xi, acts, es).route == "gram"  # the default where srlz_dynfit_supported says so
    # floats: within 10 x numpy's own sensitivity to the order of the sums
    xf = (rs.randn(n, s) * np.array([1e-2, 1.0, 1e2])[np.arange(s) % 3]).astype(np.float32)
    g, t = dynfit.fit_forward(xf, acts, es, route="gram"), dynfit.fit_forward(xf, acts, es, route="torch")
    z, y = du.design(xf, acts, dynfit.transitions(es), a)
    m = z.shape[0]
    w_fwd, b_fwd = dynfit.solve_forward_head(z.T @ z, z.T @ y, m, s, a, 1e-6)
    zr, yr = z[::-1].copy(), y[::-1].copy()
    w_rev, b_rev = dynfit.solve_forward_head(zr.T @ zr, zr.T @ yr, m, s, a, 1e-6)
    sens = max(np.abs(w_fwd - w_rev).max(), np.abs(b_fwd - b_rev).max())
    allowed = max(10.0 * sens, 1e-12 * np.abs(g.weight64).max())
    diff = max(np.abs(g.weight64 - t.weight64).max(), np.abs(g.bias64 - t.bias64).max())
    print("routes gram / torch on floats: |difference| %.3e, numpy's own sensitivity %.3e, ratio to the allowed %.3e"
          % (diff, sens, diff / allowed))
    assert diff <= allowed, "ratio to the allowed difference %.3e" % (diff / allowed)
    host = max(np.abs(g.weight64 - w_fwd).max(), np.abs(g.bias64 - b_fwd).max())
    assert host <= allowed, "against the host solve: ratio %.3e" % (host / allowed)
