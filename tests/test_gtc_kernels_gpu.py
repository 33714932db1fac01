"""srlz_gtc_rows_f64 (csrc/gtc.hip) against numpy's own corrcoef in extended precision, np.corrcoef(gt, states, rowvar=0,
dtype=np.longdouble)[:G], computed here: every coefficient within (4 N + 16) 2^-53 absolute (tests/gtc_util.py::bound — three
length-N fp64 sums of relative error <= N u each, the mean's second-order term, a few roundings for the square roots and divisions),
the column means and variances within the same figure relative to each value.  (tests/test_gtc_host_cpu.py shows that the one-pass
form sum x^2 - (sum x)^2 / N misses that bound by orders of magnitude on the two offset cases.)  Output buffers and the workspace
carry sentinel tails that must survive."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gtc_util as gu

pytestmark = pytest.mark.gpu

TAIL = 64
CORR_SENTINEL, STAT_SENTINEL, WS_SENTINEL = -7.5, -3.25, 0xAB


def run_gtc(gt, states):
    """One call through the C ABI on fp64 device copies. :return: (corr float64 [G, G + S], colstats float64 [2, G + S])"""
    from srlz import _cabi as C
    dev = torch.device("cuda", 0)
    gt_d = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float64)).to(dev)
    st_d = torch.from_numpy(np.ascontiguousarray(states, dtype=np.float64)).to(dev)
    (n, g), s = gt_d.shape, st_d.shape[1]
    c = g + s
    corr = torch.full((g * c + TAIL,), CORR_SENTINEL, dtype=torch.float64, device=dev)
    colstats = torch.full((2 * c + TAIL,), STAT_SENTINEL, dtype=torch.float64, device=dev)
    nbytes = C.gtc_workspace(n, g, s)
    assert nbytes > 0
    ws = torch.full((nbytes + TAIL,), WS_SENTINEL, dtype=torch.uint8, device=dev)
    C.gtc_rows_f64(C.ptr(gt_d), C.ptr(st_d), n, g, s, C.ptr(corr), C.ptr(colstats), C.ptr(ws), nbytes, C.stream())
    torch.cuda.synchronize()
    assert (corr[g * c:] == CORR_SENTINEL).all() and (colstats[2 * c:] == STAT_SENTINEL).all() and (ws[nbytes:] == WS_SENTINEL).all()
    return corr[:g * c].view(g, c).cpu().numpy(), colstats[:2 * c].view(2, c).cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded_case(n, g, s, dtype, kind):
    """(gt, states, reference corr, reference colstats) of a seeded case; the reference is computed once and shared."""
    gt, states = gu.kernel_input(n, g, s, dtype, kind)
    return (gt, states) + gu.reference_rows(gt, states)


def check(got, ref, n):
    (corr, colstats), (rcorr, rstats) = got, ref
    assert corr.shape == rcorr.shape and colstats.shape == rstats.shape
    nan = np.isnan(rcorr)
    assert np.array_equal(np.isnan(corr), nan), "NaN at %s, numpy has it at %s" % (np.argwhere(np.isnan(corr)).tolist(),
                                                                                 np.argwhere(nan).tolist())
    err = np.abs(corr.astype(np.longdouble) - rcorr)[~nan]
    worst = float(err.max()) if err.size else 0.0
    print("N %d: worst coefficient error %.3e (bound %.3e)" % (n, worst, gu.bound(n)))
    assert worst <= gu.bound(n), (worst, gu.bound(n))
    assert (np.abs(corr[~nan]) <= 1.0).all()
    rel = np.abs(colstats.astype(np.longdouble) - rstats)
    limit = gu.bound(n) * np.abs(rstats)
    print("N %d: worst column-statistic error / value %.3e" % (n, float((rel[rstats != 0] / np.abs(rstats[rstats != 0])).max())))
    assert (rel <= limit).all(), (float((rel - limit).max()), np.argwhere(rel > limit).tolist())


@pytest.mark.parametrize("n,g,s,dtype,kind", gu.KERNEL_CASES)
def test_seeded_cases(n, g, s, dtype, kind):
    gt, states, rcorr, rstats = seeded_case(n, g, s, dtype, kind)
    assert states.dtype == {"f32": np.float32, "f64": np.float64}[dtype]
    check(run_gtc(gt, states), (rcorr, rstats), n)


def test_calls_repeat_bit_for_bit():
    gt, states, _, _ = seeded_case(1025, 3, 200, "f32", "plain")
    a, b = run_gtc(gt, states), run_gtc(gt, states)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def test_zero_variance_columns_give_nan_where_numpy_does():
    """A constant state column and a constant ground-truth column.  The constants are powers of two: every partial sum of such a column
    is exact in any order, so its centred values are exactly 0 here as in numpy, the variance is 0 and the entries are 0 / 0."""
    n, g, s = 1025, 3, 70
    gt, states = gu.kernel_input(n, g, s, "f32", "plain")
    gt, states = gt.copy(), states.copy()
    gt[:, 1] = 0.5
    states[:, 66] = -2.0
    rcorr, rstats = gu.reference_rows(gt, states)
    want = np.zeros((g, g + s), dtype=bool)
    want[1, :] = True
    want[:, 1] = True
    want[:, g + 66] = True
    assert np.array_equal(np.isnan(rcorr), want)
    corr, colstats = run_gtc(gt, states)
    check((corr, colstats), (rcorr, rstats), n)
    assert colstats[1, 1] == 0.0 and colstats[1, g + 66] == 0.0 and colstats[0, 1] == 0.5 and colstats[0, g + 66] == -2.0
    # ... and through the binding, which raises nothing for it
    from srlz import ops
    oc = ops.gt_correlation(gt, states)
    assert oc.dtype == np.float64 and np.array_equal(oc.view(np.int64), corr.view(np.int64))


def test_binding_converts_float32_exactly_and_returns_the_kernel_rows():
    from srlz import ops
    gt, states, rcorr, rstats = seeded_case(63, 3, 65, "f32", "plain")
    corr, colstats = run_gtc(gt, states)
    oc = ops.gt_correlation(gt, torch.from_numpy(states))
    assert oc.shape == (3, 68) and oc.dtype == np.float64 and np.array_equal(oc.view(np.int64), corr.view(np.int64))


def test_bad_arguments_are_rejected_before_any_launch(cabi):
    dev = torch.device("cuda", 0)
    n, g, s = 40, 3, 5
    gt_h, st_h = gu.kernel_input(n, g, s, "f64", "plain")
    gt, st = torch.from_numpy(gt_h).to(dev), torch.from_numpy(st_h).to(dev)
    corr = torch.full((17 * 22,), CORR_SENTINEL, dtype=torch.float64, device=dev)
    colstats = torch.full((2 * 22,), STAT_SENTINEL, dtype=torch.float64, device=dev)
    nbytes = cabi.gtc_workspace(n, g, s)
    assert nbytes > 0
    ws = torch.full((nbytes,), WS_SENTINEL, dtype=torch.uint8, device=dev)
    P, raw = cabi.ptr, cabi._lib.srlz_gtc_rows_f64
    good = dict(gt=P(gt), states=P(st), N=n, G=g, S=s, corr=P(corr), colstats=P(colstats), ws=P(ws), ws_bytes=nbytes)

    def call(**change):
        a = dict(good, **change)
        return raw(a["gt"], a["states"], a["N"], a["G"], a["S"], a["corr"], a["colstats"], a["ws"], ctypes.c_size_t(a["ws_bytes"]),
                   cabi.stream())
    NULL, BAD, WSP = -4, -1, -2
    for name in ("gt", "states", "corr", "colstats", "ws"):
        assert call(**{name: None}) == NULL, name
        assert "null" in cabi.error_text()
    assert call(N=1) == BAD and call(N=0) == BAD and call(N=-4) == BAD
    assert call(G=17) == BAD and call(G=0) == BAD
    assert call(S=0) == BAD and call(S=-1) == BAD
    assert call(N=1 << 20, S=(1 << 11) - g) == BAD  # N * (G + S) = 2^31
    assert "2^31" in cabi.error_text()
    assert call(ws_bytes=nbytes - 1) == WSP and call(ws_bytes=0) == WSP
    assert "workspace" in cabi.error_text()
    assert cabi.gtc_workspace(1, g, s) == 0 and cabi.gtc_workspace(n, 17, s) == 0 and cabi.gtc_workspace(n, g, 0) == 0
    assert cabi.gtc_workspace(1 << 20, g, (1 << 11) - g) == 0
    torch.cuda.synchronize()
    assert (corr == CORR_SENTINEL).all() and (colstats == STAT_SENTINEL).all() and (ws == WS_SENTINEL).all()  # nothing was launched
    assert call() == 0  # and the same arguments unchanged do run
    torch.cuda.synchronize()
    rcorr, _ = gu.reference_rows(gt_h, st_h)
    assert float(np.abs(corr[:g * (g + s)].view(g, g + s).cpu().numpy() - rcorr).max()) <= gu.bound(n)
