"""srlz_knn_f64 (csrc/knn.hip) against the numpy oracle tests/knn_util.py::brute_knn — which tests/test_eval_host_cpu.py ties to the
reference's ball tree: indices exactly, squared distances to 1e-12 relative (the kernel's chain uses fma, the oracle a separate
multiply and add: at most D roundings of 1.1e-16 apart).  Output buffers and the workspace carry sentinel tails that must survive."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import knn_util as ku

pytestmark = pytest.mark.gpu

TAIL = 64
IDX_SENTINEL, DIST_SENTINEL, WS_SENTINEL = -12345, -7.5, 0xAB


def run_knn(db, queries, k):
    """One call through the C ABI on fp64 device copies. :return: (idx int64 [Q, k], dist2 float64 [Q, k])"""
    from srlz import _cabi as C
    dev = torch.device("cuda", 0)
    db_d = torch.from_numpy(np.ascontiguousarray(db, dtype=np.float64)).to(dev)
    q_d = db_d if queries is None else torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float64)).to(dev)
    n, d = db_d.shape
    nq = q_d.shape[0]
    idx = torch.full((nq * k + TAIL,), IDX_SENTINEL, dtype=torch.int32, device=dev)
    dist2 = torch.full((nq * k + TAIL,), DIST_SENTINEL, dtype=torch.float64, device=dev)
    nbytes = C.knn_workspace(n, nq, d, k)
    assert nbytes > 0
    ws = torch.full((nbytes + TAIL,), WS_SENTINEL, dtype=torch.uint8, device=dev)
    C.knn_f64(C.ptr(db_d), n, C.ptr(q_d), nq, d, k, C.ptr(idx), C.ptr(dist2), C.ptr(ws), nbytes, C.stream())
    torch.cuda.synchronize()
    assert (idx[nq * k:] == IDX_SENTINEL).all() and (dist2[nq * k:] == DIST_SENTINEL).all() and (ws[nbytes:] == WS_SENTINEL).all()
    return idx[:nq * k].view(nq, k).cpu().numpy().astype(np.int64), dist2[:nq * k].view(nq, k).cpu().numpy()


def check(got, ref):
    (gi, gd), (ri, rd) = got, ref
    assert np.array_equal(gi, ri), "first differing row %d: %s vs %s" % (
        np.nonzero((gi != ri).any(1))[0][0], gi[(gi != ri).any(1)][0], ri[(gi != ri).any(1)][0])
    zero = rd == 0
    assert (gd[zero] == 0).all()
    err = np.abs(gd[~zero] - rd[~zero]) / rd[~zero]
    assert err.size == 0 or err.max() <= 1e-12, err.max()


SEVEN = [0, 1, 64, 511, 1023, 1029, 1030]


@functools.lru_cache(maxsize=None)
def seeded_case(n, d, q, k):
    """(db, queries or None, oracle) of a seeded case; the oracle is computed once and shared."""
    db = ku.seeded_input(n, d)
    if q == n:
        queries = None
    elif (n, q) == (1031, 7):
        queries = db[SEVEN]
    else:
        queries = db[:q]
    return db, queries, ku.brute_knn(db, db if queries is None else queries, k)


@pytest.mark.parametrize("n,d,q,k", [(1031, 200, 1031, 6), (1031, 200, 7, 6), (257, 3, 257, 6), (2049, 7, 200, 32), (300, 65, 300, 1),
                                     (5, 3, 5, 5), (1, 1, 1, 1)])
def test_seeded_cases(n, d, q, k):
    db, queries, ref = seeded_case(n, d, q, k)
    check(run_knn(db, queries, k), ref)


def test_several_row_tiles_per_workgroup():
    """N = 5000 against 37 queries: 157 database splits of 32 rows, i.e. TWO 16-row tiles per workgroup (every shape above has one),
    and D = 70 = one full 64-dimension tile + 6.  Minimum relative gap of the 8 smallest distances of these rows: 1.9e-5."""
    db = ku.seeded_input(5000, 70)
    queries = db[::137][:37]
    check(run_knn(db, queries, 6), ku.brute_knn(db, queries, 6))


def test_rows_do_not_depend_on_the_query_set_and_calls_repeat():
    db, _, _ = seeded_case(1031, 200, 1031, 6)
    all_i, all_d = run_knn(db, None, 6)
    sev_i, sev_d = run_knn(db, db[SEVEN], 6)
    assert np.array_equal(sev_i, all_i[SEVEN]) and np.array_equal(sev_d.view(np.int64), all_d[SEVEN].view(np.int64))
    again_i, again_d = run_knn(db, None, 6)
    assert np.array_equal(again_i, all_i) and np.array_equal(again_d.view(np.int64), all_d.view(np.int64))


@pytest.mark.parametrize("duplicates", [False, True])
def test_ties_go_to_the_lower_index(duplicates):
    """The integer lattice {0..31}^2: every distance a small integer, exact in any order, ties everywhere.  With rows 3 and 900
    overwritten by row 17: duplicates, and the self-match of rows 17 and 900 is not the first entry."""
    yy, xx = np.mgrid[0:32, 0:32]
    db = np.stack([yy.ravel(), xx.ravel()], 1).astype(np.float64)
    if duplicates:
        db[3] = db[17]
        db[900] = db[17]
    ref = ku.brute_knn(db, db, 32)
    gi, gd = run_knn(db, None, 32)
    assert np.array_equal(gi, ref[0]) and np.array_equal(gd, ref[1])
    # the rule itself, not only the oracle: ascending (dist2, index)
    for r in (0, 17, 500, 900, 1023):
        d2 = ((db - db[r]) ** 2).sum(1)
        order = sorted(range(1024), key=lambda j: (d2[j], j))[:32]
        assert list(gi[r]) == order
    if duplicates:
        assert list(gi[900][:3]) == [3, 17, 900] and list(gi[17][:3]) == [3, 17, 900] and (gd[900][:3] == 0).all()


def test_float64_input_is_not_rounded():
    db = np.random.RandomState(11).randn(300, 3)
    assert not np.array_equal(db, db.astype(np.float32))
    check(run_knn(db, None, 6), ku.brute_knn(db, db, 6))
    # ... and through the binding, which uploads fp64 as it is
    from srlz import ops
    oi, od = ops.knn(db, 6)
    assert oi.dtype == np.int64 and od.dtype == np.float64
    check((oi, od), ku.brute_knn(db, db, 6))


def test_queries_that_are_not_database_rows():
    db = ku.seeded_input(1000, 2)
    queries = np.random.RandomState(12).randn(33, 2).astype(np.float32)
    ref = ku.brute_knn(db, queries, 6)
    check(run_knn(db, queries, 6), ref)
    from srlz import ops
    check(ops.knn(torch.from_numpy(db), 6, queries=queries), ref)


def test_bad_arguments_are_rejected_before_any_launch(cabi):
    dev = torch.device("cuda", 0)
    n, d, q, k = 40, 3, 9, 4
    db = torch.from_numpy(ku.seeded_input(n, d).astype(np.float64)).to(dev)
    idx = torch.full((q * 32,), IDX_SENTINEL, dtype=torch.int32, device=dev)
    dist2 = torch.full((q * 32,), DIST_SENTINEL, dtype=torch.float64, device=dev)
    nbytes = cabi.knn_workspace(n, q, d, k)
    ws = torch.full((max(nbytes, cabi.knn_workspace(n, q, d, 32)),), WS_SENTINEL, dtype=torch.uint8, device=dev)
    P, raw = cabi.ptr, cabi._lib.srlz_knn_f64
    good = dict(db=P(db), N=n, queries=P(db), Q=q, D=d, K=k, idx=P(idx), dist2=P(dist2), ws=P(ws), ws_bytes=ws.numel())

    def call(**change):
        a = dict(good, **change)
        return raw(a["db"], a["N"], a["queries"], a["Q"], a["D"], a["K"], a["idx"], a["dist2"], a["ws"], ctypes.c_size_t(a["ws_bytes"]),
                   cabi.stream())
    NULL, BAD, WSP = -4, -1, -2
    for name in ("db", "queries", "idx", "dist2", "ws"):
        assert call(**{name: None}) == NULL, name
        assert "null" in cabi.error_text()
    assert call(K=0) == BAD and call(K=-3) == BAD
    assert call(K=33) == BAD
    assert call(K=32, N=31) == BAD and call(K=n + 1) == BAD  # K > N
    assert call(D=0) == BAD and call(D=-1) == BAD
    assert call(Q=0) == BAD and call(Q=-5) == BAD
    assert call(N=1 << 20, D=1 << 11) == BAD       # N * D = 2^31
    assert call(Q=1 << 27, K=16) == BAD            # Q * K = 2^31
    assert "2^31" in cabi.error_text()
    assert call(ws_bytes=nbytes - 1) == WSP and call(ws_bytes=0) == WSP
    assert "workspace" in cabi.error_text()
    assert cabi.knn_workspace(n, q, d, 33) == 0 and cabi.knn_workspace(n, 0, d, k) == 0 and cabi.knn_workspace(1 << 20, q, 1 << 11, k) == 0
    torch.cuda.synchronize()
    assert (idx == IDX_SENTINEL).all() and (dist2 == DIST_SENTINEL).all() and (ws == WS_SENTINEL).all()  # nothing was launched
    assert call() == 0  # and the same arguments unchanged do run
    torch.cuda.synchronize()
    ref = ku.brute_knn(db.cpu().numpy(), db.cpu().numpy()[:q], k)
    assert np.array_equal(idx[:q * k].view(q, k).cpu().numpy(), ref[0])
