"""The nn.Linear GEMM (csrc/linear.hip) route by route (GPU): gemm_strided_kernel, the three gemm_vec_kernel instantiations, the
split-K combine, colsum_kernel and relu_bwd_kernel — the five C entry points called by name.

Every GEMM case first asks srlz_linear_debug_route which kernel and how many reduction chunks its call will take and asserts that
answer against the route in its own id, so a case cannot quietly test another kernel.  The workspace is pre-filled with a NaN bit
pattern no partial sum can have: after the call exactly the first nz * I * J floats have changed (none when nz = 1) — the query checked
against the launch that happened.  Outputs are NaN before the call and sit between NaN sentinels that must come back untouched.

Two CPU references per case:
  * integer-exact: every operand an integer of [-4, 4] in fp32.  Every partial sum stays below 2304 * 16 < 2^24, so any order of fp32
    accumulation is exact and the result equals numpy's int64 result bit for bit;
  * random (randn, weights x 0.1) against fp64, element by element:
        |got - ref| <= 1.01 (R + 21) 2^-24 (sum_r |a_ir| |b_rj| + |bias_j| + |res_ij|) + R 2^-126
    — an fp32 fma chain of R terms (gamma_R), at most 16 combine adds, a bias add and a residual add.  Derived, not measured.

Largest error / bound seen on an MI355X, per kernel and split mode (printed by every case as a "RATIO" line):
                 strided   vec<0,0>   vec<0,1>   vec<1,1>
    nz = 1        0.114     0.081      0.099      0.082
    nz > 1        0.0030    0.0027     0.0029     0.0031      (R >= 512: the bound grows with R, the error of a sum like sqrt R)
    colsum 0.183; through srlz.ops at M = 512: y 0.0071, next_state 0.017, dx 0.114, dstate 0.020, dw 0.0026, db 0.0005
None is near 1: the kernels are as accurate as an fp32 fma chain has to be, with room to reorder k.
"""
import functools

import numpy as np
import pytest
import torch

from test_kernels_gpu import C, DEV  # noqa: F401  (C: the module-scoped fixture of the kernel tests)
from test_linear_routes_cpu import (BWD_DATA, BWD_WEIGHT, DEFAULT, FWD, KERNEL_NAME, STRIDED, VEC_IJ, VEC_RJ, VEC_RR, gemm_shape,
                                    replay_kernel, route)
from test_update_path_gpu import GUARD, NAN, guarded, same_bits, tail_intact

pytestmark = pytest.mark.gpu

WS_SENTINEL = 0x7FC0BEEF  # a NaN with a payload: no sum of finite numbers has these bits
U = 2.0 ** -24
OP = {"fwd": FWD, "fwd_res": FWD, "bwd_data": BWD_DATA, "bwd_data_res": BWD_DATA, "bwd_weight": BWD_WEIGHT}


# ---- inputs (made once per shape and kind, never modified) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_data(M, N, K, kind):
    """x [M,K], w [N,K], bias [N], dy [M,N], res_y [M,N], res_dx [M,K] as fp32 numpy arrays: small integers, or randn (w x 0.1)."""
    rs = np.random.RandomState(1000003 * M + 1009 * N + K + (7 if kind == "int" else 0))
    shapes = {"x": (M, K), "w": (N, K), "bias": (N,), "dy": (M, N), "res_y": (M, N), "res_dx": (M, K)}
    d = {}
    for name, shape in shapes.items():
        if kind == "int":
            d[name] = rs.randint(-4, 5, size=shape).astype(np.float32)
        else:
            d[name] = (rs.standard_normal(shape) * (0.1 if name == "w" else 1.0)).astype(np.float32)
        d[name].setflags(write=False)
    return d


def operands(entry, d, Kout, bias):
    """(A [I,R], B [R,J], bias [J] or None, res [I,J] or None) of the GEMM an entry point states, as fp32 numpy arrays."""
    if entry in ("fwd", "fwd_res"):
        return d["x"], d["w"].T, (d["bias"] if bias else None), (d["res_y"] if entry == "fwd_res" else None)
    if entry in ("bwd_data", "bwd_data_res"):
        return d["dy"], d["w"][:, :Kout], None, (np.ascontiguousarray(d["res_dx"][:, :Kout]) if entry == "bwd_data_res" else None)
    return d["dy"].T, d["x"], None, None


def reference(A, B, bias, res, relu, dtype):
    """C = A . B (+ bias) (ReLU) (+ res) in `dtype` (int64: exact; float64), and for float64 the magnitude the error bound scales with."""
    v = A.astype(dtype) @ B.astype(dtype)
    if bias is not None:
        v = v + bias.astype(dtype)
    if relu:
        v = np.maximum(v, 0)
    if res is not None:
        v = v + res.astype(dtype)
    if dtype is np.int64:
        return v, None
    mag = np.abs(A).astype(dtype) @ np.abs(B).astype(dtype)
    if bias is not None:
        mag = mag + np.abs(bias).astype(dtype)
    if res is not None:
        mag = mag + np.abs(res).astype(dtype)
    return v, mag


def gemm_bound(mag, R):
    return 1.01 * (R + 21) * U * mag + R * 2.0 ** -126


def worst_ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


# ---- device buffers ----------------------------------------------------------------------------------------------------------------
def put(src, off=0):
    """Device copy of a numpy array starting `off` bytes behind a 16-byte boundary (a [off/4:] view of a longer buffer)."""
    k, n = off // 4, src.size
    whole = torch.full((n + k,), NAN, device=DEV)
    view = whole[k:].view(src.shape)
    view.copy_(torch.from_numpy(np.array(src, dtype=np.float32)))  # (a writable copy: the cached inputs are read-only)
    assert view.data_ptr() % 16 == off
    return view


class Out:
    """An output of NaNs between NaN sentinels, `off` bytes behind a 16-byte boundary."""

    def __init__(self, shape, off=0):
        self.k, self.n = off // 4, int(np.prod(shape))
        self.whole = torch.full((self.k + self.n + GUARD,), NAN, device=DEV)
        self.view = self.whole[self.k:self.k + self.n].view(shape)
        assert self.view.data_ptr() % 16 == off

    def result(self):
        """The payload as a numpy array; the sentinels before and behind it must be intact."""
        assert bool(torch.isnan(self.whole[:self.k]).all()) and tail_intact(self.whole[self.k:], self.n)
        return self.view.cpu().numpy()


class Workspace:
    """`nbytes` of workspace (None: the call passes no workspace) filled with WS_SENTINEL, and GUARD more words behind it."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.words = None if nbytes is None else torch.full(((nbytes + 3) // 4 + GUARD,), WS_SENTINEL, dtype=torch.int32, device=DEV)

    def args(self, C):
        return (None, 0) if self.words is None else (C.ptr(self.words), self.nbytes)

    def check(self, nz, I, J):
        """Exactly the first nz * I * J floats were written (none for nz = 1)."""
        if self.words is None:
            assert nz == 1
            return
        used = nz * I * J if nz > 1 else 0
        assert used * 4 <= self.nbytes
        assert bool((self.words[:used] != WS_SENTINEL).all()), "a partial tile the route query promised was not written"
        assert bool((self.words[used:] == WS_SENTINEL).all()), "the workspace was written behind nz * I * J floats"


def call(C, entry, M, N, K, d, Kout=None, relu=0, ws=DEFAULT, offs=None, bias=True, expect=None, want_db=True, alias_res=False):
    """One call of an entry point on device copies of d.  Asserts the route (query against `expect` = (kernel, nz), the workspace against
    the query) and every sentinel.  Returns (result, db or None, (kernel, nz, rchunk))."""
    offs = offs or {}
    op = OP[entry]
    Kout = K if Kout is None else Kout
    I, J, R = gemm_shape(op, M, N, K, Kout)
    a = put(d["dy"] if op != FWD else d["x"], offs.get("a", 0))
    b = put(d["x"] if op == BWD_WEIGHT else d["w"], offs.get("b", 0))
    nbytes = C.linear_workspace(M, N, K) if ws == DEFAULT else ws
    plan = route(C, op, M, N, K, Kout, a.data_ptr(), b.data_ptr(), nbytes)
    if expect is not None:
        assert plan[:2] == tuple(expect), "route (kernel, nz) is %r, the case is written for %r" % (plan[:2], tuple(expect))
    W = Workspace(nbytes)
    out = Out((I, J), offs.get("out", 0))
    st = C.stream()
    db = None
    if entry in ("fwd", "fwd_res"):
        bd = put(d["bias"], offs.get("bias", 0)) if bias else None
        if entry == "fwd":
            C.linear_fwd(C.ptr(a), C.ptr(b), C.ptr(bd), C.ptr(out.view), M, N, K, relu, *W.args(C), st)
        else:
            res = put(d["res_y"], offs.get("res", 0))
            C.linear_fwd_res(C.ptr(a), C.ptr(b), C.ptr(bd), C.ptr(res), C.ptr(out.view), M, N, K, relu, *W.args(C), st)
    elif entry == "bwd_data":
        assert Kout == K
        C.linear_bwd_data(C.ptr(a), C.ptr(b), C.ptr(out.view), M, N, K, *W.args(C), st)
    elif entry == "bwd_data_res":
        res = a if alias_res else put(np.ascontiguousarray(d["res_dx"][:, :Kout]), offs.get("res", 0))
        C.linear_bwd_data_res(C.ptr(a), C.ptr(b), C.ptr(res), C.ptr(out.view), M, N, K, Kout, *W.args(C), st)
    else:
        db = Out((N,), offs.get("bias", 0)) if want_db else None
        C.linear_bwd_weight(C.ptr(a), C.ptr(b), C.ptr(out.view), C.ptr(db.view) if db else None, M, N, K, *W.args(C), st)
    torch.cuda.synchronize()
    W.check(plan[1], I, J)
    return out.result(), (db.result() if db else None), plan


def check_colsum(d_int, d_rnd, got_int, got_rnd, M):
    """db = column sums of dy: integers bit for bit; random within 1.01 (M + 4) 2^-24 sum_m |dy_mn| (M - 1 adds in four chains of four
    accumulators each, then four adds to join them)."""
    assert same_bits(torch.from_numpy(got_int), d_int["dy"].astype(np.int64).sum(0).astype(np.float32))
    dy = d_rnd["dy"].astype(np.float64)
    bound = 1.01 * (M + 4) * U * np.abs(dy).sum(0)
    err = np.abs(got_rnd.astype(np.float64) - dy.sum(0))
    assert (err <= bound).all(), float((err / bound).max())
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
def from_ijr(op, I, J, R):
    """(M, N, K) of the entry point whose GEMM has an I x J result and a reduction of R."""
    return {FWD: (I, J, R), BWD_DATA: (I, R, J), BWD_WEIGHT: (R, I, J)}[op]


def G(entry, M, N, K, nz=1, Kout=None, relu=0, ws=DEFAULT, offs=None, bias=True, tag=""):
    """One row of the sweep.  The kernel in the id comes from the replay of the vectorisation predicate in test_linear_routes_cpu, nz
    from the row; the test asserts both against the route query before it launches."""
    offs = offs or {}
    kernel = replay_kernel(OP[entry], M, N, K, Kout, 4096 + offs.get("a", 0), 4096 + offs.get("b", 0))
    name = "%s-%dx%dx%d" % (entry, M, N, K)
    if Kout is not None:
        name += "-kout%d" % Kout
    if relu:
        name += "-relu"
    if not bias:
        name += "-nobias"
    if ws != DEFAULT:
        name += "-ws%s" % ws
    for key in sorted(offs):
        name += "-%s+%d" % (key, offs[key])
    if tag:
        name += "-" + tag
    name += "-%s-nz%d" % (KERNEL_NAME[kernel], nz)
    return pytest.param(entry, M, N, K, kernel, nz, Kout, relu, ws, offs, bias, id=name)


def sweep():
    rows = []
    pairs = [(63, 65), (65, 63), (1, 130), (130, 1), (31, 64), (64, 31), (64, 64), (65, 65)]
    vec_pairs_j4 = [(63, 68), (65, 60), (1, 132), (130, 4), (64, 64)]  # the data gradient's vec route needs J % 4 == 0

    def both_relu(entry, M, N, K, **kw):
        return [G(entry, M, N, K, relu=0, **kw), G(entry, M, N, K, relu=1, **kw)]

    # tile edges on the strided route (R = 33, 65: one past a step) and on the vec routes (R = 68: one float4 past a step)
    for I, J in pairs:
        for R in (33, 65) if (I, J) in ((63, 65), (65, 63), (64, 64)) else (33,):
            rows += both_relu("fwd", *from_ijr(FWD, I, J, R))
            rows += [G("bwd_data", *from_ijr(BWD_DATA, I, J, R)), G("bwd_weight", *from_ijr(BWD_WEIGHT, I, J, R))]
        rows += both_relu("fwd_res", *from_ijr(FWD, I, J, 33))
        rows += [G("bwd_data_res", *from_ijr(BWD_DATA, I, J, 33))]
        rows += both_relu("fwd", *from_ijr(FWD, I, J, 68)) + both_relu("fwd_res", *from_ijr(FWD, I, J, 68))
    for I, J in vec_pairs_j4:
        rows += [G("bwd_data", *from_ijr(BWD_DATA, I, J, 68)), G("bwd_data_res", *from_ijr(BWD_DATA, I, J, 68))]
    # the weight gradient's along_row loaders: a last group of four rows at, before and behind the tile edge, both operands
    for n in (4, 60, 64, 68):
        for k in (4, 60, 64, 68):
            rows.append(G("bwd_weight", 68, n, k))
    # reduction lengths around the strided kernel's steps of 32 ...
    for R in (1, 2, 31, 32, 33, 65, 206):
        # (a forward GEMM with K % 4 == 0 is a vec case unless an operand is misaligned)
        rows += both_relu("fwd", 65, 63, R, offs={"a": 4} if R % 4 == 0 else None)
        rows += [G("bwd_data", *from_ijr(BWD_DATA, 63, 65, R)), G("bwd_weight", *from_ijr(BWD_WEIGHT, 65, 63, R))]
    # ... and around the vec kernels' steps of 64
    for R in (4, 60, 64, 68, 128, 132):
        rows += both_relu("fwd", 63, 65, R)
        rows += [G("bwd_data", *from_ijr(BWD_DATA, 65, 68, R)), G("bwd_weight", *from_ijr(BWD_WEIGHT, 60, 68, R))]
    # split-K: the model's layers at batch 256 (both frames as one batch: M = 512), every direction of each shape
    rows += both_relu("fwd", 256, 200, 2304, nz=12) + both_relu("fwd_res", 256, 200, 2304, nz=12)
    rows += [G("bwd_data", 256, 200, 2304), G("bwd_weight", 256, 200, 2304)]
    rows += [G("bwd_data", 512, 2304, 200, nz=12), G("bwd_data_res", 512, 2304, 200, nz=12), G("fwd", 512, 2304, 200),
             G("bwd_weight", 512, 2304, 200)]
    rows += [G("bwd_weight", 512, 6, 400, nz=4), G("fwd", 512, 6, 400), G("bwd_data", 512, 6, 400)]
    rows += [G("bwd_weight", 512, 200, 206, nz=4), G("fwd_res", 512, 200, 206), G("bwd_data_res", 512, 200, 206, Kout=200)]
    rows += [G("fwd", 3, 200, 206)]
    # ... the chunk rounded up to a step: 516 asks for 4 splits and gets 3 chunks of 192; 515 goes strided with 4 chunks of 160;
    # 508 < 512 is not split; 640 gives 5 chunks of 128
    for K, nz in ((512, 4), (516, 3), (515, 4), (508, 1), (640, 5)):
        rows += both_relu("fwd", 64, 64, K, nz=nz) + both_relu("fwd_res", 64, 64, K, nz=nz)
    for N, nz in ((512, 4), (516, 3), (515, 4)):
        rows += [G("bwd_data", 64, N, 64, nz=nz), G("bwd_data_res", 64, N, 64, nz=nz), G("bwd_weight", N, 64, 64, nz=nz)]
    rows += [G("bwd_data_res", 63, 515, 65, nz=4), G("bwd_weight", 515, 63, 65, nz=4), G("bwd_weight", 516, 60, 68, nz=3)]
    # ... a workspace too small for the wanted split (12 chunks of 192 with the default one), and none
    rows += [G("fwd", 64, 64, 2304, nz=12), G("fwd", 64, 64, 2304, nz=5, ws=5 * 64 * 64 * 4), G("fwd", 64, 64, 2304, ws=2 * 64 * 64 * 4 - 1),
             G("fwd", 64, 64, 2304, ws=None), G("fwd_res", 64, 64, 2304, nz=5, ws=5 * 64 * 64 * 4, relu=1),
             G("bwd_weight", 512, 6, 400, ws=None), G("bwd_weight", 512, 6, 400, nz=2, ws=2 * 6 * 400 * 4 + 3),
             G("bwd_data_res", 64, 2304, 64, nz=5, ws=5 * 64 * 64 * 4)]
    # the data gradient of the first Kout input columns (J = Kout columns of a K-wide w); Kout = 1 is never a vec case
    for M, N, K, Kout in ((5, 64, 72, 68), (65, 128, 136, 64), (3, 200, 206, 200), (65, 10, 14, 10)):
        for ko in (Kout, K, 1):
            rows.append(G("bwd_data_res", M, N, K, Kout=ko))
    rows += [G("bwd_data_res", 4, 512, 516, nz=4, Kout=512), G("bwd_data_res", 5, 515, 14, nz=4, Kout=10)]
    # degenerate strides: a leading dimension of 1 that makes the "other" stride 1 too
    for M, N, K in ((5, 1, 7), (5, 7, 1), (1, 5, 7), (1, 1, 1), (8, 1, 8), (1, 8, 8), (8, 8, 1), (4, 4, 4), (68, 1, 64), (1, 68, 64)):
        rows += both_relu("fwd", M, N, K) + [G("fwd_res", M, N, K), G("bwd_data", M, N, K), G("bwd_data_res", M, N, K),
                                             G("bwd_weight", M, N, K)]
    rows += [G("fwd", 65, 63, 68, bias=False), G("fwd", 65, 63, 33, bias=False, relu=1), G("fwd_res", 64, 64, 516, nz=3, bias=False)]
    # a GEMM operand that does not start on a 16-byte boundary: the strided kernel, and right results
    for entry, (M, N, K) in (("fwd", (65, 63, 68)), ("bwd_data", (65, 68, 64)), ("bwd_weight", (68, 60, 64))):
        for which in ("a", "b"):
            for off in (4, 8, 12):
                rows.append(G(entry, M, N, K, offs={which: off}))
    rows += [G("fwd", 64, 64, 516, nz=4, offs={"b": 8}), G("bwd_weight", 516, 64, 64, nz=4, offs={"a": 12})]
    # everything else at a 4-byte offset: still the vec route
    rest = {"out": 4, "bias": 4, "res": 4}
    rows += [G("fwd", 65, 63, 68, offs=rest, relu=1), G("fwd_res", 65, 63, 68, offs=rest), G("bwd_data", 65, 68, 64, offs=rest),
             G("bwd_data_res", 65, 68, 64, offs=rest), G("bwd_weight", 68, 60, 64, offs=rest), G("fwd_res", 64, 64, 516, nz=3, offs=rest)]
    unique = {}  # (a shape that two of the groups above ask for runs once)
    for row in rows:
        unique.setdefault(row.id, row)
    return list(unique.values())


@pytest.mark.parametrize("entry,M,N,K,kernel,nz,Kout,relu,ws,offs,bias", sweep())
def test_gemm(C, entry, M, N, K, kernel, nz, Kout, relu, ws, offs, bias):
    R = gemm_shape(OP[entry], M, N, K, Kout)[2]
    for kind in ("int", "randn"):
        d = make_data(M, N, K, kind)
        got, db, plan = call(C, entry, M, N, K, d, Kout=Kout, relu=relu, ws=ws, offs=offs, bias=bias, expect=(kernel, nz))
        A, B, bias_v, res = operands(entry, d, K if Kout is None else Kout, bias)
        if kind == "int":
            want, _ = reference(A, B, bias_v, res, relu, np.int64)
            assert np.abs(want).max() < 2 ** 24
            assert same_bits(torch.from_numpy(got), want.astype(np.float32)), \
                "%d of %d elements differ from the exact result" % (int((got != want.astype(np.float32)).sum()), got.size)
            db_int = db
        else:
            want, mag = reference(A, B, bias_v, res, relu, np.float64)
            ratio = worst_ratio(got, want, gemm_bound(mag, R))
            print("RATIO %s %s %.4f" % (KERNEL_NAME[kernel], "split" if nz > 1 else "direct", ratio))
            assert ratio <= 1.0, ratio
            if db is not None:
                print("RATIO colsum - %.4f" % check_colsum(make_data(M, N, K, "int"), d, db_int, db, M))


# ---- exact promises ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,M,N,K,kernel,nz", [
    ("fwd", 65, 63, 33, STRIDED, 1), ("fwd", 64, 64, 515, STRIDED, 4), ("fwd", 65, 63, 68, VEC_RR, 1), ("fwd", 64, 64, 516, VEC_RR, 3),
    ("bwd_data", 65, 68, 64, VEC_RJ, 1), ("bwd_data", 64, 516, 64, VEC_RJ, 3), ("bwd_weight", 68, 60, 64, VEC_IJ, 1),
    ("bwd_weight", 516, 60, 68, VEC_IJ, 3), ("bwd_weight", 512, 200, 206, STRIDED, 4)])
def test_two_calls_are_bit_identical(C, entry, M, N, K, kernel, nz):
    """"Deterministic, no atomics": the same call twice, into fresh buffers, gives the same bits."""
    d = make_data(M, N, K, "randn")
    first, db1, _ = call(C, entry, M, N, K, d, relu=0, expect=(kernel, nz))
    second, db2, _ = call(C, entry, M, N, K, d, relu=0, expect=(kernel, nz))
    assert same_bits(torch.from_numpy(first), second)
    if db1 is not None:
        assert same_bits(torch.from_numpy(db1), db2)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("entry,M,N,K,kernel,nz", [
    ("fwd", 65, 63, 33, STRIDED, 1), ("fwd", 63, 65, 515, STRIDED, 4), ("fwd", 65, 63, 68, VEC_RR, 1), ("fwd", 63, 65, 516, VEC_RR, 3),
    ("bwd_data", 65, 68, 64, VEC_RJ, 1), ("bwd_data", 65, 33, 63, STRIDED, 1), ("bwd_weight", 68, 60, 68, VEC_IJ, 1),
    ("bwd_weight", 33, 65, 63, STRIDED, 1)])
def test_element_zero_stays_where_it_belongs(C, entry, M, N, K, kernel, nz, which):
    """The loaders are branch-free: a request outside the matrix or behind the chunk reads element 0 of the operand and is zeroed when it
    is stashed.  With an infinity in element 0 of either operand, a dropped mask on ONE operand shows (inf x 0 = NaN) where finite
    inputs hide it behind the other operand's zero: every result the infinity does not belong to keeps the bits it has without it."""
    d = make_data(M, N, K, "randn")
    name = ("x" if entry == "fwd" else "dy") if which == "a" else ("x" if entry == "bwd_weight" else "w")
    hot = np.array(d[name])
    hot[0, 0] = np.inf
    plain, _, _ = call(C, entry, M, N, K, d, expect=(kernel, nz))
    got, _, _ = call(C, entry, M, N, K, dict(d, **{name: hot}), expect=(kernel, nz))
    A, B, _, _ = operands(entry, dict(d, **{name: hot}), K, True)
    touched = (np.isinf(A).astype(np.float64) @ np.ones(B.shape) + np.ones(A.shape) @ np.isinf(B).astype(np.float64)) > 0
    assert touched.any() and not touched.all() and touched.shape == got.shape
    assert not np.isfinite(got[touched]).any()
    assert same_bits(torch.from_numpy(got[~touched]), plain[~touched])


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("M,N,K,kernel,nz", [(65, 63, 33, STRIDED, 1), (64, 64, 515, STRIDED, 4), (65, 63, 68, VEC_RR, 1),
                                             (64, 64, 516, VEC_RR, 3), (256, 200, 2304, VEC_RR, 12), (7, 200, 206, STRIDED, 1)])
def test_fwd_res_is_fwd_plus_a_separately_rounded_add(C, M, N, K, kernel, nz, relu):
    """y = fp32(relu(x . w^T + b)) + res with the last add rounded on its own, BEHIND the ReLU: bit for bit numpy's float32 add of the
    plain entry point's result and res."""
    d = make_data(M, N, K, "randn")
    plain, _, _ = call(C, "fwd", M, N, K, d, relu=relu, expect=(kernel, nz))
    fused, _, _ = call(C, "fwd_res", M, N, K, d, relu=relu, expect=(kernel, nz))
    assert plain.dtype == np.float32 and d["res_y"].dtype == np.float32
    assert same_bits(torch.from_numpy(fused), plain + d["res_y"])
    if relu:
        assert (plain == 0).any() and (plain > 0).any()  # both sides of the ReLU are exercised
        assert (fused[plain == 0] == d["res_y"][plain == 0]).all()


@pytest.mark.parametrize("M,N,K,kernel,nz", [(65, 33, 63, STRIDED, 1), (64, 515, 64, STRIDED, 4), (65, 68, 64, VEC_RJ, 1),
                                             (64, 516, 64, VEC_RJ, 3), (512, 2304, 200, VEC_RJ, 12)])
def test_bwd_data_res_is_bwd_data_plus_a_separately_rounded_add(C, M, N, K, kernel, nz):
    d = make_data(M, N, K, "randn")
    plain, _, _ = call(C, "bwd_data", M, N, K, d, expect=(kernel, nz))
    fused, _, _ = call(C, "bwd_data_res", M, N, K, d, Kout=K, expect=(kernel, nz))
    assert same_bits(torch.from_numpy(fused), plain + d["res_dx"])


@pytest.mark.parametrize("M,S,A,kernel,nz", [(7, 200, 6, STRIDED, 1), (8, 64, 8, VEC_RJ, 1), (4, 512, 4, VEC_RJ, 4), (3, 515, 2, STRIDED, 4)])
def test_bwd_data_res_with_res_aliased_to_dy(C, M, S, A, kernel, nz):
    """d state = dy + (dy . W)[:, :S] as ops.ForwardModelFn.backward calls it: res IS dy (N = Kout = S, K = S + A)."""
    N, K = S, S + A
    for kind in ("int", "randn"):
        d = make_data(M, N, K, kind)
        got, _, _ = call(C, "bwd_data_res", M, N, K, d, Kout=S, alias_res=True, expect=(kernel, nz))
        A_, B_ = d["dy"], d["w"][:, :S]
        if kind == "int":
            want, _ = reference(A_, B_, None, d["dy"], 0, np.int64)
            assert same_bits(torch.from_numpy(got), want.astype(np.float32))
        else:
            want, mag = reference(A_, B_, None, d["dy"], 0, np.float64)
            assert worst_ratio(got, want, gemm_bound(mag, N)) <= 1.0
            # the same bits as with a copy of dy for res
            d2 = dict(d, res_dx=np.ascontiguousarray(np.pad(d["dy"], ((0, 0), (0, A)))))
            same, _, _ = call(C, "bwd_data_res", M, N, K, d2, Kout=S, expect=(kernel, nz))
            assert same_bits(torch.from_numpy(got), same)


# ---- colsum_kernel: the db of bwd_weight ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 7, 8, 9, 17, 257])
def test_colsum(C, M):
    """Four row slices of per = (M + 3) / 4 rows: empty slices (M = 1, 2, 3, 5: per * 3 >= M), ragged last slices, the four-way unrolled
    loop and its tail; N around the 64-column block."""
    K = 3
    for N in (1, 63, 64, 65, 129):
        got = {}
        for kind in ("int", "randn"):
            d = make_data(M, N, K, kind)
            dw, got[kind], _ = call(C, "bwd_weight", M, N, K, d, expect=(STRIDED, 1))
            want, mag = reference(d["dy"].T, d["x"], None, None, 0, np.float64)
            assert worst_ratio(dw, want, gemm_bound(mag, M)) <= 1.0
        print("RATIO colsum - %.4f" % check_colsum(make_data(M, N, K, "int"), make_data(M, N, K, "randn"), got["int"], got["randn"], M))
        # db = NULL: dw as before (its sentinels and the workspace are checked inside call), no column sums anywhere
        dw2, none, _ = call(C, "bwd_weight", M, N, K, d, want_db=False, expect=(STRIDED, 1))
        assert none is None and same_bits(torch.from_numpy(dw2), dw)


# ---- relu_bwd_kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 3])
def test_relu_bwd_inplace(C, n):
    """dy *= (y > 0) as written: `if (!(y > 0)) dy = 0`.  A NaN y zeroes the gradient, a positive subnormal y keeps it (fp32 subnormals
    are not flushed), zeros of either sign and everything negative zero it; kept values are untouched bit for bit (a NaN or -0.0
    gradient included).  n behind the cap of 4096 blocks takes the grid-stride loop a second time."""
    rs = np.random.RandomState(n % 1000)
    sub = np.float32(2.0 ** -149)
    special = np.array([0.0, -0.0, sub, -sub, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)
    y = rs.standard_normal(n).astype(np.float32)
    dy = rs.standard_normal(n).astype(np.float32)
    # the special y at the front (as many as fit), and again at the very end; special gradients under kept and under zeroed positions
    for start in (0, max(0, n - len(special))):
        m = min(len(special), n - start)
        y[start:start + m] = special[:m]
    if n > 64:
        y[40:48] = [1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, np.nan]
        dy[40:48] = [np.nan, -0.0, np.inf, sub, np.nan, -0.0, np.inf, np.nan]
    with np.errstate(invalid="ignore"):
        want = np.where(y > 0, dy, np.float32(0.0)).astype(np.float32)
    yd = put(y)
    whole, dyd = guarded(torch.from_numpy(dy))
    C.relu_bwd_inplace(C.ptr(yd), C.ptr(dyd), n, C.stream())
    torch.cuda.synchronize()
    assert tail_intact(whole, n)
    assert same_bits(dyd, want)
    got = dyd.cpu().numpy()
    if n >= len(special):
        keep = [False, False, True, False, True, False, False, True, False]
        assert [bool(got[i] == dy[i]) for i in range(len(special))] == keep
        assert all(got[i] == 0 and not np.signbit(got[i]) for i in range(len(special)) if not keep[i])
    assert same_bits(yd, y)


# ---- through srlz.ops: the two shapes whose weight gradient takes strided split-K in a batch-256 step ----------------------------------
def check_elementwise(name, got, ref, bound):
    ratio = worst_ratio(got.detach().cpu().numpy(), ref, bound)
    print("RATIO ops:%s - %.4f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("relu", [False, True])
def test_linear_fn_at_the_inverse_heads_batch_256_shape(C, relu):
    from srlz import ops
    M, N, K = 512, 6, 400
    assert route(C, BWD_WEIGHT, M, N, K) == (STRIDED, 4, 128) and route(C, FWD, M, N, K)[:2] == (VEC_RR, 1)
    d = make_data(M, N, K, "randn")
    x, w, b = (torch.from_numpy(d[k].copy()).to(DEV).requires_grad_(True) for k in ("x", "w", "bias"))
    y = ops.LinearFn.apply(x, w, b, relu)
    y.backward(torch.from_numpy(d["dy"].copy()).to(DEV))
    torch.cuda.synchronize()
    x64, w64, b64, dy64 = (d[k].astype(np.float64) for k in ("x", "w", "bias", "dy"))
    pre = x64 @ w64.T + b64
    bound_y = gemm_bound(np.abs(x64) @ np.abs(w64).T + np.abs(b64), K)
    check_elementwise("y", y, np.maximum(pre, 0) if relu else pre, bound_y)
    if relu:
        # the gradient reference takes the kernel's own ReLU decisions; they are the fp64 ones wherever fp32 can tell
        mask = y.detach().cpu().numpy() > 0
        sure = np.abs(pre) > bound_y
        assert sure.mean() > 0.99 and (mask[sure] == (pre[sure] > 0)).all()
        dy64 = dy64 * mask
    check_elementwise("dx", x.grad, dy64 @ w64, gemm_bound(np.abs(dy64) @ np.abs(w64), N))
    check_elementwise("dw", w.grad, dy64.T @ x64, gemm_bound(np.abs(dy64).T @ np.abs(x64), M))
    check_elementwise("db", b.grad, dy64.sum(0), 1.01 * (M + 4) * U * np.abs(dy64).sum(0))


def test_forward_model_fn_at_batch_256(C):
    from srlz import ops
    B, S, A = 512, 200, 6
    K = S + A
    assert route(C, BWD_WEIGHT, B, S, K) == (STRIDED, 4, 128) and route(C, FWD, B, S, K)[:2] == (STRIDED, 1)
    assert route(C, BWD_DATA, B, S, K, S)[:2] == (STRIDED, 1)
    d = make_data(B, S, K, "randn")
    state = torch.from_numpy(d["res_y"].copy()).to(DEV).requires_grad_(True)
    w, b = (torch.from_numpy(d[k].copy()).to(DEV).requires_grad_(True) for k in ("w", "bias"))
    act_np = np.random.RandomState(5).randint(0, A, size=B)
    y = ops.ForwardModelFn.apply(state, torch.from_numpy(act_np).to(DEV), w, b, A)
    y.backward(torch.from_numpy(d["dy"].copy()).to(DEV))
    torch.cuda.synchronize()
    s64, w64, b64, dy64 = (d[k].astype(np.float64) for k in ("res_y", "w", "bias", "dy"))
    cat = np.concatenate([s64, np.eye(A)[act_np]], 1)
    check_elementwise("next_state", y, s64 + (cat @ w64.T + b64), gemm_bound(np.abs(cat) @ np.abs(w64).T + np.abs(b64) + np.abs(s64), K))
    check_elementwise("dstate", state.grad, dy64 + (dy64 @ w64)[:, :S], gemm_bound((np.abs(dy64) @ np.abs(w64))[:, :S] + np.abs(dy64), S))
    check_elementwise("dw", w.grad, dy64.T @ cat, gemm_bound(np.abs(dy64).T @ np.abs(cat), B))
    check_elementwise("db", b.grad, dy64.sum(0), 1.01 * (B + 4) * U * np.abs(dy64).sum(0))
