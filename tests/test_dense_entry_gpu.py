"""The dense-layer kernels (csrc/dense.hip) entry by entry at the tile's edges (GPU): the twelve srlz_dense_* / srlz_tanh_* /
srlz_add_f32 entry points called by name, at the smallest shapes at which each edge of dense_tile_kernel exists (DENSE_EDGE_SHAPES of
test_dense_host_cpu.py: K, plane, M and n off every multiple of the tile, a split with two r-steps per chunk and a short last chunk).

Every case first asserts the library's split / workspace / workgroup queries against the table, so a case cannot quietly test another
split.  Workspaces are pre-filled with a NaN bit pattern no sum can have: after a call exactly the floats the entry point owns have
changed.  Outputs are NaN before the call and sit between NaN sentinels that must come back untouched.  Operands have NaNs behind
them too: a loader that runs on behind its operand without zeroing what it read shows as NaN (inf x 0), as does one that runs on into
the next row (test_a_row_ends_where_the_reduction_ends).

Two CPU references per case:
  * integer-exact: every fp32 operand an integer of [-4, 4]; the uint8 routes get a table lut[c][v] = ((5 v + 3 c) % 9) - 4 that differs
    per channel, so a wrong channel is an exact mismatch.  Every partial sum stays below 8223 * 16 < 2^24: any order of fp32 accumulation
    is exact and the result equals numpy's int64 result bit for bit (the fp64 loss partials included, tile by tile);
  * random (uniform uint8 frames through the real srlz_normalize_lut table, weights uniform +-R^-1/2, the rest uniform +-1, gain 0.37,
    div = half * K) against fp64, element by element:
        |got - ref| <= 1.01 (R + Z + 3) 2^-24 (sum_r |a_ir| |b_rj| + |bias_j|) + R 2^-126
    with R the whole reduction length and Z the number of split partials (1 without a split): any order of R fused or unfused
    multiply-adds, Z - 1 combines and a bias add.  dOut adds three roundings (the subtraction, g / div, the product) on
    |gd| (mag + |t|); a loss partial propagates the element bound delta on d through d^2 (2 |d| delta + delta^2 per element; the fp64
    additions, below 4096 * 2^-53 relative, vanish in the 1 % of the factor 1.01).  Derived, not measured.

Largest error / bound seen on an MI355X per entry point (printed by every case as a "RATIO" line):
    in_fwd        y 0.077 (K = 33; below 0.0001 at K = 8223: the bound grows with R, the error of a sum like sqrt R)
    in_wgrad      dw 0.204, db 0.102
    out_fwd       out 0.078
    out_fwd_loss  partial 0.139
    out_bwd       dOut 0.146
    out_bwd_from  dw 0.221, db 0.113, dz 0.090
    tanh_bwd      0.482
    through srlz.ops: DenseInFn y 0.0081 (tanh 0.0042), dw 0.204, db 0.102; DenseOutFn out 0.073, dz 0.0085, dw 0.221, db 0.113;
                      DenseOutLossFn loss 0.0018, dz 0.0039, dw 0.017, db 0.022
None is near 1: the kernels are as accurate as R fp32 multiply-adds have to be, with room to reorder.

tanhf: the largest distance from the fp64 tanh of the same fp32 argument seen on an MI355X is 1.29 ulp (in_fwd with act = 2; 0.97 ulp
in srlz_tanh_fwd on 4096 points of [-9, 9] plus +-0, +-1e-30, +-88, 1.05 ulp on the random points of test_tanh_and_add):
TANH_ULP_SEEN.  TANH_ULP_ALLOWED = 3 ulp is twice that, rounded up to a whole ulp.
"""
import functools

import numpy as np
import pytest
import torch

from test_dense_host_cpu import DENSE_EDGE_SHAPES, assert_dense_split_table
from test_kernels_gpu import C, DEV  # noqa: F401  (C: the module-scoped fixture of the kernel tests)
from test_update_path_gpu import GUARD, NAN, guarded, same_bits, tail_intact  # noqa: F401

pytestmark = pytest.mark.gpu

WS_SENTINEL = 0x7FC0BEEF  # a NaN with a payload: no sum of finite numbers has these bits
U = 2.0 ** -24
TANH_ULP_SEEN = 1.29
TANH_ULP_ALLOWED = 3.0
SHAPE_IDS = ["%dx%d-plane%d-c%d" % s[:4] for s in DENSE_EDGE_SHAPES]
S_7x50 = DENSE_EDGE_SHAPES[1]
S_65x65 = DENSE_EDGE_SHAPES[4]
S_64x64 = DENSE_EDGE_SHAPES[3]
S_130x256 = DENSE_EDGE_SHAPES[5]
assert S_7x50[:2] == (7, 50) and S_65x65[:2] == (65, 65) and S_64x64[:2] == (64, 64) and S_130x256[:2] == (130, 256)

# the arguments of every entry point in the order of include/srlz.h (the stream follows)
ARGS = {
    "dense_in_fwd": ["x", "x_u8", "lut", "w", "b", "y", "M", "n", "K", "plane", "act", "ws", "ws_bytes"],
    "dense_in_wgrad": ["dy", "x", "x_u8", "lut", "dw", "db", "M", "n", "K", "plane"],
    "dense_out_fwd": ["z", "w", "b", "out", "M", "n", "K", "plane"],
    "dense_out_fwd_loss": ["z", "w", "b", "target", "target_u8", "lut", "partial", "M", "n", "K", "plane", "half"],
    "dense_out_bwd": ["z", "w", "b", "target", "target_u8", "lut", "gain", "div", "dz", "dw", "db", "M", "n", "K", "plane", "ws",
                      "ws_bytes"],
    "dense_out_bwd_from": ["dout", "z", "w", "dz", "dw", "db", "M", "n", "K", "plane", "ws", "ws_bytes"],
    "tanh_fwd": ["x", "y", "n"],
    "tanh_bwd": ["y", "dy", "dx", "n"],
    "add_f32": ["a", "b", "out", "n"],
}
DENSE = [e for e in ARGS if e.startswith("dense_")]


def cdiv(a, b):
    return (a + b - 1) // b


# ---- inputs (made once per shape and kind, never modified) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_lut():
    """The 3 x 256 normalisation table of srlz_normalize_lut, as the device fills it."""
    from srlz import _cabi
    t = torch.empty((3, 256), dtype=torch.float32, device=DEV)
    _cabi.normalize_lut(_cabi.ptr(t), _cabi.stream())
    torch.cuda.synchronize()
    return t.cpu().numpy()


def int_lut():
    v, c = np.arange(256)[None, :], np.arange(3)[:, None]
    return (((5 * v + 3 * c) % 9) - 4).astype(np.float32)


def channel(K, plane):
    return (np.arange(K) // plane) % 3


@functools.lru_cache(maxsize=None)
def make_data(S, kind):
    """fp32 / uint8 numpy arrays of one shape: frames x8, t8 [M,K] with their table and looked-up values x, t; the in layer's w_in [n,K],
    b_in [n], dy [M,n]; the out layer's z [M,n], w_out [K,n], b_out [K], dout [M,K]."""
    M, n, plane, Cc, _ = S
    K = Cc * plane
    rs = np.random.RandomState(1000003 * M + 1009 * n + K + (7 if kind == "int" else 0))
    d = {"x8": rs.randint(0, 256, size=(M, K)).astype(np.uint8), "t8": rs.randint(0, 256, size=(M, K)).astype(np.uint8)}
    d["lut"] = int_lut() if kind == "int" else real_lut()
    ch = channel(K, plane)[None, :]
    d["x"], d["t"] = d["lut"][ch, d["x8"]], d["lut"][ch, d["t8"]]
    shapes = {"w_in": (n, K), "b_in": (n,), "dy": (M, n), "z": (M, n), "w_out": (K, n), "b_out": (K,), "dout": (M, K)}
    scale = {"w_in": K ** -0.5, "w_out": n ** -0.5}
    for name, shape in shapes.items():
        if kind == "int":
            d[name] = rs.randint(-4, 5, size=shape).astype(np.float32)
        else:
            d[name] = (rs.uniform(-1.0, 1.0, size=shape) * scale.get(name, 1.0)).astype(np.float32)
    for v in d.values():
        assert v.dtype in (np.float32, np.uint8)
        v.setflags(write=False)
    return d


def bound(mag, R, Z=1):
    return 1.01 * (R + Z + 3) * U * mag + R * 2.0 ** -126


def gemm(A, B, bias, dtype):
    """A . B (+ bias) in dtype (np.int64: exact; np.float64), and the magnitude sum |a||b| (+ |bias|) the error bound scales with."""
    v = A.astype(dtype) @ B.astype(dtype)
    mag = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    if bias is not None:
        v, mag = v + bias.astype(dtype), mag + np.abs(bias).astype(np.float64)
    return v, mag


@functools.lru_cache(maxsize=None)
def refs(S, kind):
    """The products of one shape in int64 (kind "int") or fp64, each with its magnitude: {name: (value, mag)}."""
    d = make_data(S, kind)
    t = np.int64 if kind == "int" else np.float64
    r = {"y": gemm(d["x"], d["w_in"].T, d["b_in"], t), "y_nobias": gemm(d["x"], d["w_in"].T, None, t),
         "dw_in": gemm(d["dy"].T, d["x"], None, t), "db_in": gemm(np.ones((1, S[0]), np.float32), d["dy"], None, t),
         "out": gemm(d["z"], d["w_out"].T, d["b_out"], t), "out_nobias": gemm(d["z"], d["w_out"].T, None, t),
         "dw_out": gemm(d["dout"].T, d["z"], None, t), "db_out": gemm(np.ones((1, S[0]), np.float32), d["dout"], None, t),
         "dz": gemm(d["dout"], d["w_out"], None, t)}
    for k in ("db_in", "db_out"):
        r[k] = (r[k][0][0], r[k][1][0])
    return r


def worst_ratio(got, ref, bnd):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300)).max())


def check(name, kind, got, ref, R, Z=1, extra=0.0):
    """Integers bit for bit; random values within the derived bound (+ extra: an error the inputs of this product already carry)."""
    value, mag = ref
    assert got.shape == value.shape, (name, got.shape, value.shape)
    if kind == "int":
        assert np.abs(value).max() < 2 ** 24
        assert same_bits(torch.from_numpy(got), value.astype(np.float32)), \
            "%s: %d of %d elements differ from the exact result" % (name, int((got != value.astype(np.float32)).sum()), got.size)
    else:
        ratio = worst_ratio(got, value, bound(mag, R, Z) + extra)
        print("RATIO %s %.4f" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)


def tile_sums(a, half):
    """[2][nwg] sums of a [M][K] array over the 64 x 64 tiles, rows < half and >= half, workgroup index by * gridDim.x + bx."""
    M, K = a.shape
    gy, gx = cdiv(M, 64), cdiv(K, 64)
    out = []
    for rows in (np.arange(M) < half, np.arange(M) >= half):
        p = np.zeros((gy * 64, gx * 64), dtype=a.dtype)
        p[:M, :K] = a * rows[:, None].astype(a.dtype)
        out.append(p.reshape(gy, 64, gx, 64).sum(axis=(1, 3)).reshape(-1))
    return np.stack(out)


def tanh_ulps(got, arg):
    """Largest distance of got (fp32) from the fp64 tanh of arg (fp32) in ulps of the result's binade."""
    ref = np.tanh(arg.astype(np.float64))
    e = np.maximum(np.frexp(np.abs(ref))[1], -125)
    return float((np.abs(got.astype(np.float64) - ref) / np.ldexp(1.0, e - 24)).max())


# ---- device buffers ----------------------------------------------------------------------------------------------------------------
def put(src, off=0):
    """Device copy of a numpy array starting `off` bytes behind a 16-byte boundary (a view into a longer buffer), with GUARD NaNs (bytes
    of 255 for uint8) behind it: a loader that reads behind its operand and does not zero what it read turns the result into NaN."""
    src = np.asarray(src)
    k, n = (0 if src.dtype == np.uint8 else off // 4), src.size
    if src.dtype == np.uint8:
        whole = torch.full((n + GUARD,), 255, dtype=torch.uint8, device=DEV)
    else:
        whole = torch.full((k + n + GUARD,), NAN, device=DEV)
    view = whole[k:k + n].view(src.shape)
    # (a writable copy: the cached inputs are read-only)
    view.copy_(torch.from_numpy(np.array(src, dtype=np.uint8 if src.dtype == np.uint8 else np.float32)))
    assert src.dtype == np.uint8 or view.data_ptr() % 16 == off
    return view


class Out:
    """An output of NaNs between NaN sentinels, `off` bytes behind a 16-byte boundary (fp32; fp64 for the loss partials)."""

    def __init__(self, shape, off=0, dtype=torch.float32):
        self.k, self.n = off // 4, int(np.prod(shape))
        self.whole = torch.full((self.k + self.n + GUARD,), NAN, dtype=dtype, device=DEV)
        self.view = self.whole[self.k:self.k + self.n].view(shape)
        assert self.view.data_ptr() % 16 == off

    def result(self):
        """The payload as a numpy array; the sentinels before and behind it must be intact."""
        assert bool(torch.isnan(self.whole[:self.k]).all()) and tail_intact(self.whole[self.k:], self.n)
        return self.view.cpu().numpy()

    def untouched(self):
        return bool(torch.isnan(self.whole).all())


class Workspace:
    """`nbytes` of workspace filled with WS_SENTINEL, `off` bytes behind a 16-byte boundary, and GUARD more words behind it."""

    def __init__(self, nbytes, off=0):
        self.nbytes, self.k = nbytes, off // 4
        self.whole = torch.full((self.k + (nbytes + 3) // 4 + GUARD,), WS_SENTINEL, dtype=torch.int32, device=DEV)
        self.words = self.whole[self.k:]
        assert self.words.data_ptr() % 16 == off

    def check(self, used):
        """Exactly the first `used` floats were written."""
        assert used * 4 <= self.nbytes
        assert bool((self.whole[:self.k] == WS_SENTINEL).all())
        assert bool((self.words[:used] != WS_SENTINEL).all()), "a float of the workspace the entry point owns was not written"
        assert bool((self.words[used:] == WS_SENTINEL).all()), "the workspace was written behind its first %d floats" % used

    def floats(self, count):
        return self.words[:count].view(torch.float32).cpu().numpy()

    def untouched(self):
        return bool((self.whole == WS_SENTINEL).all())


@functools.lru_cache(maxsize=None)
def dev(S, kind, off=0):
    """Device copies of make_data(S, kind), the fp32 ones `off` bytes behind a 16-byte boundary.  For the random kind the fp32 frames are
    srlz_normalize_u8_planar's output of the uint8 frames with the real table — and equal the table lookup bit for bit."""
    from srlz import _cabi
    d = make_data(S, kind)
    D = {k: put(v, off) for k, v in d.items()}
    if kind == "rnd":
        M, _, plane, Cc, _ = S
        for f, b in (("x", "x8"), ("t", "t8")):
            o = Out(d[f].shape, off)
            _cabi.normalize_u8_planar(_cabi.ptr(D[b]), _cabi.ptr(D["lut"]), _cabi.ptr(o.view), M, Cc, plane, _cabi.stream())
            torch.cuda.synchronize()
            assert same_bits(torch.from_numpy(o.result()), np.array(d[f]))
            D[f] = o.view
    return D


def build(C, entry, S, kind, off=0, u8=False, act=0, bias=True, want_db=True, want_dz=True, half=None, gain=None, div=None, dout=None):
    """The arguments of one call at shape S by name (ARGS[entry]): device tensors, Out / Workspace objects, None for NULL, numbers."""
    M, n, plane, Cc, Z = S
    K = Cc * plane
    D = dev(S, kind, off)
    a = {"M": M, "n": n, "K": K, "plane": plane, "lut": D["lut"] if u8 else None}
    img = lambda f, b: (None, D[b]) if u8 else (D[f], None)  # noqa: E731
    if entry == "dense_in_fwd":
        a["x"], a["x_u8"] = img("x", "x8")
        nbytes = C.dense_in_workspace(M, n, K)
        a.update(w=D["w_in"], b=D["b_in"] if bias else None, y=Out((M, n), off), act=act, ws=Workspace(nbytes, off), ws_bytes=nbytes)
    elif entry == "dense_in_wgrad":
        a["x"], a["x_u8"] = img("x", "x8")
        a.update(dy=D["dy"], dw=Out((n, K), off), db=Out((n,), off) if want_db else None)
    elif entry == "dense_out_fwd":
        a.update(z=D["z"], w=D["w_out"], b=D["b_out"] if bias else None, out=Out((M, K), off))
    elif entry == "dense_out_fwd_loss":
        a["target"], a["target_u8"] = img("t", "t8")
        nwg = C.dense_out_fwd_loss_workgroups(M, K)
        a.update(z=D["z"], w=D["w_out"], b=D["b_out"] if bias else None, partial=Out((2, nwg), 0, torch.float64),
                 half=M // 2 if half is None else half)
    elif entry == "dense_out_bwd":
        a["target"], a["target_u8"] = img("t", "t8")
        nbytes = C.dense_out_bwd_workspace(M, n, K)
        a.update(z=D["z"], w=D["w_out"], b=D["b_out"] if bias else None, gain=put(np.array([gain], np.float32), off), div=div,
                 dz=Out((M, n), off) if want_dz else None, dw=Out((K, n), off), db=Out((K,), off), ws=Workspace(nbytes, off),
                 ws_bytes=nbytes)
    elif entry == "dense_out_bwd_from":
        nbytes = C.dense_in_workspace(M, n, K)
        a.update(dout=D["dout"] if dout is None else dout, z=D["z"], w=D["w_out"], dz=Out((M, n), off) if want_dz else None,
                 dw=Out((K, n), off), db=Out((K,), off), ws=Workspace(nbytes, off), ws_bytes=nbytes)
    else:
        raise KeyError(entry)
    return a


def launch(C, entry, a, raw=False):
    """The call, by name.  raw: the library's own status instead of the binding's exception."""
    vals = []
    for name in ARGS[entry]:
        v = a[name]
        if isinstance(v, Out):
            v = C.ptr(v.view)
        elif isinstance(v, Workspace):
            v = C.ptr(v.words)
        elif isinstance(v, torch.Tensor):
            v = C.ptr(v)
        vals.append(v)
    fn = getattr(C._lib, "srlz_" + entry) if raw else getattr(C, entry)
    rc = fn(*vals, C.stream())
    torch.cuda.synchronize()
    return rc


def ws_used(entry, a):
    """The floats of the workspace the call must have written, from the table's Z."""
    M, n, K = a["M"], a["n"], a["K"]
    zmn = a["ws"].nbytes // 4 - (M * K if entry == "dense_out_bwd" else 0)
    if entry == "dense_in_fwd":
        return zmn
    return (M * K if entry == "dense_out_bwd" else 0) + (zmn if a["dz"] is not None else 0)


def run(C, entry, S, kind, override=None, **kw):
    """One call at shape S (override: {argument name: another device tensor}): asserts the queries against the table, the workspace and
    every sentinel; {output name: numpy array}."""
    assert_dense_split_table(C, *S)
    a = build(C, entry, S, kind, **kw)
    a.update(override or {})
    if "ws" in a:
        M, n, K, Z = a["M"], a["n"], a["K"], S[4]
        assert a["ws_bytes"] == (Z * M * n + (M * K if entry == "dense_out_bwd" else 0)) * 4
    launch(C, entry, a)
    res = {k: v.result() for k, v in a.items() if isinstance(v, Out)}
    if "ws" in a:
        a["ws"].check(ws_used(entry, a))
        if entry == "dense_out_bwd":
            res["dout"] = a["ws"].floats(a["M"] * a["K"]).reshape(a["M"], a["K"])
    return res


def same(a, b):
    """Two results of run() equal bit for bit, output by output."""
    assert sorted(a) == sorted(b)
    for k in a:
        if a[k].dtype == np.float64:
            assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
        else:
            assert same_bits(torch.from_numpy(a[k]), b[k]), k
    return True


KINDS = ("int", "rnd")


# ---- the in layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", DENSE_EDGE_SHAPES, ids=SHAPE_IDS)
def test_in_fwd(C, S):
    """y = act(x . W^T + b) over the split: fp32 and uint8 x agree bit for bit for every act; ReLU is the bitwise max(., 0) and tanh the
    tanhf of the act = 0 output (same partials, same z order, same bias add: the pre-activation bits are identical)."""
    M, n, plane, Cc, Z = S
    K = Cc * plane
    for kind in KINDS:
        got = {(u8, act): run(C, "dense_in_fwd", S, kind, u8=u8, act=act)["y"] for u8 in (False, True) for act in (0, 1, 2)}
        for act in (0, 1, 2):
            assert same_bits(torch.from_numpy(got[True, act]), got[False, act]), act
        y0 = got[False, 0]
        check("in_fwd:y", kind, y0, refs(S, kind)["y"], K, Z)
        assert same_bits(torch.from_numpy(got[False, 1]), np.where(y0 > 0, y0, np.float32(0.0)))
        ulps = tanh_ulps(got[False, 2], y0)
        print("TANH_ULPS in_fwd %.4f" % ulps)
        assert ulps <= TANH_ULP_ALLOWED, ulps
        assert same_bits(torch.from_numpy(run(C, "dense_in_fwd", S, kind, u8=True, act=2)["y"]), got[True, 2])  # two runs


@pytest.mark.parametrize("S", DENSE_EDGE_SHAPES, ids=SHAPE_IDS)
def test_in_wgrad(C, S):
    """dW = dy^T . x with M as the reduction and K as the column index (the uint8 channel per element of a tile), db = column sums."""
    M = S[0]
    for kind in KINDS:
        f32, u8 = run(C, "dense_in_wgrad", S, kind), run(C, "dense_in_wgrad", S, kind, u8=True)
        assert same(f32, u8) and same(u8, run(C, "dense_in_wgrad", S, kind, u8=True))
        check("in_wgrad:dw", kind, f32["dw"], refs(S, kind)["dw_in"], M)
        check("in_wgrad:db", kind, f32["db"], refs(S, kind)["db_in"], M)


# ---- the out layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", DENSE_EDGE_SHAPES, ids=SHAPE_IDS)
def test_out_fwd(C, S):
    n = S[1]
    for kind in KINDS:
        got = run(C, "dense_out_fwd", S, kind)
        check("out_fwd:out", kind, got["out"], refs(S, kind)["out"], n)
        assert same(got, run(C, "dense_out_fwd", S, kind))


@pytest.mark.parametrize("S", [S_7x50, DENSE_EDGE_SHAPES[2], S_65x65], ids=["7x50", "33x63", "65x65"])
@pytest.mark.parametrize("entry,name,key", [("dense_in_fwd", "x", "y"), ("dense_out_fwd", "z", "out")])
def test_a_row_ends_where_the_reduction_ends(C, S, entry, name, key):
    """The loaders are branch-free: a request behind the reduction's end reads offset 0 and is zeroed when it is stashed.  With an
    infinity in the first column of row 1, a last r-step of row 0 that runs on into row 1 shows (inf x 0 = NaN) where finite values hide
    behind the other operand's zero: every row but row 1 keeps the bits it has without the infinity."""
    assert (S[2] * S[3]) % 32 and S[1] % 32  # the last r-step is a partial one
    plain = run(C, entry, S, "rnd")[key]
    hot = np.array(make_data(S, "rnd")[name])
    hot[1, 0] = np.inf
    got = run(C, entry, S, "rnd", override={name: put(hot)})[key]
    rest = np.arange(S[0]) != 1
    assert not np.isfinite(got[1]).any()
    assert same_bits(torch.from_numpy(got[rest]), plain[rest])


def halves(M):
    h = sorted({0, 1, M // 2, M} if M % 2 == 0 else {0, M // 2, M})
    return h + [64, 65] if M == 130 else h


def d_and_delta(S, kind, bias=True):
    """d = out - target of the references and, for the random kind, the element bound delta on it: the product's bound plus the rounding
    of the subtraction."""
    d = make_data(S, kind)
    out, mag = refs(S, kind)["out" if bias else "out_nobias"]
    t = d["t"].astype(out.dtype)
    return out - t, bound(mag, S[1]) + 1.01 * U * (mag + np.abs(t)), mag + np.abs(t)


def check_partials(name, kind, got, S, half, bias=True):
    dd, delta, _ = d_and_delta(S, kind, bias)
    if kind == "int":
        want = tile_sums(dd * dd, half)
        assert np.abs(want).max() < 2 ** 53
        assert np.array_equal(got, want.astype(np.float64)), "%s: %d partials differ" % (name, int((got != want).sum()))
    else:
        ratio = worst_ratio(got, tile_sums(dd * dd, half), tile_sums(2 * np.abs(dd) * delta + delta * delta, half))
        print("RATIO %s %.4f" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("S", DENSE_EDGE_SHAPES, ids=SHAPE_IDS)
def test_out_fwd_loss(C, S):
    """The 2 * nwg fp64 partials, each against the sum over its own 64 x 64 tile, rows < half and >= half (index by * gridDim.x + bx);
    the per-lane channel of the uint8 target against the per-element one of the reference."""
    for kind in KINDS:
        for half in halves(S[0]):
            f32 = run(C, "dense_out_fwd_loss", S, kind, half=half)
            assert same(f32, run(C, "dense_out_fwd_loss", S, kind, half=half, u8=True))
            check_partials("out_fwd_loss:partial", kind, f32["partial"], S, half)
        assert same(f32, run(C, "dense_out_fwd_loss", S, kind, half=half))  # two runs


@pytest.mark.parametrize("S", DENSE_EDGE_SHAPES, ids=SHAPE_IDS)
def test_out_bwd_from(C, S):
    """dW = dOut^T . z and db (the column of ones beside z) with M as the reduction, dz = dOut . W split over K; without dz nothing of
    the workspace is written and dW, db keep their bits."""
    M, n, plane, Cc, Z = S
    for kind in KINDS:
        got = run(C, "dense_out_bwd_from", S, kind)
        r = refs(S, kind)
        check("out_bwd_from:dw", kind, got["dw"], r["dw_out"], M)
        check("out_bwd_from:db", kind, got["db"], r["db_out"], M)
        check("out_bwd_from:dz", kind, got["dz"], r["dz"], Cc * plane, Z)
        assert same(got, run(C, "dense_out_bwd_from", S, kind))
        nodz = run(C, "dense_out_bwd_from", S, kind, want_dz=False)
        assert "dz" not in nodz and same(nodz, {k: got[k] for k in ("dw", "db")})


def gain_div(S, kind):
    """gain = 3, div = 4 for the integers (gd = 1.5 exactly); gain = 0.37, div = half * K for the random kind."""
    return (3.0, 4.0) if kind == "int" else (0.37, float(max(1, S[0] // 2) * S[2] * S[3]))


def check_dout(name, kind, got, S, gain, div, bias=True):
    """dOut = ((g / div) * 2) * (out - t): three more roundings (the subtraction, g / div, the product) on |gd| (mag + |t|)."""
    dd, _, magt = d_and_delta(S, kind, bias)
    gd = np.float64(np.float32(gain)) / np.float64(np.float32(div)) * 2.0
    mag = refs(S, kind)["out" if bias else "out_nobias"][1]
    if kind == "int":
        assert gd == 1.5
        assert same_bits(torch.from_numpy(got), (1.5 * dd).astype(np.float32)), name
    else:
        bnd = abs(gd) * (1.01 * (S[1] + 4) * U * mag + 1.01 * 3 * U * magt) + S[1] * 2.0 ** -126
        ratio = worst_ratio(got, gd * dd, bnd)
        print("RATIO %s %.4f" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("S", DENSE_EDGE_SHAPES, ids=SHAPE_IDS)
def test_out_bwd(C, S):
    """The fused backward at a gain that is not 1: dOut (read back from the first M * K floats of the workspace) against the reference;
    dz, dW, db bit for bit those of out_bwd_from on that dOut (same kernels, same inputs); uint8 and fp32 targets agree bit for bit."""
    M, K = S[0], S[2] * S[3]
    for kind in KINDS:
        gain, div = gain_div(S, kind)
        got = run(C, "dense_out_bwd", S, kind, gain=gain, div=div)
        assert same(got, run(C, "dense_out_bwd", S, kind, gain=gain, div=div, u8=True))
        check_dout("out_bwd:dout", kind, got["dout"], S, gain, div)
        again = run(C, "dense_out_bwd_from", S, kind, dout=put(got["dout"]))
        assert same(again, {k: got[k] for k in ("dz", "dw", "db")})
        nodz = run(C, "dense_out_bwd", S, kind, gain=gain, div=div, u8=True, want_dz=False)
        assert "dz" not in nodz and same(nodz, {k: got[k] for k in ("dout", "dw", "db")})


# ---- optional pointers, misaligned operands ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [S_7x50, S_65x65], ids=["7x50", "65x65"])
def test_optional_pointers(C, S):
    """bias = NULL for the four entry points that take one; db = NULL for in_wgrad (dz = NULL: test_out_bwd_from, test_out_bwd)."""
    M, n, plane, Cc, Z = S
    K = Cc * plane
    for kind in KINDS:
        r = refs(S, kind)
        check("in_fwd:y-nobias", kind, run(C, "dense_in_fwd", S, kind, u8=True, bias=False)["y"], r["y_nobias"], K, Z)
        check("out_fwd:out-nobias", kind, run(C, "dense_out_fwd", S, kind, bias=False)["out"], r["out_nobias"], n)
        got = run(C, "dense_out_fwd_loss", S, kind, u8=True, bias=False)
        check_partials("out_fwd_loss:partial-nobias", kind, got["partial"], S, M // 2, bias=False)
        gain, div = gain_div(S, kind)
        got = run(C, "dense_out_bwd", S, kind, gain=gain, div=div, bias=False)
        check_dout("out_bwd:dout-nobias", kind, got["dout"], S, gain, div, bias=False)
        nodb = run(C, "dense_in_wgrad", S, kind, u8=True, want_db=False)
        assert "db" not in nodb and same(nodb, {"dw": run(C, "dense_in_wgrad", S, kind, u8=True)["dw"]})


@pytest.mark.parametrize("entry", DENSE)
def test_operands_four_bytes_behind_a_16_byte_boundary(C, entry):
    """Every fp32 operand, output and workspace at 16 k + 4: the kernels use dword accesses, which this pins.  The same bits as aligned."""
    S = S_7x50
    for kind in KINDS:
        gain, div = gain_div(S, kind)
        kw = {"gain": gain, "div": div} if entry == "dense_out_bwd" else {}
        got = run(C, entry, S, kind, off=4, **kw)
        assert same(got, run(C, entry, S, kind, **kw))
        key, name, R, Z = {"dense_in_fwd": ("y", "y", 105, 4), "dense_in_wgrad": ("dw", "dw_in", 7, 1),
                           "dense_out_fwd": ("out", "out", 50, 1), "dense_out_bwd_from": ("dz", "dz", 105, 4)}.get(entry, (None,) * 4)
        if key:
            check("%s:%s+4" % (entry[6:], key), kind, got[key], refs(S, kind)[name], R, Z)
        elif entry == "dense_out_bwd":
            check_dout("out_bwd:dout+4", kind, got["dout"], S, gain, div)
        else:
            check_partials("out_fwd_loss:partial+4", kind, got["partial"], S, S[0] // 2)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refused(C, entry, a, code, what):
    """The call returns `code`, leaves a message, and touches no output and no workspace."""
    rc = launch(C, entry, a, raw=True)
    assert rc == code, "%s %s: status %d, expected %d (%s)" % (entry, what, rc, code, C.error_text())
    text = C.error_text()
    assert text and any(tag in text for tag in ("dense", "tanh", "add")), (entry, what, text)
    for k, v in a.items():
        if isinstance(v, (Out, Workspace)):
            assert v.untouched(), "%s %s: %s was written" % (entry, what, k)


REQUIRED = {"dense_in_fwd": ["w", "y", "ws"], "dense_in_wgrad": ["dy", "dw"], "dense_out_fwd": ["z", "w", "out"],
            "dense_out_fwd_loss": ["z", "w", "partial"], "dense_out_bwd": ["z", "w", "gain", "dw", "db", "ws"],
            "dense_out_bwd_from": ["dout", "z", "w", "dw", "db", "ws"]}
IMAGE = {"dense_in_fwd": ("x", "x_u8"), "dense_in_wgrad": ("x", "x_u8"), "dense_out_fwd_loss": ("target", "target_u8"),
         "dense_out_bwd": ("target", "target_u8")}


@pytest.mark.parametrize("entry", DENSE)
def test_refusals(C, entry):
    """SRLZ_ERR_NULL (-4) for each required pointer in turn, SRLZ_ERR_BAD_DESC (-1) for each shape, option and workspace size the entry
    point does not take: by its code, with a message, and with every output and workspace sentinel untouched."""
    S = S_7x50
    M, n, plane, Cc, _ = S
    K = Cc * plane
    kw = {"gain": 3.0, "div": 4.0} if entry == "dense_out_bwd" else {}

    def fresh(**change):
        u8 = change.pop("u8", False)
        a = build(C, entry, S, "int", u8=u8, **kw)
        a.update(change)
        return a

    for name in REQUIRED[entry]:
        refused(C, entry, fresh(**{name: None}), -4, name + " = NULL")
    if entry in IMAGE:
        f, b = IMAGE[entry]
        refused(C, entry, fresh(**{f: None}), -4, "%s and %s both NULL" % (f, b))
        refused(C, entry, fresh(u8=True, lut=None), -4, b + " without lut")
    bad = [{"M": 0}, {"n": 0}, {"n": 257}, {"plane": 0}, {"K": 2 * plane}, {"K": 4 * plane}, {"K": K + 1}]
    if entry == "dense_in_fwd":
        bad += [{"act": -1}, {"act": 3}]
    if entry == "dense_out_fwd_loss":
        bad += [{"half": -1}, {"half": M + 1}]
    if entry == "dense_out_bwd":
        bad += [{"div": 0.0}, {"div": -1.0}]
    if "ws" in ARGS[entry]:
        bad += [{"ws_bytes": fresh()["ws_bytes"] - 1}]
    for change in bad:
        refused(C, entry, fresh(**change), -1, repr(change))
    # ... and the untouched call goes through
    assert launch(C, entry, fresh(), raw=True) == 0


# ---- tanh_fwd / tanh_bwd / add_f32 ------------------------------------------------------------------------------------------------
def elementwise(C, entry, ins, n, off=0):
    names = ARGS[entry]
    a = {k: put(v, off) for k, v in zip(names, ins)}
    a[names[len(ins)]] = Out((n,), off)
    a["n"] = n
    launch(C, entry, a)
    return a[names[len(ins)]].result()


def test_tanh_fwd_points(C):
    """4096 points of [-9, 9] plus +-0, +-1e-30, +-88 against fp64 tanh, in ulps."""
    x = np.concatenate([np.linspace(-9.0, 9.0, 4096), [0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0]]).astype(np.float32)
    y = elementwise(C, "tanh_fwd", [x], x.size)
    ulps = tanh_ulps(y, x)
    print("TANH_ULPS tanh_fwd %.4f" % ulps)
    assert ulps <= TANH_ULP_ALLOWED, ulps
    assert (np.abs(y) <= 1.0).all() and (np.signbit(y) == np.signbit(x)).all()
    assert y[-2] == 1.0 and y[-1] == -1.0 and y[-6] == 0.0 and y[-5] == 0.0


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_tanh_and_add(C, n, off):
    """The `e < n` guard at, before and behind a block edge; tanh_bwd within 3 * 2^-24 |dy| of dy (1 - y^2) (two or three roundings on
    terms each at most |dy|); add_f32 bit for bit numpy's fp32 sum."""
    rs = np.random.RandomState(n)
    x = rs.uniform(-4.0, 4.0, n).astype(np.float32)
    dy = rs.uniform(-1.0, 1.0, n).astype(np.float32)
    y = elementwise(C, "tanh_fwd", [x], n, off)
    ulps = tanh_ulps(y, x)
    assert ulps <= TANH_ULP_ALLOWED, ulps
    dx = elementwise(C, "tanh_bwd", [y, dy], n, off)
    y64, dy64 = y.astype(np.float64), dy.astype(np.float64)
    ratio = worst_ratio(dx, dy64 * (1.0 - y64 * y64), 3 * U * np.abs(dy64))
    print("RATIO tanh_bwd %.4f" % ratio)
    assert ratio <= 1.0, ratio
    assert same_bits(torch.from_numpy(elementwise(C, "add_f32", [x, dy], n, off)), x + dy)


@pytest.mark.parametrize("entry", ["tanh_fwd", "tanh_bwd", "add_f32"])
def test_elementwise_refusals(C, entry):
    names = ARGS[entry]
    v = np.ones(8, np.float32)

    def fresh(**change):
        a = {k: put(v) for k in names[:-2]}
        a[names[-2]] = Out((8,))
        a["n"] = 8
        a.update(change)
        return a

    for name in names[:-1]:
        refused(C, entry, fresh(**{name: None}), -4, name + " = NULL")
    refused(C, entry, fresh(n=0), -1, "n = 0")
    assert launch(C, entry, fresh(), raw=True) == 0


# ---- through srlz.ops ----------------------------------------------------------------------------------------------------------------
def leaf(a):
    return torch.from_numpy(np.array(a)).to(DEV).requires_grad_(True)


def check_elementwise(name, got, ref, bnd):
    ratio = worst_ratio(got.detach().cpu().numpy(), ref, bnd)
    print("RATIO ops:%s %.4f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("u8,act,bias", [(u8, act, True) for u8 in (True, False) for act in (0, 1, 2)] + [(True, 0, False)],
                         ids=lambda v: {True: "y", False: "n"}.get(v, str(v)) if isinstance(v, bool) else "act%d" % v)
@pytest.mark.parametrize("S", [S_7x50, S_65x65], ids=["7x50", "65x65"])
def test_dense_in_fn(C, S, u8, act, bias):
    """DenseInFn (ids: u8 y/n - act - bias y/n) against fp64, element by element.  The gradient reference takes the kernel's own
    activation (the ReLU decisions, which are the fp64 ones wherever fp32 can tell; 1 - y^2 of the fp32 y, whose rounding in tanh_bwd is
    3 * 2^-24 |dy| more on dy)."""
    from srlz import ops
    M, n, plane, Cc, Z = S
    K = Cc * plane
    d = make_data(S, "rnd")
    x = torch.from_numpy(np.array(d["x8"])).to(DEV).view(M, Cc, plane, 1) if u8 else dev(S, "rnd")["x"]
    w, b = leaf(d["w_in"]), (leaf(d["b_in"]) if bias else None)
    y = ops.DenseInFn.apply(x, w, b, act, plane)
    y.backward(torch.from_numpy(np.array(d["dy"])).to(DEV))
    torch.cuda.synchronize()
    pre, mag = refs(S, "rnd")["y" if bias else "y_nobias"]
    bnd = bound(mag, K, Z)
    y_np = y.detach().cpu().numpy().astype(np.float64)
    dy, extra = d["dy"].astype(np.float64), 0.0
    if act == 0:
        check_elementwise("in:y", y, pre, bnd)
    elif act == 1:
        check_elementwise("in:y-relu", y, np.maximum(pre, 0), bnd)
        sure = np.abs(pre) > bnd
        assert sure.mean() > 0.9 and ((y_np > 0)[sure] == (pre > 0)[sure]).all()
        dy = dy * (y_np > 0)
    else:
        check_elementwise("in:y-tanh", y, np.tanh(pre), bnd + TANH_ULP_ALLOWED * U)  # (tanh is 1-Lipschitz, |tanh| <= 1)
        extra, dy = 1.01 * 3 * U * np.abs(dy), dy * (1.0 - y_np * y_np)
    x64 = d["x"].astype(np.float64)
    check_elementwise("in:dw", w.grad, dy.T @ x64, bound(np.abs(dy).T @ np.abs(x64), M) + (extra.T @ np.abs(x64) if act == 2 else 0.0))
    if bias:
        check_elementwise("in:db", b.grad, dy.sum(0), bound(np.abs(dy).sum(0), M) + (extra.sum(0) if act == 2 else 0.0))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("S", [S_7x50, S_65x65], ids=["7x50", "65x65"])
def test_dense_out_fn(C, S, bias):
    from srlz import ops
    M, n, plane, Cc, Z = S
    K = Cc * plane
    d = make_data(S, "rnd")
    r = refs(S, "rnd")
    grads = {}
    for z_grad in (True, False):
        z = leaf(d["z"]) if z_grad else torch.from_numpy(np.array(d["z"])).to(DEV)
        w, b = leaf(d["w_out"]), (leaf(d["b_out"]) if bias else None)
        out = ops.DenseOutFn.apply(z, w, b, plane)
        out.backward(torch.from_numpy(np.array(d["dout"])).to(DEV))
        torch.cuda.synchronize()
        grads[z_grad] = (w.grad, b.grad if bias else None)
        if z_grad:
            check_elementwise("out:out", out, r["out" if bias else "out_nobias"][0], bound(r["out" if bias else "out_nobias"][1], n))
            check_elementwise("out:dz", z.grad, r["dz"][0], bound(r["dz"][1], K, Z))
            check_elementwise("out:dw", w.grad, r["dw_out"][0], bound(r["dw_out"][1], M))
            if bias:
                check_elementwise("out:db", b.grad, r["db_out"][0], bound(r["db_out"][1], M))
        else:
            assert z.grad is None
    # z without a gradient: dz is not computed, and the weight gradients keep their bits
    assert same_bits(grads[False][0], grads[True][0])
    if bias:
        assert same_bits(grads[False][1], grads[True][1])


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
@pytest.mark.parametrize("mean", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("S", [S_130x256, S_64x64], ids=["130x256", "64x64"])
def test_dense_out_loss_fn(C, S, mean, u8):
    """DenseOutLossFn with (0.37 * loss).backward(): the device-side gain is not 1.  The loss within the bound propagated through d^2
    plus srlz_pair_loss_finalize's fp32 roundings (2 * 2^-24 relative); the gradients within the bound of their products plus what the
    element bound on dOut contributes."""
    from srlz import ops
    M, n, plane, Cc, Z = S
    K = Cc * plane
    d = make_data(S, "rnd")
    z, w, b = leaf(d["z"]), leaf(d["w_out"]), leaf(d["b_out"])
    t = torch.from_numpy(np.array(d["t8"])).to(DEV).view(M, Cc, plane, 1) if u8 else dev(S, "rnd")["t"].view(M, Cc, plane, 1)
    loss = ops.DenseOutLossFn.apply(z, w, b, t, mean, plane)
    (0.37 * loss).backward()
    torch.cuda.synchronize()
    dd, delta, magt = d_and_delta(S, "rnd")
    div = float(M // 2 * K) if mean else 1.0
    loss64 = (dd * dd).sum() / div
    err = abs(float(loss.item()) - loss64)
    bnd = (2 * np.abs(dd) * delta + delta * delta).sum() / div + 2 * U * abs(loss64)
    print("RATIO ops:loss %.4f" % (err / bnd))
    assert err <= bnd, (err, bnd)
    gd = np.float64(np.float32(0.37)) / div * 2.0
    dout = gd * dd
    e_dout = abs(gd) * (1.01 * (n + 4) * U * refs(S, "rnd")["out"][1] + 1.01 * 3 * U * magt) + n * 2.0 ** -126
    z64, w64 = d["z"].astype(np.float64), d["w_out"].astype(np.float64)
    check_elementwise("loss:dz", z.grad, dout @ w64, bound(np.abs(dout) @ np.abs(w64), K, Z) + 1.01 * e_dout @ np.abs(w64))
    check_elementwise("loss:dw", w.grad, dout.T @ z64, bound(np.abs(dout).T @ np.abs(z64), M) + 1.01 * e_dout.T @ np.abs(z64))
    check_elementwise("loss:db", b.grad, dout.sum(0), bound(np.abs(dout).sum(0), M) + 1.01 * e_dout.sum(0))
