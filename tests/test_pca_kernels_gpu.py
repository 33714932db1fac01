"""csrc/pca.hip entry point by entry point through the C ABI, against the fp64 numpy restatement of tests/pca_util.py (NumpyIPCA), on the
frames of tests/golden/pca_kats.npz: every minibatch of every case (the first one without a basis, later ones with basis and
correction row, ragged last ones), for the uint8 / table and the fp32 input forms.  Sentinels sit behind every output and workspace.

Tolerances: the fp64 outputs (statistics, G, the projected basis) are fp64 sums of at most a few thousand products of fp32 inputs,
each rounded to 1.1e-16 — 1e-12 of the output's scale is three orders above that; the fp32 states are one rounding (6e-8) of an
fp64 sum: 1e-6 of their scale."""
import numpy as np
import pytest
import torch

import pca_util as pu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PAD = 64          # sentinel elements behind every output
SENTINEL = -(2.0 ** 100)  # (exact in fp32 and fp64 alike)
TOL64, TOL32 = 1e-12, 1e-6


@pytest.fixture(scope="module")
def kats():
    return pu.load_kats()


@pytest.fixture(scope="module")
def walks(kats):
    """name -> (frames uint8, X float64, the NumpyIPCA steps of every minibatch, the final NumpyIPCA): computed once, never changed."""
    out = {}
    for case in pu.CASES:
        name = pu.case_name(case)
        N, C, W, H, bs, k = case
        frames = kats[name + "/frames"]
        X = pu.normalised(frames, kats["lut"])
        p = pu.NumpyIPCA(k)
        steps = [(b, p.partial_fit(X[b])) for b in pu.minibatches(N, bs) if len(b)]
        out[name] = (frames, X, steps, p)
    return out


def padded(n, dtype=torch.float64):
    """(buffer of n + PAD elements filled with the sentinel, its first n elements)"""
    buf = torch.full((n + PAD,), SENTINEL if dtype.is_floating_point else 0xA5, dtype=dtype, device=DEV)
    return buf, buf[:n]


def intact(buf, n):
    tail = buf[n:].cpu().numpy()
    return bool((tail == (SENTINEL if buf.dtype.is_floating_point else 0xA5)).all())


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


class Frames(object):
    """The two input forms of the entry points as their leading arguments (x_u8, x_f32, lut, plane)."""

    def __init__(self, frames_u8, X64, form):
        from srlz import ops
        self.m, self.D = len(frames_u8), frames_u8[0].size
        if form == "u8":
            self.t = torch.from_numpy(np.ascontiguousarray(frames_u8)).to(DEV)
            self.args = (ops.ptr(self.t), None, ops.ptr(ops.norm_lut(DEV)), int(frames_u8[0, 0].size))
        else:
            self.t = torch.from_numpy(np.ascontiguousarray(X64, dtype=np.float32)).to(DEV)  # (exact: the table's values are float32)
            self.args = (None, ops.ptr(self.t), None, 1)


def test_device_table_is_the_fixture_table(kats):
    from srlz import ops
    assert np.array_equal(ops.norm_lut(DEV).cpu().numpy(), kats["lut"])


@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("case", pu.CASES, ids=pu.case_name)
def test_every_entry_point_on_every_minibatch(cabi, walks, case, form):
    from srlz import ops
    C = cabi
    name = pu.case_name(case)
    k = case[5]
    frames, X, steps, _ = walks[name]
    D = X.shape[1]
    worst = {"stats": 0.0, "gram": 0.0, "project": 0.0}
    state = {"mean": np.zeros(D), "var": np.zeros(D)}
    for b, st in steps:
        f = Frames(frames[b], X[b], form)
        m, first = len(b), int(st["first"])
        r = m if first else k + m + 1
        s = ops.stream()
        # ---- srlz_pca_stats: mean / var in place, bmean, corr
        bufs = {q: padded(D) for q in ("mean", "var", "bmean", "corr")}
        bufs["mean"][1].copy_(dev64(state["mean"]))
        bufs["var"][1].copy_(dev64(state["var"]))
        C.pca_stats(*f.args, m, D, st["n_seen"], *(ops.ptr(bufs[q][1]) for q in ("mean", "var", "bmean", "corr")), s)
        for q in ("mean", "var", "bmean", "corr"):
            assert intact(bufs[q][0], D), "pca_stats wrote behind " + q
            scale = max(np.abs(st[q]).max(), 1e-300)
            if q == "corr" and first:
                assert not bufs[q][1].cpu().numpy().any()
                continue
            worst["stats"] = max(worst["stats"], float(np.abs(bufs[q][1].cpu().numpy() - st[q]).max() / scale))
        state = {"mean": st["mean"], "var": st["var"]}
        # ---- srlz_pca_gram on the numpy state: symmetric, sentinel-clean, twice the same bits
        basis = dev64(st["old_basis"]) if not first else None
        bmean, corr = dev64(st["bmean"]), dev64(st["corr"])
        nbytes = C.pca_workspace(r, D)
        assert nbytes > 0
        runs = []
        for _ in range(2):
            ws_buf, ws = padded(nbytes, torch.uint8)
            g_buf, G = padded(r * r)
            C.pca_gram(ops.ptr(basis), k, first, *f.args, m, ops.ptr(bmean), None if first else ops.ptr(corr), D, ops.ptr(G), ops.ptr(ws),
                       nbytes, s)
            assert intact(ws_buf, nbytes) and intact(g_buf, r * r), "pca_gram wrote behind its workspace or G"
            runs.append(G.cpu().numpy().reshape(r, r))
        assert np.array_equal(runs[0], runs[1]), "pca_gram: two runs differ"
        assert np.array_equal(runs[0], runs[0].T), "G is not exactly symmetric"
        worst["gram"] = max(worst["gram"], rel(runs[0], st["G"]))
        # ---- srlz_pca_project: W·A into a second buffer
        Wd = dev64(st["W"])
        o_buf, out = padded(k * D)
        C.pca_project(ops.ptr(Wd), ops.ptr(basis), k, first, *f.args, m, ops.ptr(bmean), None if first else ops.ptr(corr), D, ops.ptr(out), s)
        assert intact(o_buf, k * D), "pca_project wrote behind its output"
        worst["project"] = max(worst["project"], rel(out.cpu().numpy().reshape(k, D), st["W"].dot(st["A"])))
    print("%s %s: worst relative errors %s" % (name, form, {q: "%.2e" % v for q, v in worst.items()}))
    for q, v in worst.items():
        assert v <= TOL64, "%s: %.3e of the output's scale" % (q, v)


@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("case", pu.CASES, ids=pu.case_name)
def test_transform(cabi, walks, case, form):
    from srlz import ops
    C = cabi
    name = pu.case_name(case)
    k = case[5]
    frames, X, _, p = walks[name]
    N, D = X.shape
    f = Frames(frames, X, form)
    nbytes = C.pca_transform_workspace(N, k, D)
    mean, basis, S = dev64(p.mean), dev64(p.basis), dev64(p.S)
    runs = []
    for _ in range(2):
        ws_buf, ws = padded(nbytes, torch.uint8)
        s_buf, states = padded(N * k, torch.float32)
        C.pca_transform(*f.args, N, ops.ptr(mean), ops.ptr(basis), ops.ptr(S), k, D, ops.ptr(states), ops.ptr(ws), nbytes, ops.stream())
        assert intact(ws_buf, nbytes) and intact(s_buf, N * k), "pca_transform wrote behind its workspace or the states"
        runs.append(states.cpu().numpy().reshape(N, k))
    assert np.array_equal(runs[0], runs[1])
    err = rel(runs[0].astype(np.float64), p.transform(X))
    print("%s %s: states %.2e of scale" % (name, form, err))
    assert err <= TOL32
    # a component without a singular value gives zeros, not a division by zero
    S0 = p.S.copy()
    S0[-1] = 0.0
    s_buf, states = padded(N * k, torch.float32)
    ws_buf, ws = padded(nbytes, torch.uint8)
    C.pca_transform(*f.args, N, ops.ptr(mean), ops.ptr(basis), ops.ptr(dev64(S0)), k, D, ops.ptr(states), ops.ptr(ws), nbytes, ops.stream())
    got = states.cpu().numpy().reshape(N, k)
    assert not got[:, -1].any() and np.array_equal(got[:, :-1], runs[0][:, :-1])


def test_rejected_shapes_return_minus_one_with_a_message(cabi):
    from srlz import ops
    C = cabi
    x = torch.zeros((4, 10), dtype=torch.float32, device=DEV)
    v = torch.zeros(1024, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    px, pv, pw = ops.ptr(x), ops.ptr(v), ops.ptr(ws)
    lib = C._lib
    for what, rc in (
            ("k > m on the first minibatch", lib.srlz_pca_gram(None, 5, 1, None, px, None, 1, 4, pv, None, 10, pv, pw, 1 << 16, None)),
            ("k > D", lib.srlz_pca_gram(pv, 11, 0, None, px, None, 1, 4, pv, pv, 10, pv, pw, 1 << 16, None)),
            ("m < 1", lib.srlz_pca_gram(pv, 3, 0, None, px, None, 1, 0, pv, pv, 10, pv, pw, 1 << 16, None)),
            ("stats m < 1", lib.srlz_pca_stats(None, px, None, 1, 0, 10, 0, pv, pv, pv, pv, None)),
            ("project k > m first", lib.srlz_pca_project(pv, None, 5, 1, None, px, None, 1, 4, pv, None, 10, pv, None)),
            ("transform k > D", lib.srlz_pca_transform(None, px, None, 1, 4, pv, pv, pv, 11, 10, pv, pw, 1 << 16, None)),
            ("uint8 frames whose plane does not divide D", lib.srlz_pca_stats(px, None, pv, 4, 4, 10, 0, pv, pv, pv, pv, None))):
        assert rc == -1, what
        assert C.error_text(), what
    assert lib.srlz_pca_gram(pv, 3, 0, None, px, None, 1, 4, pv, pv, 10, pv, pw, 8, None) == -2 and "workspace" in C.error_text()
    assert lib.srlz_pca_transform(None, px, None, 1, 4, pv, pv, pv, 3, 10, pv, pw, 8, None) == -2 and "workspace" in C.error_text()
    torch.cuda.synchronize()
    assert not v.cpu().numpy().any(), "a rejected call wrote"
