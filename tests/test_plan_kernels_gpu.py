"""csrc/plan.hip on the GPU through the C ABI, against the numpy restatement of plan_util — every comparison exact.

The planner is integer arithmetic except for the returns, and the returns are held to the bits srlz_rollout leaves for the same
plans (the two kernels instantiate one text, csrc/rollout_tile.h), so nothing here has a tolerance.
Shapes: A in {1, 2, 6, 37, 256 = the limit}, K in {1, 31, 32, 33, 257, 1024 = the limit} (below, on and above the 32-row tile, nine and
thirty-two tiles an environment), T in {1, 2, 5, 32 = the limit} (one to eight Philox blocks a plan), N in {1, 3}; for the returns
S in {3, 33, 200, 512} and H in {1, 16, 32}.  A sentinel tail behind every output and the workspace."""
import functools

import numpy as np
import pytest
import torch

import dynamics_util as dy
import plan_util as pu

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL, B_SENTINEL = 1234.5, -77, 0xAB
TAIL = 64
GAMMA = 0.9


def _dev():
    return torch.device("cuda", 0)


def _buffer(numel, dtype, fill):
    return torch.full((numel + TAIL,), fill, dtype=dtype, device=_dev())


def _take(buf, shape, fill, name):
    host = buf.cpu()
    numel = host.numel() - TAIL
    assert bool((host[numel:] == fill).all()), "%s: sentinel tail overwritten" % name
    return host[:numel].view(shape).numpy().copy()


@functools.lru_cache(maxsize=None)
def problem(s, a, h, n, seed=0):
    """Seeded heads and states of one shape (host and device), made once and shared."""
    params = dy.seeded_heads(s, a, h, seed=seed)
    z = dy.sine_states(n, s)
    dev = _dev()
    return dict(params_dev=tuple(p.to(dev) for p in params), z=z, z_dev=torch.from_numpy(z).to(dev), dims=(s, a, h, n))


def cem(pb, k, t, iterations=1, elites=1, q=8, seed=0, init=None, keep=True, z_dev=None, raw=False, head=True, n=None, h=None,
        n_rewards=2, short_ws=0):
    """One srlz_plan_cem call.  Returns (dict of numpy arrays, status); every sentinel tail is checked here."""
    from srlz import _cabi as C
    s, a, h0, n0 = pb["dims"]
    n, h = n0 if n is None else n, h0 if h is None else h
    nn, kk, tt, ii = max(n, 1), max(k, 1), max(t, 1), max(iterations, 1)
    ws_bytes = max(int(C.plan_workspace(nn, min(kk, 1024), min(tt, 32), int(keep))), nn * 8) - short_ws
    bufs = dict(best_plan=_buffer(nn * tt, torch.int32, I_SENTINEL), best_return=_buffer(nn, torch.float32, F_SENTINEL),
                cum=_buffer(nn * tt * a, torch.int32, I_SENTINEL), ws=_buffer(ws_bytes, torch.uint8, B_SENTINEL))
    if keep:
        bufs["plans"] = _buffer(ii * nn * kk * tt, torch.int32, I_SENTINEL)
        bufs["returns"] = _buffer(ii * nn * kk, torch.float32, F_SENTINEL)
    init_dev, stride = None, 0
    if init is not None:
        init_dev = torch.from_numpy(np.asarray(init).astype(np.int32)).to(_dev())
        stride = t * a if init_dev.dim() == 3 else 0
    p = pb["params_dev"]
    heads = [C.ptr(x) for x in p[2:]] if head else [None] * 6
    args = [C.ptr(pb["z_dev"] if z_dev is None else z_dev), C.ptr(p[0]), C.ptr(p[1])] + heads + \
           [C.ptr(init_dev), stride, C.ptr(bufs["best_plan"]), C.ptr(bufs["best_return"]), C.ptr(bufs["cum"]), C.ptr(bufs.get("plans")),
            C.ptr(bufs.get("returns")), C.ptr(bufs["ws"]), ws_bytes, n, k, t, s, a, h, n_rewards, iterations, elites, q, GAMMA, seed,
            C.stream()]
    status = C._lib.srlz_plan_cem(*args) if raw else C.plan_cem(*args)
    torch.cuda.synchronize()
    fills = dict(best_plan=I_SENTINEL, best_return=F_SENTINEL, cum=I_SENTINEL, ws=B_SENTINEL, plans=I_SENTINEL, returns=F_SENTINEL)
    shapes = dict(best_plan=(nn, tt), best_return=(nn,), cum=(nn, tt, a), ws=(ws_bytes,), plans=(ii, nn, kk, tt), returns=(ii, nn, kk))
    out = {q_: _take(b, shapes[q_], fills[q_], q_) for q_, b in bufs.items()}
    out["cum"] = out["cum"].view(np.uint32)
    out["tickets"] = out["ws"][:nn * 4].copy().view(np.uint32)
    return out, status


def rollout_returns(pb, plans, z_dev=None):
    """fp32 [N,K]: srlz_rollout's returns for plans int32 [N,K,T]."""
    from srlz import _cabi as C
    s, a, h, _ = pb["dims"]
    n, k, t = plans.shape
    pl = torch.from_numpy(np.ascontiguousarray(plans, np.int32)).to(_dev())
    final, ret = _buffer(n * k * s, torch.float32, F_SENTINEL), _buffer(n * k, torch.float32, F_SENTINEL)
    p = pb["params_dev"]
    C.rollout(C.ptr(pb["z_dev"] if z_dev is None else z_dev), C.ptr(pl), k * t, C.ptr(p[0]), C.ptr(p[1]), *[C.ptr(x) for x in p[2:]],
              C.ptr(final), C.ptr(ret), None, None, n, k, t, s, a, h, 2, GAMMA, C.stream())
    torch.cuda.synchronize()
    return _take(ret, (n, k), F_SENTINEL, "rollout returns")


def same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))


#               A    K     T  N
POPULATIONS = [(1, 1, 1, 1),
               (2, 31, 2, 3),
               (6, 32, 5, 1),
               (6, 33, 5, 3),
               (37, 257, 5, 1),
               (256, 33, 32, 3),
               (6, 1024, 2, 1),
               (256, 1024, 32, 1)]


@pytest.mark.parametrize("shape", POPULATIONS, ids=lambda v: "A%d_K%d_T%d_N%d" % v)
def test_first_population_is_the_restatements_bit_for_bit(shape):
    a, k, t, n = shape
    pb = problem(3, a, 16, n)
    seed = 2 ** 40 + 5
    got = cem(pb, k, t, seed=seed)[0]
    assert np.array_equal(got["plans"][0], pu.sample(pu.uniform_cum(n, t, a), seed, 0, k))
    assert not got["tickets"].any()
    # with a table of the caller's: one shared [T,A] with zero-weight actions, and one per environment
    w = (np.arange(t * a).reshape(t, a) * 7 % 5).astype(np.int64)
    w[:, -1] += 1
    got = cem(pb, k, t, seed=seed, init=w)[0]
    assert np.array_equal(got["plans"][0], pu.sample(pu.cum_of(w, n), seed, 0, k))
    wn = np.stack([(w + 3 * e) % 11 + (np.arange(a) == e % a) for e in range(n)])
    got = cem(pb, k, t, seed=seed, init=wn)[0]
    assert np.array_equal(got["plans"][0], pu.sample(pu.cum_of(wn, n), seed, 0, k))


def test_a_sample_does_not_depend_on_the_size_of_the_call():
    big = cem(problem(3, 6, 16, 3), 33, 5, seed=9)[0]
    small = cem(problem(3, 6, 16, 1), 4, 5, seed=9)[0]
    assert np.array_equal(big["plans"][0, 0, :4], small["plans"][0, 0])
    assert same_bits(big["returns"][0, 0, :4], small["returns"][0, 0])


@pytest.mark.parametrize("shape", [(3, 6, 16, 3, 33, 5), (33, 37, 1, 1, 257, 2), (200, 6, 16, 3, 64, 10), (200, 6, 32, 1, 31, 7),
                                   (512, 6, 16, 1, 33, 5), (512, 256, 32, 2, 40, 32)],
                         ids=lambda v: "S%d_A%d_H%d_N%d_K%d_T%d" % v)
def test_population_returns_are_srlz_rollouts_bits(shape):
    s, a, h, n, k, t = shape
    pb = problem(s, a, h, n)
    got = cem(pb, k, t, iterations=2, elites=min(4, k), seed=3)[0]
    for i in range(2):
        assert same_bits(got["returns"][i], rollout_returns(pb, got["plans"][i])), i
    assert np.isfinite(got["returns"]).all() and got["returns"].std() > 0


def _held_to_the_restatement(pb, k, t, iterations, elites, q, seed, init=None, z_dev=None):
    s, a, h, n = pb["dims"]
    ref = pu.cem(lambda pl: rollout_returns(pb, pl, z_dev), n, k, t, a, iterations, elites, q, seed, init_weights=init)
    for upto in range(1, iterations + 1):  # (a run of j iterations leaves the table the j-th refit made)
        got = cem(pb, k, t, iterations=upto, elites=elites, q=q, seed=seed, init=init, z_dev=z_dev)[0]
        assert np.array_equal(got["cum"], ref["cums"][upto]), upto
        assert np.array_equal(got["plans"], ref["plans"][:upto]), upto
        assert same_bits(got["returns"], ref["returns"][:upto]), upto
    assert np.array_equal(got["best_plan"], ref["best_plan"])
    assert same_bits(got["best_return"], ref["best_return"])
    assert not got["tickets"].any()
    # without the population the same results
    lean = cem(pb, k, t, iterations=iterations, elites=elites, q=q, seed=seed, init=init, z_dev=z_dev, keep=False)[0]
    for name in ("best_plan", "cum"):
        assert np.array_equal(lean[name], got[name]), name
    assert same_bits(lean["best_return"], got["best_return"])
    return got, ref


@pytest.mark.parametrize("shape", [(3, 6, 16, 3, 33, 5, 8), (200, 6, 16, 2, 64, 10, 8), (33, 37, 32, 1, 257, 7, 32), (8, 2, 16, 3, 31, 32, 1)],
                         ids=lambda v: "S%d_A%d_H%d_N%d_K%d_T%d_E%d" % v)
def test_three_iterations_are_exact_against_the_restatement(shape):
    s, a, h, n, k, t, e = shape
    got, ref = _held_to_the_restatement(problem(s, a, h, n), k, t, 3, e, 8, 5)
    assert (ref["history"][-1] >= ref["history"][0]).all()
    assert not np.array_equal(got["plans"][0], got["plans"][2])


def test_three_iterations_from_a_table_of_the_callers():
    n, t, a = 3, 5, 6
    w = np.ones((n, t, a), np.int64)
    w[1, :, 2] = 30
    w[2, 3] = [0, 0, 5, 0, 0, 1]
    got, _ = _held_to_the_restatement(problem(3, a, 16, n), 33, t, 3, 8, 8, 5, init=w)
    assert (got["plans"][0, 1] == 2).mean() > 0.5 and set(np.unique(got["plans"][0, 2, :, 3])) <= {2, 5}
    _held_to_the_restatement(problem(3, a, 16, n), 33, t, 2, 8, 4096, 5, init=w[0])  # shared [T,A], the sharpest refit


def test_ties_go_to_the_lowest_k():
    n, k, t, e, q = 2, 70, 5, 8, 8
    got = cem(problem(8, 1, 16, n), k, t, iterations=2, elites=e, q=q)[0]  # A = 1: every plan is the same plan
    assert not got["plans"].any() and not got["best_plan"].any()
    for env in range(n):
        assert len(set(got["returns"][:, env].view(np.uint32).ravel())) == 1
    assert same_bits(got["best_return"], got["returns"][0, :, 0])
    assert (got["cum"] == 1 + q * e).all()  # refit from E elites: which ones cannot show at A = 1 ...
    # ... so with A = 6 and a state of NaN: every key is -inf, the elites are k = 0 .. E-1 and the best is iteration 0's k = 0
    pb = problem(8, 6, 16, 3)
    z = pb["z"].copy()
    z[1, 2] = np.nan
    z_dev = torch.from_numpy(z).to(_dev())
    sick = cem(pb, k, t, iterations=2, elites=e, q=q, z_dev=z_dev)[0]
    well = cem(pb, k, t, iterations=2, elites=e, q=q)[0]
    assert np.isnan(sick["returns"][:, 1]).all() and np.isnan(sick["best_return"][1])
    assert np.array_equal(sick["best_plan"][1], sick["plans"][0, 1, 0])
    assert np.array_equal(sick["cum"][1], pu.refit(sick["plans"][1, 1, :e], 6, q))
    assert np.array_equal(sick["plans"][1, 1], pu.sample(pu.refit(sick["plans"][0, 1, :e], 6, q)[None], 0, 1, k, n0=1)[0])
    for env in (0, 2):  # the neighbours keep the bits they have without it
        for name in ("plans", "returns"):
            assert np.array_equal(sick[name][:, env].view(np.uint32), well[name][:, env].view(np.uint32)), (env, name)
        for name in ("best_plan", "best_return", "cum"):
            assert np.array_equal(sick[name][env].view(np.uint32), well[name][env].view(np.uint32)), (env, name)
    _held_to_the_restatement(pb, k, t, 2, e, q, 0, z_dev=z_dev)


def test_two_runs_give_the_same_bits_and_another_seed_another_population():
    pb = problem(200, 6, 16, 3)
    one, two = cem(pb, 257, 10, iterations=3, elites=16, seed=1)[0], cem(pb, 257, 10, iterations=3, elites=16, seed=1)[0]
    for name in ("plans", "returns", "best_plan", "best_return", "cum", "tickets"):
        assert np.array_equal(one[name].view(np.uint32), two[name].view(np.uint32)), name
    assert not one["tickets"].any()
    other = cem(pb, 257, 10, iterations=3, elites=16, seed=2)[0]
    assert not np.array_equal(one["plans"][0], other["plans"][0])
    high = cem(pb, 257, 10, iterations=1, elites=16, seed=1 + 2 ** 32)[0]  # the seed's upper word is the second key word
    assert not np.array_equal(one["plans"][0], high["plans"][0])
    assert (one["best_return"] >= one["returns"][0].max(axis=1)).all()  # best so far starts at iteration 0's best
    assert same_bits(one["best_return"], one["returns"].max(axis=(0, 2)))


REFUSED = [dict(k=1025), dict(k=0), dict(t=33), dict(t=0), dict(n=0), dict(iterations=0), dict(elites=0), dict(elites=34), dict(q=-1),
           dict(q=4097), dict(head=False), dict(h=33), dict(n_rewards=3), dict(keep="half"), dict(stride=7)]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "_".join("%s%s" % kv for kv in c.items()))
def test_refused_calls_return_minus_one_and_write_nothing(case):
    from srlz import _cabi as C
    kw = dict(k=33, t=5, iterations=2, elites=8, q=8, raw=True)
    kw.update({key: v for key, v in case.items() if key not in ("keep", "stride")})
    pb = problem(3, 6, 16, 2)
    if "keep" in case or "stride" in case:
        # half a population / an init stride that is neither 0 nor T * A: straight through the binding
        s, a, h, n = pb["dims"]
        p = pb["params_dev"]
        bufs = [_buffer(64 * 1024, torch.int32, I_SENTINEL) for _ in range(5)]
        best_plan, best_return, cum, plans, ws = bufs
        args = [C.ptr(pb["z_dev"]), C.ptr(p[0]), C.ptr(p[1])] + [C.ptr(x) for x in p[2:]] + \
               [C.ptr(cum) if "stride" in case else None, case.get("stride", 0), C.ptr(best_plan), C.ptr(best_return), C.ptr(cum),
                C.ptr(plans) if "keep" in case else None, None, C.ptr(ws), 4 * ws.numel(), n, 33, 5, s, a, h, 2, 2, 8, 8, GAMMA, 0,
                C.stream()]
        status = C._lib.srlz_plan_cem(*args)
        torch.cuda.synchronize()
        assert status == -1, C.error_text()
        for b in bufs:
            assert bool((b == I_SENTINEL).all())
        return
    out, status = cem(pb, **kw)
    assert status == -1, C.error_text()
    assert "plan_cem" in C.error_text()
    for name, fill in (("best_plan", I_SENTINEL), ("plans", I_SENTINEL), ("best_return", F_SENTINEL), ("returns", F_SENTINEL),
                       ("ws", B_SENTINEL)):
        assert (out[name] == fill).all(), name
    assert (out["cum"].view(np.int32) == I_SENTINEL).all()


def test_short_workspace_and_null_pointers_have_their_own_codes():
    from srlz import _cabi as C
    pb = problem(3, 6, 16, 2)
    out, status = cem(pb, 33, 5, iterations=2, elites=8, raw=True, short_ws=1)
    assert status == -2 and (out["ws"] == B_SENTINEL).all() and (out["best_plan"] == I_SENTINEL).all()
    out, status = cem(pb, 33, 5, iterations=2, elites=8, raw=True, keep=False, short_ws=1)
    assert status == -2 and (out["ws"] == B_SENTINEL).all()
    with pytest.raises(C.SrlzError, match="workspace"):
        cem(pb, 33, 5, iterations=2, elites=8, short_ws=1)
