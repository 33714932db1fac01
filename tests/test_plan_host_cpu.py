"""The deployment planner on the host side (no GPU): Philox4x32-10's known answers against the restatement of plan_util and against
srlz.deploy's own sampler; the sampler's edges; the new symbols in header, library and binding; the limits of srlz_plan_supported; the
route table of LatentDynamics.plan; argument validation before any GPU call; and the host fallback's whole cross-entropy loop against
the restatement on a toy return."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import plan_util as pu
from test_dynamics_host_cpu import _modules, _split

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srlz_plan_supported", "srlz_plan_workspace", "srlz_plan_cem")
TOY_SEEDS = list(range(8)) + [2 ** 40 + 5]


@pytest.mark.parametrize("kat", pu.PHILOX_KATS, ids=["zeros", "ones", "pi"])
def test_philox_known_answers_restatement_and_implementation(kat):
    from srlz import deploy
    counter, key, want = kat
    assert tuple(int(w) for w in pu.philox(counter, key)) == want
    assert tuple(int(w) for w in deploy.philox4x32_10([np.uint64(c) for c in counter], key)) == want
    # vectorised: the answer of each lane is its own
    both = deploy.philox4x32_10([np.array([c, pu.PHILOX_KATS[0][0][i]], np.uint64) for i, c in enumerate(counter)], key)
    assert tuple(int(w[0]) for w in both) == want


def test_implementation_samples_what_the_restatement_samples():
    from srlz import deploy
    rng = np.random.RandomState(0)
    for n, k, t, a in ((1, 1, 1, 1), (2, 5, 7, 6), (3, 33, 9, 37), (1, 4, 32, 256)):
        cum = np.cumsum(rng.randint(0, 50, size=(n, t, a)) + (rng.rand(n, t, a) < 0.2), axis=2).astype(np.uint32)
        cum[:, :, -1] += 1  # a positive total in every row
        for seed, it in ((0, 0), (2 ** 40 + 5, 3), (2 ** 64 - 1, 1)):
            assert np.array_equal(deploy.sample_plans(cum, seed, it, k), pu.sample(cum, seed, it, k)), (n, k, t, a, seed)
    # a sample depends on (seed, i, n, k, t) and its row alone: a sub-block of a larger population is the smaller one
    cum = pu.uniform_cum(3, 5, 6)
    big, small = pu.sample(cum, 7, 2, 33), pu.sample(cum[:1], 7, 2, 4)
    assert np.array_equal(big[0, :4], small[0])
    assert np.array_equal(pu.sample(cum[1:2], 7, 2, 9, n0=1, k0=20)[0], big[1, 20:29])


def test_sampler_edges():
    from srlz import deploy
    top = 2 ** 32 - 1
    for row in ([1, 2, 3, 4, 5, 6], [5], [0, 0, 3, 3, 10], [7, 7, 7, 9], [2 ** 31, 2 ** 32 - 1]):
        for u in (0, 1, top // 2, top - 1, top):
            got = int(deploy.sample_actions(np.array([u], np.uint64), np.array(row, np.uint32))[0])
            assert got == pu.pick(u, row), (row, u)
    assert pu.pick(0, [1, 2, 3]) == 0 and pu.pick(top, [1, 2, 3]) == 2     # u = 0 the first action, u = 2^32 - 1 the last
    assert pu.pick(0, [0, 0, 3, 3, 10]) == 2                                # never an action of weight 0
    # a table with zero-weight actions never yields them; A = 1 yields action 0
    w = np.array([[0, 3, 0, 1, 0, 2]] * 4)
    pl = deploy.sample_plans(pu.cum_of(w, 2), 11, 0, 257)
    assert set(np.unique(pl)) == {1, 3, 5}
    assert not deploy.sample_plans(pu.uniform_cum(2, 3, 1), 11, 0, 40).any()
    assert np.array_equal(pl, pu.sample(pu.cum_of(w, 2), 11, 0, 257))


def test_header_library_and_binding_agree_on_the_new_symbols(cabi):
    text = open(os.path.join(REPO, "include", "srlz.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(cabi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in cabi.EXPORTED, name
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).strip()
        assert len(cabi._PROTOS[name][1]) == decl.count(",") + 1, name  # one binding argument per parameter
    assert cabi.version() == cabi.ABI_VERSION == 104  # the additions are backward compatible


def test_supported_at_each_limit_and_one_past_it(cabi):
    ok = cabi.plan_supported
    for s, a, h, k, t in ((1, 1, 1, 1, 1), (200, 6, 16, 64, 10), (512, 256, 32, 1024, 32), (3, 256, 16, 1, 32), (3, 6, 16, 1024, 1)):
        assert ok(s, a, h, 2, k, t) == 1, (s, a, h, k, t)
        assert cabi.rollout_supported(s, a, h, 2) == 1
    for s, a, h, nr, k, t in ((513, 6, 16, 2, 64, 10), (0, 6, 16, 2, 64, 10), (200, 257, 16, 2, 64, 10), (200, 0, 16, 2, 64, 10),
                              (200, 6, 33, 2, 64, 10), (200, 6, 0, 2, 64, 10), (200, 6, 16, 3, 64, 10), (200, 6, 16, 2, 1025, 10),
                              (200, 6, 16, 2, 0, 10), (200, 6, 16, 2, 64, 33), (200, 6, 16, 2, 64, 0)):
        assert ok(s, a, h, nr, k, t) == 0, (s, a, h, nr, k, t)
    assert cabi.rollout_supported(200, 257, 16, 2) == 1  # the rollout kernel's own limit on A is wider
    from srlz import ops
    assert ops.plan_supported(200, 6, 16, 2, 64, 10) and not ops.plan_supported(200, 6, 16, 2, 64, 33)
    # the workspace: tickets and best keys, plus one iteration's population when the caller keeps none; 0 for a refused shape
    assert ops.plan_workspace(3, 33, 5, True) == 3 * 8
    assert ops.plan_workspace(3, 33, 5, False) == 3 * 8 + 3 * 33 * 4 + 3 * 33 * 5 * 4
    assert ops.plan_workspace(0, 33, 5) == 0 and ops.plan_workspace(3, 1025, 5) == 0 and ops.plan_workspace(3, 33, 33) == 0


def test_route_table():
    from srlz import deploy
    m = _modules(8, ["forward", "reward"])
    assert deploy.plan_route_for(m, 64, 10) == "rollout"
    assert deploy.plan_route_for(m, 1024, 32) == "rollout"
    assert deploy.plan_route_for(m, 1025, 10) == "model"                  # K over the limit
    assert deploy.plan_route_for(m, 64, 33) == "model"                    # T over the limit
    assert deploy.plan_route_for(m, 64, 10, n_envs=128) == "rollout"
    assert deploy.plan_route_for(m, 64, 10, n_envs=129) == "model"        # beyond max_rows
    assert deploy.plan_route_for(m, 64, 10, n_envs=129, max_rows=16384) == "rollout"
    assert deploy.plan_route_for(_split(), 64, 10) == "model"             # the heads see masked states
    assert deploy.plan_route_for(_modules(513, ["forward", "reward"]), 64, 10) == "model"
    import preprocessing.preprocess as pre
    from models.modules import SRLModules
    pre.N_CHANNELS = 3
    many = SRLModules(state_dim=8, action_dim=257, cuda=False, losses=["forward", "reward"])
    assert deploy.dynamics_route_for(many) == "rollout" and deploy.plan_route_for(many, 64, 10) == "model"  # A over the planner's limit


def test_arguments_are_validated_before_any_gpu_call():
    from srlz import deploy
    assert deploy.check_plan_args(10, 64, 4, 8, 8, 0) == (10, 64, 4, 8, 8, 0)
    assert deploy.check_plan_args(np.int64(1), 1, 1, 1, 0, 2 ** 64 - 1) == (1, 1, 1, 1, 0, 2 ** 64 - 1)
    for bad, match in (((0, 64, 4, 8, 8, 0), "at least 1"), ((10, 0, 4, 8, 8, 0), "at least 1"), ((10, 64, 0, 8, 8, 0), "at least 1"),
                       ((10, 64, 4, 0, 8, 0), "elites"), ((10, 64, 4, 65, 8, 0), "elites"), ((10, 64, 4, 8, -1, 0), "sharpness"),
                       ((10, 64, 4, 8, 4097, 0), "sharpness"), ((10, 64, 4, 8, 8, -1), "seed"), ((10, 64, 4, 8, 8, 2 ** 64), "seed"),
                       ((10.0, 64, 4, 8, 8, 0), "integer"), ((10, 64, 4, 8, True, 0), "integer")):
        with pytest.raises(ValueError, match=match):
            deploy.check_plan_args(*bad)
    w = np.ones((7, 6), np.int64)
    assert deploy.check_init_weights(None, 3, 7, 6) == (None, True)
    assert deploy.check_init_weights(w, 3, 7, 6)[1] is True
    assert deploy.check_init_weights(np.ones((3, 7, 6), np.int32), 3, 7, 6)[1] is False
    assert deploy.check_init_weights(torch.ones((3, 7, 6), dtype=torch.int32), 3, 7, 6)[1] is False
    for bad, match in ((w.astype(np.float32), "integers"), (np.ones((6, 7), np.int64), "shape"), (np.ones((2, 7, 6), np.int64), "shape"),
                       ([[1] * 6] * 7, "numpy array or a torch tensor")):
        with pytest.raises(ValueError, match=match):
            deploy.check_init_weights(bad, 3, 7, 6)
    neg, zero, huge = w.copy(), w.copy(), w.copy()
    neg[2, 3] = -1
    zero[4] = 0
    huge[:] = 2 ** 31 - 1
    with pytest.raises(ValueError, match="non-negative"):
        deploy.check_init_weights(neg, 3, 7, 6)
    with pytest.raises(ValueError, match="positive total"):
        deploy.check_init_weights(zero, 3, 7, 6)
    with pytest.raises(ValueError, match="positive total"):
        deploy.check_init_weights(huge, 3, 7, 6)


@pytest.mark.parametrize("seed", TOY_SEEDS)
def test_host_fallback_is_the_restatement_on_a_toy_return(seed):
    from srlz import deploy
    c = pu.TOY
    n = 2
    got = deploy.cem_host(pu.toy_returns, n, c["k"], c["t"], c["a"], c["iterations"], c["elites"], c["q"], seed, keep_population=True)
    ref = pu.cem(pu.toy_returns, n, c["k"], c["t"], c["a"], c["iterations"], c["elites"], c["q"], seed)
    for q in ("plans", "returns", "cum", "best_plan", "best_return", "history"):
        assert np.array_equal(got[q], ref[q]), q
    assert (got["best_return"] == c["t"]).all(), got["best_return"]          # the full return after six iterations
    assert (np.diff(got["history"], axis=0) >= 0).all()                      # best so far never decreases
    assert np.array_equal(pu.toy_returns(got["best_plan"]), got["best_return"])
    assert not np.array_equal(got["plans"][0, 0], got["plans"][0, 1])        # environments draw their own plans
    # with a table of its own, per environment
    w = np.ones((n, c["t"], c["a"]), np.int64)
    w[1, :, 0] = 40
    got = deploy.cem_host(pu.toy_returns, n, c["k"], c["t"], c["a"], 2, c["elites"], c["q"], seed, init_weights=w, keep_population=True)
    ref = pu.cem(pu.toy_returns, n, c["k"], c["t"], c["a"], 2, c["elites"], c["q"], seed, init_weights=w)
    for q in ("plans", "returns", "cum", "best_plan", "best_return"):
        assert np.array_equal(got[q], ref[q]), q
    assert (got["plans"][0, 1] == 0).mean() > 0.5 > (got["plans"][0, 0] == 0).mean()


def test_shifted_table_and_select_rules_of_the_restatement():
    cum = pu.refit(np.array([[0, 1, 2], [0, 1, 1]]), 3, 8)
    assert np.array_equal(pu.weights_of(cum), [[17, 1, 1], [1, 17, 1], [1, 9, 9]])
    assert np.array_equal(pu.shifted(cum), [[1, 17, 1], [1, 9, 9], [1, 1, 1]])
    el, key = pu.select(np.array([1.0, np.nan, 3.0, 3.0, -np.inf], np.float32), 5)
    assert list(el) == [2, 3, 0, 1, 4] and key[1] == -np.inf                  # NaN reads as -inf, ties go to the lower k
