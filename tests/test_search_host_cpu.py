"""The tree search on the host side (no GPU): the tree's sizes against hand-computed tables; the host algorithm (srlz.deploy.beam_host)
on toy deterministic scorers — exact search against brute force, W = 1 greedy, ties, NaN; argument validation; the route table of
LatentDynamics.search; the new symbols in header, library and binding; the limits of srlz_beam_supported; and reach's default planner."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from test_dynamics_host_cpu import _modules, _split

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srlz_beam_supported", "srlz_beam_workspace", "srlz_beam_leaves", "srlz_beam_search")


def all_plans(a, t):
    return np.array(list(itertools.product(range(a), repeat=t)), np.int32)


# ---- sizes ----
@pytest.mark.parametrize("beam,horizon,a,frontier,children,exact", [
    (1, 4, 3, [1, 1, 1, 1], [3, 3, 3, 3], False),                       # greedy
    (64, 5, 6, [1, 6, 36, 64, 64], [6, 36, 216, 384, 384], False),      # the default beam on the arm's six actions
    (36, 3, 6, [1, 6, 36], [6, 36, 216], True),                         # W = A^(T-1): the boundary
    (35, 3, 6, [1, 6, 35], [6, 36, 210], False),                        # one below it
    (27, 4, 3, [1, 3, 9, 27], [3, 9, 27, 81], True),
    (26, 4, 3, [1, 3, 9, 26], [3, 9, 27, 78], False),
    (1, 1, 6, [1], [6], True),                                          # one step is always exact
    (1000, 3, 2, [1, 2, 4], [2, 4, 8], True),                           # a beam wider than the tree
    (5, 3, 1, [1, 1, 1], [1, 1, 1], True),                              # one action
])
def test_search_sizes_against_hand_computed_tables(beam, horizon, a, frontier, children, exact):
    from srlz import deploy
    got = deploy.search_sizes(beam, horizon, a)
    assert got["frontier"] == frontier and got["children"] == children
    assert got["leaves"] == children[-1] and got["expanded"] == sum(children) and got["exact"] is exact


def test_exact_search_counts_every_prefix_once():
    from srlz import deploy
    got = deploy.search_sizes(6 ** 4, 5, 6)
    assert got["exact"] and got["leaves"] == 7776 and got["expanded"] == 9330 and 5 * 7776 == 38880  # the issue's derived count


def test_sizes_agree_with_the_library(cabi):
    from srlz import deploy
    for w, a, t in ((1, 3, 4), (64, 6, 5), (36, 6, 3), (35, 6, 3), (4096, 2, 2), (2048, 4, 8), (1, 1, 32)):
        assert cabi.beam_leaves(w, a, t) == deploy.search_sizes(w, t, a)["leaves"], (w, a, t)


# ---- the host algorithm on toy scorers ----
def toy_score(plans):
    """fp32 [N,C]: a deterministic return with no ties — sum_t 0.9^t v(n, t, a_t), v a fixed table of distinct irrational values;
    a prefix's score is the prefix of the sum, as a rollout's return is."""
    n, c, t = plans.shape
    e, step = np.meshgrid(np.arange(n), np.arange(t), indexing="ij")
    v = np.sin(1.7 * e[:, None, :] + 2.3 * step[:, None, :] + 0.9 * plans * (1 + step[:, None, :]) + 0.3)
    return (v * 0.9 ** np.arange(t)).sum(axis=2).astype(np.float32)


@pytest.mark.parametrize("a,t", [(2, 6), (3, 4), (6, 3), (4, 1)])
def test_exact_host_search_is_brute_force(a, t):
    from srlz import deploy
    n, plans = 3, all_plans(a, t)
    got = deploy.beam_host(toy_score, n, a ** (t - 1), t, a)
    brute = toy_score(np.broadcast_to(plans, (n,) + plans.shape))
    assert got["exact"] and np.array_equal(got["leaf_plans"], np.broadcast_to(plans, (n,) + plans.shape))
    assert np.array_equal(got["leaf_returns"], brute)
    top = brute.argmax(axis=1)
    assert np.array_equal(got["best_plan"], plans[top]) and np.array_equal(got["best_return"], brute[np.arange(n), top])
    assert got["best_plan"].dtype == np.int32 and got["best_return"].dtype == np.float32
    # one below the boundary something is pruned, and the answer can only be worse or equal
    if t > 1 and a > 1:
        less = deploy.beam_host(toy_score, n, a ** (t - 1) - 1, t, a)
        assert not less["exact"] and (less["best_return"] <= got["best_return"]).all()
        assert less["leaf_plans"].shape == (n, (a ** (t - 1) - 1) * a, t)


def test_beam_of_one_is_greedy():
    from srlz import deploy
    n, a, t = 3, 4, 5
    got = deploy.beam_host(toy_score, n, 1, t, a)
    want = np.zeros((n, 0), np.int32)
    for step in range(t):
        cand = np.stack([np.concatenate((want, np.full((n, 1), x, np.int32)), axis=1) for x in range(a)], axis=1)
        want = cand[np.arange(n), toy_score(cand).argmax(axis=1)]
    assert np.array_equal(got["best_plan"], want) and got["leaf_plans"].shape == (n, a, t) and got["expanded"] == a * t
    assert np.array_equal(got["leaf_plans"][:, :, :-1], np.repeat(want[:, None, :-1], a, axis=1))


@pytest.mark.parametrize("beam", [1, 2, 9])
def test_ties_keep_the_lowest_indices(beam):
    from srlz import deploy
    got = deploy.beam_host(lambda pl: np.full(pl.shape[:2], 0.5 * pl.shape[2], np.float32), 2, beam, 3, 3)
    assert not got["best_plan"].any() and (got["best_return"] == 1.5).all()
    if beam == 2:
        want = np.array([(0, 0, x) for x in range(3)] + [(0, 1, x) for x in range(3)], np.int32)
        assert np.array_equal(got["leaf_plans"], np.broadcast_to(want, (2,) + want.shape))
    # -0 and +0 are one key
    got = deploy.beam_host(lambda pl: np.where(pl[:, :, -1] == 0, np.float32(-0.0), np.float32(0.0)), 1, 2, 3, 3)
    assert not got["best_plan"].any()


@pytest.mark.parametrize("beam", [1, 2, 4])
def test_nan_is_never_chosen_over_a_number_and_an_all_nan_environment_reports_nan(beam):
    from srlz import deploy

    def score(pl):  # environment 0: every plan that starts with action 0 is NaN, the rest -5 - (its actions' sum); environment 1: all NaN
        r = -5.0 - pl.sum(axis=2).astype(np.float32)
        r[0][pl[0, :, 0] == 0] = np.nan
        r[1] = np.nan
        return r
    got = deploy.beam_host(score, 2, beam, 3, 2)
    assert np.array_equal(got["best_plan"][0], [1, 0, 0]) and got["best_return"][0] == -6.0
    assert np.isnan(got["best_return"][1]) and not got["best_plan"][1].any()
    if beam < 4:  # (beam 4 prunes nothing: the leaves are in child-index order)
        assert not np.isnan(got["leaf_returns"][0, 0])  # the first leaf kept is a number: NaN orders last


# ---- arguments ----
def test_arguments_are_validated_before_any_gpu_call():
    from srlz import deploy
    assert deploy.check_search_args(10, 64) == (10, 64) and deploy.check_search_args(np.int64(1), np.int32(1)) == (1, 1)
    for bad, match in (((0, 64), "at least 1"), ((10, 0), "at least 1"), ((-1, 1), "at least 1"), ((10.0, 64), "integer"),
                       ((10, 64.0), "integer"), ((True, 64), "integer"), ((10, None), "integer")):
        with pytest.raises(ValueError, match=match):
            deploy.check_search_args(*bad)
    with pytest.raises(ValueError, match="at least 1"):
        deploy.search_sizes(0, 3, 6)
    with pytest.raises(ValueError, match="n_actions"):
        deploy.search_sizes(4, 3, 0)
    with pytest.raises(ValueError, match="at least 1"):
        deploy.beam_host(toy_score, 1, 4, 0, 3)


def test_route_table():
    from srlz import deploy
    m = _modules(8, ["forward", "reward"])                                # A = 6
    assert deploy.search_route_for(m, 64, 10) == "rollout"
    assert deploy.search_route_for(m, 1296, 5) == "rollout"               # exact at T = 5: 7776 children
    assert deploy.search_route_for(m, 1365, 32) == "rollout"              # W * A = 8190
    assert deploy.search_route_for(m, 1366, 32) == "model"                # W * A = 8196 over the limit
    assert deploy.search_route_for(m, 10 ** 9, 3) == "rollout"            # a beam wider than the tree counts as the tree
    assert deploy.search_route_for(m, 10 ** 9, 6) == "model"              # 6^6 leaves
    assert deploy.search_route_for(m, 64, 33) == "model"                  # T over the limit
    assert deploy.search_route_for(m, 64, 10 ** 6) == "model"
    assert deploy.search_route_for(m, 64, 10, n_envs=21) == "rollout"     # 21 * 384 = 8064 children a level
    assert deploy.search_route_for(m, 64, 10, n_envs=22) == "model"       # beyond max_rows
    assert deploy.search_route_for(m, 64, 10, n_envs=22, max_rows=16384) == "rollout"
    assert deploy.search_route_for(_split(), 64, 10) == "model"           # the heads see masked states
    assert deploy.search_route_for(_modules(513, ["forward", "reward"]), 64, 10) == "model"
    # a goal-only call does not look at the reward head's shape
    odd = _modules(8, ["forward", "reward"])
    import torch
    odd.reward_net = torch.nn.Linear(16, 2)
    assert deploy.search_route_for(odd, 64, 10) == "model" and deploy.search_route_for(odd, 64, 10, has_goal_only=True) == "rollout"
    # the existing tables are what they were
    assert deploy.plan_route_for(m, 64, 10) == "rollout" and deploy.plan_route_for(m, 1025, 10) == "model"


# ---- the C ABI ----
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
    section = text[text.index("Deployment tree search"):text.index("int srlz_beam_supported")]
    assert "forward_inverse.py:21-31" in section and ":78-95" in section  # the entry cites the reference lines it composes


def test_supported_at_each_limit_and_one_past_it(cabi):
    ok = cabi.beam_supported
    for s, a, h, r, w, t in ((1, 1, 1, 1, 1, 1), (200, 6, 16, 1, 64, 10), (512, 2, 32, 1, 4096, 32), (3, 8192, 16, 1, 1, 32),
                             (200, 6, 0, 0, 1365, 1), (512, 6, 99, 0, 64, 10)):
        assert ok(s, a, h, 2 if r else 0, r, w, t) == 1, (s, a, h, r, w, t)
    for s, a, h, nr, r, w, t in ((513, 6, 16, 2, 1, 64, 10), (0, 6, 16, 2, 1, 64, 10), (200, 0, 16, 2, 1, 64, 10), (200, 6, 33, 2, 1, 64, 10),
                                 (200, 6, 0, 2, 1, 64, 10), (200, 6, 16, 3, 1, 64, 10), (200, 6, 16, 2, 1, 1366, 10),
                                 (200, 2, 16, 2, 1, 4097, 2), (200, 6, 16, 2, 1, 0, 10), (200, 6, 16, 2, 1, 64, 33), (200, 6, 16, 2, 1, 64, 0),
                                 (200, 8193, 16, 2, 1, 1, 3), (200, 6, 16, 2, 1, 2 ** 30, 10)):
        assert ok(s, a, h, nr, r, w, t) == 0, (s, a, h, nr, r, w, t)
    from srlz import ops
    assert ops.beam_supported(200, 6, 16, 2, True, 64, 10) and not ops.beam_supported(200, 6, 16, 2, True, 64, 33)
    assert ops.beam_leaves(64, 6, 5) == 384 and ops.beam_leaves(1366, 6, 5) == 0
    # the workspace: tickets (padded to 16 bytes), two return buffers [N,L], the frontiers [T-1,N,W], two state buffers [N,C_{T-2},S]
    n, w, t, s, a = 3, 5, 4, 33, 3       # C = 3, 9, 15, 15
    assert ops.beam_workspace(n, w, t, s, a) == 16 + 2 * n * 15 * 4 + (t - 1) * n * w * 4 + 2 * n * 15 * s * 4
    assert ops.beam_workspace(1, 7, 1, 33, 3) == 16 + 2 * 3 * 4                      # one level: no frontier, no states
    assert ops.beam_workspace(0, 5, 4, 33, 3) == 0 and ops.beam_workspace(3, 5, 33, 33, 3) == 0 and ops.beam_workspace(3, 2731, 4, 33, 3) == 0


def test_reach_keeps_its_default_planner():
    from srlz import deploy
    sig = inspect.signature(deploy.reach)
    assert list(sig.parameters)[:5] == ["encoder", "dynamics", "frames", "goal_frames", "horizon"]
    assert sig.parameters["planner"].default == "cem"
    assert sig.parameters["plan_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    d = inspect.signature(deploy.LatentDynamics.search).parameters
    assert [d[k].default for k in ("beam", "gamma", "keep_leaves", "goal", "goal_weight", "goal_mode")] == [64, 1.0, False, None, 1.0, "running"]
    assert deploy.Search.__slots__ == ("best_plan", "best_return", "action", "exact", "expanded", "leaves", "leaf_plans", "leaf_returns")
