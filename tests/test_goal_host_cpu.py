"""Goal-distance scores on the host side (no GPU): the new symbols in header, library and binding; the limits of the *_goal_supported
predicates and the LDS budget at them; check_goal and the weight / mode validation; the route tables (a split model on "model", a
forward-inverse model on the kernel); goal_scores in numpy and torch against the restatement of goal_util and against the fixture of
the unmodified reference (tests/golden/goal_kats.npz) within the recorded bound; and the host planner on the integer world."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import dynamics_util as dy
import goal_util as gu
from test_dynamics_host_cpu import _modules, _split

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW = ("srlz_rollout_goal_supported", "srlz_rollout_goal", "srlz_plan_goal_supported", "srlz_plan_goal_workspace", "srlz_plan_cem_goal")


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
    # the goal calls take their neighbours' arguments, in their order, then the goal's
    for base, goal, extra in (("srlz_rollout", "srlz_rollout_goal", 5), ("srlz_plan_cem", "srlz_plan_cem_goal", 4)):
        b, g = cabi._PROTOS[base][1], cabi._PROTOS[goal][1]
        assert len(g) == len(b) + extra and list(g[:len(b) - 1]) == list(b[:-1]) and g[-1] is b[-1], goal  # (the stream stays last)


def test_supported_at_each_limit_and_one_past_it(cabi):
    from srlz import ops
    ro, pl = cabi.rollout_goal_supported, cabi.plan_goal_supported
    for s, a, h in ((1, 1, 1), (200, 6, 16), (512, 65536, 32), (33, 6, 32)):
        assert ro(s, a, h, 2, 1) == 1 and ro(s, a, 0, 0, 0) == 1 and ro(s, a, 77, 5, 0) == 1, (s, a, h)  # no head: H, n_rewards not looked at
    for s, a, h, nr in ((513, 6, 16, 2), (0, 6, 16, 2), (200, 0, 16, 2), (200, 65537, 16, 2), (200, 6, 33, 2), (200, 6, 0, 2), (200, 6, 16, 3)):
        assert ro(s, a, h, nr, 1) == 0, (s, a, h, nr)
    assert ro(513, 6, 16, 2, 0) == 0 and ro(200, 0, 16, 2, 0) == 0
    for s, a, h, k, t in ((1, 1, 1, 1, 1), (200, 6, 16, 64, 10), (512, 256, 32, 1024, 32), (3, 256, 16, 1, 32), (3, 6, 16, 1024, 1)):
        assert pl(s, a, h, 2, 1, k, t) == 1 and pl(s, a, 0, 0, 0, k, t) == 1, (s, a, h, k, t)
    for s, a, h, nr, k, t in ((513, 6, 16, 2, 64, 10), (200, 257, 16, 2, 64, 10), (200, 6, 33, 2, 64, 10), (200, 6, 16, 3, 64, 10),
                              (200, 6, 16, 2, 1025, 10), (200, 6, 16, 2, 0, 10), (200, 6, 16, 2, 64, 33), (200, 6, 16, 2, 64, 0)):
        assert pl(s, a, h, nr, 1, k, t) == 0, (s, a, h, nr, k, t)
    assert pl(200, 257, 0, 0, 0, 64, 10) == 0 and pl(200, 6, 0, 0, 0, 1025, 10) == 0
    assert ops.rollout_goal_supported(200, 6, 16, 2, True) and ops.rollout_goal_supported(200, 6, 0, 0, has_reward=False)
    assert ops.plan_goal_supported(200, 6, 16, 2, True, 64, 10) and not ops.plan_goal_supported(200, 6, 16, 2, True, 64, 33)
    # the workspace is the planner's own
    for args in ((3, 33, 5, True), (3, 33, 5, False), (0, 33, 5, False), (3, 1025, 5, False), (3, 33, 33, False)):
        assert ops.plan_goal_workspace(*args) == ops.plan_workspace(*args), args
    # the budget DESIGN.md 3.17 states: the goal's partials add 16 * 33 floats; at the limits everything stays inside 160 KB of LDS
    tile = (512 * 33 + 8 * 32 * 33 + 2 * 32 * 33 + 32 * 32 + 4 * 32 + 4 + 2 * 32) * 4
    goal = 16 * 33 * 4
    assert tile == 114704 and tile + goal <= 160 * 1024
    assert tile + goal + (32 * 256 + 2 * 1024) * 4 + 16 <= 160 * 1024


def test_check_goal_weight_and_mode():
    from srlz import deploy
    assert deploy.check_goal(np.zeros(8, np.float32), 3, 8) is True
    assert deploy.check_goal(np.zeros((3, 8), np.float64), 3, 8) is False
    assert deploy.check_goal(torch.zeros(8), 1, 8) is True and deploy.check_goal(torch.zeros((1, 8), dtype=torch.float16), 1, 8) is False
    for bad, match in ((np.zeros(8, np.int64), "floating point"), (np.zeros(7, np.float32), "wide"), (np.zeros((2, 8), np.float32), "environments"),
                       (np.zeros((3, 7), np.float32), "wide"), (np.zeros((1, 3, 8), np.float32), "shape"), (np.zeros((), np.float32), "shape"),
                       ([0.0] * 8, "numpy array or a torch tensor"), (None, "numpy array or a torch tensor")):
        with pytest.raises(ValueError, match=match):
            deploy.check_goal(bad, 3, 8)
    assert deploy.check_goal_args(1, "running") == (1.0, "running") and deploy.check_goal_args(np.float32(0.5), "final") == (0.5, "final")
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-46, True, "1", None):  # (1e39 / 1e-46: not finite / not > 0 as the kernel's float)
        with pytest.raises(ValueError, match="goal_weight"):
            deploy.check_goal_args(bad, "running")
    for bad in ("Running", "last", 0, None):
        with pytest.raises(ValueError, match="goal_mode"):
            deploy.check_goal_args(1.0, bad)


def test_route_tables():
    from srlz import deploy
    both, fwd_only = _modules(8, ["forward", "reward"]), _modules(8, ["forward", "inverse"])
    for m in (both, fwd_only):
        for goal_only in (False, True):
            assert deploy.goal_route_for(m, goal_only) == "rollout"
            assert deploy.plan_goal_route_for(m, goal_only, 64, 10) == "rollout"
            assert deploy.plan_goal_route_for(m, goal_only, 1024, 32) == "rollout"
            assert deploy.plan_goal_route_for(m, goal_only, 1025, 10) == "model"
            assert deploy.plan_goal_route_for(m, goal_only, 64, 33) == "model"
            assert deploy.plan_goal_route_for(m, goal_only, 64, 10, n_envs=129) == "model"
            assert deploy.plan_goal_route_for(m, goal_only, 64, 10, n_envs=129, max_rows=16384) == "rollout"
    for goal_only in (False, True):  # every split model: its heads see masked states
        assert deploy.goal_route_for(_split(), goal_only) == "model" and deploy.plan_goal_route_for(_split(), goal_only, 64, 10) == "model"
        assert deploy.goal_route_for(_modules(513, ["forward", "reward"]), goal_only) == "model"
    # the tables without a goal keep their answers
    assert deploy.dynamics_route_for(both) == "rollout" and deploy.plan_route_for(both, 64, 10) == "rollout"
    assert deploy.dynamics_route_for(_split()) == "model" and deploy.plan_route_for(both, 64, 33) == "model"


def _fixture():
    return np.load(os.path.join(GOLDEN, "goal_kats.npz")), json.load(open(os.path.join(GOLDEN, "goal_spread.json")))


def test_fixture_records_its_condition():
    kats, spread = _fixture()
    assert spread["kstar"] == gu.KSTAR == int(kats["kstar"]) and spread["gamma"] == gu.GAMMA and spread["weight"] == gu.WEIGHT
    assert spread["act_weight"] == gu.ACT_WEIGHT
    for name in dy.CASES:
        sp = spread["cases"][name]
        last = kats[name + "/goal_dist64"][:, :, -1]
        assert (last.argmin(axis=1) == gu.KSTAR).all() and (kats[name + "/act_score64"].argmax(axis=1) == gu.KSTAR).all(), name
        assert sp["final_margin"] > 0 and sp["act_margin"] > 0
        # in every case the margin exceeds twice the bound: an answer within the bound cannot change the argmin
        assert sp["final_margin_exceeds_bound"] is True and sp["final_margin"] > 2 * dy.bound(sp["goal_dist"]), name
        assert sp["act_margin_exceeds_bound"] is True and sp["act_margin"] > 2 * dy.bound(sp["act_score"]), name
        assert kats[name + "/goal"].dtype == np.float32 and kats[name + "/goal"].shape == (dy.N_ENVS, dy.CASES[name]["state_dim"])
    pl = gu.case_inputs("s8_mlp")[1]
    for n in range(dy.N_ENVS):  # the fixture's plans are pairwise different in every environment
        assert len({tuple(row) for row in pl[n]}) == dy.N_PLANS


@pytest.mark.parametrize("name", list(dy.CASES))
def test_goal_scores_against_the_reference_fixture(name):
    """goal_scores on this build's own seeded model rolled in torch fp32 on the CPU, in numpy and in torch, against the fp64 figures of
    the unmodified reference, within max(1e-4, 10 x the reference's own fp32-to-fp64 spread)."""
    from srlz import deploy
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    kats, spread = _fixture()
    sp = spread["cases"][name]
    model = dy.build_case(name, modules)
    z, plans = gu.case_inputs(name)
    own = dy.restate(dy.head_params(model.state_dict()), z, plans, gu.GAMMA, torch.float32)
    goal = kats[name + "/goal"]
    probs = gu.probs(own["reward_logits"], np.float32)
    for as_torch in (False, True):
        tr = torch.from_numpy(own["trajectory"]) if as_torch else own["trajectory"]
        pr = torch.from_numpy(probs) if as_torch else probs
        for key in gu.SCORE_KEYS:
            mode, head = key.split("_")
            score, dist = deploy.goal_scores(tr, torch.from_numpy(goal) if as_torch else goal, pr if head == "head" else None, gu.GAMMA,
                                             gu.WEIGHT, mode)
            score, dist = np.asarray(score), np.asarray(dist)
            assert score.dtype == np.float32 and score.shape == (dy.N_ENVS, dy.N_PLANS) and dist.shape == (dy.N_ENVS, dy.N_PLANS, dy.HORIZON)
            e_dist = dy.rel_err(dist[..., None], kats[name + "/goal_dist64"][..., None], True)
            e_score = dy.rel_err(score, kats["%s/%s64" % (name, key)], False)
            print("%s %s torch=%s: goal_dist %.2e (bound %.2e), score %.2e (bound %.2e)"
                  % (name, key, as_torch, e_dist, dy.bound(sp["goal_dist"]), e_score, dy.bound(sp[key])))
            assert e_dist <= dy.bound(sp["goal_dist"]) and e_score <= dy.bound(sp[key]), (key, e_dist, e_score)
    # a shared goal [S] is the same goal tiled, and fp64 in gives fp64 out
    shared = deploy.goal_scores(own["trajectory"], goal[1], probs, gu.GAMMA, gu.WEIGHT, "running")
    tiled = deploy.goal_scores(own["trajectory"], np.tile(goal[1], (dy.N_ENVS, 1)), probs, gu.GAMMA, gu.WEIGHT, "running")
    assert np.array_equal(shared[0], tiled[0]) and np.array_equal(shared[1], tiled[1])
    assert deploy.goal_scores(own["trajectory"].astype(np.float64), goal, None)[0].dtype == np.float64


def test_goal_scores_is_the_restatement_where_both_are_exact():
    """On the integer world every operation is exact in fp32: goal_scores, the restatement of goal_util and the known answers agree
    bit for bit, in both modes, with gamma = 1 and with a gamma whose powers round."""
    from srlz import deploy
    rng = np.random.RandomState(0)
    plans = rng.randint(0, 4, size=(3, 17, 4))
    plans[1, 5] = 0
    tr = gu.world_trajectory(plans)
    for mode, want in (("running", -14.0), ("final", 0.0)):
        for as_torch in (False, True):
            score, dist = deploy.goal_scores(torch.from_numpy(tr) if as_torch else tr, gu.WORLD_GOAL, None, 1.0, 1.0, mode)
            score, dist = np.asarray(score), np.asarray(dist)
            assert np.array_equal(score, gu.world_scores(plans, mode)) and float(score[1, 5]) == want
            assert np.array_equal(dist[1, 5], [9, 4, 1, 0]) and np.array_equal(dist, gu.dist(tr, gu.WORLD_GOAL, np.float32))
        got = np.asarray(deploy.goal_scores(tr, gu.WORLD_GOAL, None, 0.9, 0.5, mode)[0])
        assert np.array_equal(got.view(np.uint32), gu.world_scores(plans, mode, 0.9, 0.5).view(np.uint32))
    # with probabilities: term_t = p_t - w c_t
    p = rng.rand(3, 17, 4).astype(np.float32)
    for mode in gu.MODES:
        got = np.asarray(deploy.goal_scores(tr, gu.WORLD_GOAL, p, 0.9, 0.5, mode)[0])
        ref = gu.scores(gu.dist(tr, gu.WORLD_GOAL, np.float32), p, 0.9, 0.5, mode, np.float32)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), mode


@pytest.mark.parametrize("mode,want", [("running", -14.0), ("final", 0.0)])
def test_host_planner_finds_the_way_in_the_integer_world(mode, want):
    from srlz import deploy
    w, n = gu.WORLD, 2

    def scorer(pl):
        return deploy.goal_scores(gu.world_trajectory(pl), gu.WORLD_GOAL, None, 1.0, 1.0, mode)[0]
    out = deploy.cem_host(scorer, n, w["k"], w["t"], w["a"], w["iterations"], w["elites"], w["q"], w["seed"], keep_population=True)
    assert not out["best_plan"].any() and (out["best_return"] == want).all(), (out["best_plan"], out["best_return"])
    assert out["best_return"].dtype == np.float32 and (np.diff(out["history"], axis=0) >= 0).all()
    assert (out["returns"] <= want).all()  # nothing scores above the way itself
    import plan_util as pu
    ref = pu.cem(lambda pl: gu.world_scores(pl, mode), n, w["k"], w["t"], w["a"], w["iterations"], w["elites"], w["q"], w["seed"])
    for q in ("plans", "returns", "cum", "best_plan", "best_return"):
        assert np.array_equal(out[q], ref[q]), q
