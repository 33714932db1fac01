"""Host side of the robotic priors (no GPU): the pair mining of losses/utils.py reproduces the unmodified reference index for index
(tests/golden/robotic_kats.npz, tools/make_golden_robotic.py), its in-place effects and quirks included; the exits; the incidence
table the backward kernel walks; and the float64 restatement the GPU tests compare with matches the reference's own function called
with double tensors."""
import contextlib
import io

import numpy as np
import pytest

import golden_util as gu
import robotic_util as ru


def _mine(rec, sort=True, fn="priors_pairs"):
    import losses.utils as lu
    actions, rewards, starts = ru.recording(rec)
    mlist = ru.minibatch_list(rec, starts, sort=sort)
    n_pairs = np.zeros(rec["A"], np.int64)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        dis, same = getattr(lu, fn)(rec["B"], mlist, actions, rewards, rec["A"], n_pairs)
    return mlist, dis, same, n_pairs, text.getvalue()


def _assert_equals_fixture(prefix, mlist, dis, same, n_pairs):
    g = gu.load("robotic_kats")
    np.testing.assert_array_equal(np.stack(mlist), g[prefix + "/minibatches"])
    np.testing.assert_array_equal(n_pairs, g[prefix + "/n_pairs_per_action"])
    for name, got in (("dis", dis), ("same", same)):
        ref = ru.split(g["%s/%s" % (prefix, name)], g["%s/%s_offsets" % (prefix, name)])
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert a.dtype == np.int64 and a.ndim == 2
            np.testing.assert_array_equal(a, b, err_msg="%s %s minibatch %d" % (prefix, name, k))


@pytest.mark.parametrize("rec", ru.RECORDINGS, ids=[r["name"] for r in ru.RECORDINGS])
@pytest.mark.parametrize("fn", ["priors_pairs", "findPriorsPairs"])
def test_pairs_match_reference(rec, fn):
    mlist, dis, same, n_pairs, text = _mine(rec, fn=fn)
    assert len(mlist) == ru.N_MINIBATCHES[rec["name"]]
    _assert_equals_fixture(rec["name"], mlist, dis, same, n_pairs)
    lines = text.splitlines()
    assert lines[0] == "Dealt with %d minibatches - dissimilar pairs" % ru.TOUCHED[rec["name"]]
    assert lines[1] == "Number of pairs per action:" and lines[2] == str(n_pairs)
    assert lines[3] == "Pairs of %d unique actions" % int((n_pairs > 0).sum())
    assert int(gu.load("robotic_kats")[rec["name"] + "/touched"]) == ru.TOUCHED[rec["name"]]


def test_over_sampling_quirk_is_kept():
    """The modified minibatch list differs from the learner's cut in exactly one frame per dealt-with minibatch; such a minibatch
    has ONE dissimilar pair, may be unsorted, and the pair may run backwards."""
    rec = ru.RECORDINGS[2]
    mlist, dis, same, _, _ = _mine(rec)
    before = ru.minibatch_list(rec, ru.recording(rec)[2])
    changed = [k for k in range(len(mlist)) if not np.array_equal(mlist[k], before[k])]
    assert len(changed) == ru.TOUCHED[rec["name"]]
    unsorted, backwards = 0, 0
    for k in changed:
        assert (mlist[k] != before[k]).sum() == 1 and dis[k].shape == (1, 2)
        i, j = dis[k][0]
        assert mlist[k][j] != before[k][j]
        unsorted += bool(np.any(np.diff(mlist[k]) < 0))
        backwards += bool(j < i)
    # (what the reference's run shows for this recording: four of the ten end unsorted, two of the single pairs run backwards)
    assert unsorted == 4 and backwards == 2


@pytest.mark.parametrize("rec", ru.RECORDINGS[:2], ids=[r["name"] for r in ru.RECORDINGS[:2]])
def test_pairs_from_unsorted_minibatches_match_reference(rec):
    mlist, dis, same, n_pairs, _ = _mine(rec, sort=False)
    _assert_equals_fixture(rec["name"] + "/unsorted", mlist, dis, same, n_pairs)


def _one_action_constant_reward(n=33, b=8):
    actions, rewards = np.zeros(n, np.int64), np.ones(n, np.int64)
    mlist = [np.arange(s, s + b) for s in range(0, n - 1 - b + 1, b)]
    return b, mlist, actions, rewards, 1, np.zeros(1, np.int64)


def test_no_pairs_exit_code():
    """One action with constant rewards: no dissimilar pair anywhere, and no minibatch can donate one.  The reference would scan for
    ever; here the intended exit is taken, with the reference's message."""
    import losses.utils as lu
    import pipeline
    assert pipeline.NO_PAIRS_ERROR == 10
    text = io.StringIO()
    with contextlib.redirect_stdout(text), pytest.raises(SystemExit) as e:
        lu.findPriorsPairs(*_one_action_constant_reward())
    assert e.value.code == 10
    assert "No same actions or dissimilar pairs found for at least one minibatch (currently is 8)" in text.getvalue()
    assert "=> Consider increasing the batch_size or changing the seed" in text.getvalue()


def test_no_donor_raises_instead_of_hanging():
    import losses.utils as lu
    assert issubclass(lu.NoPairsError, ValueError)
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(lu.NoPairsError, match="increasing the batch_size"):
        lu.priors_pairs(*_one_action_constant_reward())
    # overSampling under its own name takes the exit too
    b, mlist, actions, rewards, _, _ = _one_action_constant_reward()
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(SystemExit) as e:
        lu.overSampling(b, mlist, [np.array([], np.int64) for _ in mlist], lu.findDissimilar, actions, rewards)
    assert e.value.code == 10


def test_no_same_action_pair_raises():
    """Every row its own action: dissimilar pairs cannot exist either (they need the same action)."""
    import losses.utils as lu
    n, b = 9, 4
    actions, rewards = np.arange(n, dtype=np.int64) % 4, np.arange(n, dtype=np.int64) % 2
    mlist = [np.arange(0, 4), np.arange(4, 8)]
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(lu.NoPairsError):
        lu.priors_pairs(b, mlist, actions, rewards, 4, np.zeros(4, np.int64))


def test_find_functions():
    import losses.utils as lu
    actions = np.array([0, 1, 0, 0, 1, 0])
    rewards = np.array([0, 0, 1, 0, 1, 1, 0])
    m = np.array([0, 2, 3, 4])
    np.testing.assert_array_equal(lu.findSameActions(0, m, actions), [0, 1, 2])
    np.testing.assert_array_equal(lu.findSameActions(3, m, actions), [3])
    # row 0: action 0, reward rewards[1] = 0; rows 1, 2 (frames 2, 3) share the action, their rewards are rewards[3] = 0, rewards[4] = 1
    np.testing.assert_array_equal(lu.findDissimilar(0, m, m, actions, rewards), [2])
    np.testing.assert_array_equal(lu.findDissimilar(0, m, np.array([5, 1]), actions, rewards), [])


def test_incidence_table():
    from srlz import ops
    pairs = np.array([[0, 2], [3, 1], [0, 2], [2, 2], [1, 0]])  # a duplicate, an i > j and an i == j entry
    got = ops.robotic_incidence(pairs, 5)
    assert got.dtype == np.int32
    # offsets, then row 0: 2, 2, 1; row 1: 3, 0; row 2: 0, 0, 2, 2; row 3: 1; row 4: none
    np.testing.assert_array_equal(got, [0, 3, 5, 9, 10, 10, 2, 2, 1, 3, 0, 0, 0, 2, 2, 1])
    np.testing.assert_array_equal(got, ru.incidence_by_hand(pairs, 5))
    rs = np.random.RandomState(0)
    big = rs.randint(0, 37, (500, 2))
    np.testing.assert_array_equal(ops.robotic_incidence(big, 37), ru.incidence_by_hand(big, 37))


def test_pair_list_checks():
    from srlz import ops
    with pytest.raises(ValueError, match="empty"):
        ops.robotic_pairs(np.zeros((0, 2), np.int64), 4)
    with pytest.raises(ValueError, match="empty"):
        ops.robotic_pairs(np.array([], np.int64), 4)
    for bad in ([[0, 4]], [[-1, 2]]):
        with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
            ops.robotic_pairs(np.array(bad), 4)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        ops.robotic_pairs(np.array([0, 1, 2]), 4)
    with pytest.raises(ValueError, match="integers"):
        ops.robotic_pairs(np.array([[0.0, 1.0]]), 4)
    assert ops.ROBOTIC_TERMS == ("temp_coherence_loss", "causality_loss", "proportionality_loss", "repeatability_loss")


def _close(got, ref, what):
    scale = max(float(np.abs(ref).max()), 1e-300)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= 1e-12, "%s: %.3e" % (what, err)


@pytest.mark.parametrize("case", ru.LOSS_CASES, ids=[c["name"] for c in ru.LOSS_CASES])
def test_restatement_matches_reference(case):
    """The float64 restatement against the reference's function called with double tensors: 1e-12 of each tensor's scale (both are
    float64 sums of at most 32 640 terms in different orders)."""
    g = gu.load("robotic_kats")
    states, next_states, dis, same = ru.loss_case(case)
    for name, d, p in ru.variants(dis, same, case["seed"]):
        terms, ds, dns = ru.priors_f64(states, next_states, d, p)
        prefix = "loss/%s/%s/" % (case["name"], name)
        np.testing.assert_allclose(terms, g[prefix + "terms"], rtol=1e-12)
        _close(ds, g[prefix + "dstates"], prefix + "dstates")
        _close(dns, g[prefix + "dnext"], prefix + "dnext")


def test_restatement_zero_step_matches_reference():
    g = gu.load("robotic_kats")
    terms, ds, dns = ru.priors_f64(*ru.zero_step_case())
    assert np.isfinite(g["loss/zero_step/dstates"]).all() and np.isfinite(ds).all() and np.isfinite(dns).all()
    np.testing.assert_allclose(terms, g["loss/zero_step/terms"], rtol=1e-12)
    _close(ds, g["loss/zero_step/dstates"], "dstates")
    _close(dns, g["loss/zero_step/dnext"], "dnext")


def test_loss_case_conditioning():
    """What the GPU tests rely on: every step at least 1e-2 of the longest, every squared distance inside a pair at most 20."""
    for case in ru.LOSS_CASES:
        states, next_states, dis, same = ru.loss_case(case)
        s, step = states.astype(np.float64), next_states.astype(np.float64) - states.astype(np.float64)
        length = np.sqrt((step * step).sum(1))
        assert length.min() >= 1e-2 * length.max(), case["name"]
        for p in (dis, same):
            gap = s[p[:, 0]] - s[p[:, 1]]
            assert (gap * gap).sum(1).max() <= 20.0, case["name"]
        assert len(dis) >= 1 and len(same) >= 1
    assert len(ru.loss_case(ru.LOSS_CASES[-1])[3]) == 32640


# ---------------------------------------------------------------------------------------------------------------- the fit's host side
def _header_supported(D, S, B):
    """include/srlz.h, srlz_robotic_supported, restated."""
    if D < 1 or S < 1 or B < 1:
        return False
    spad = ((S + 3) & ~3) | 4
    return 2 * (D + 1) * spad + 512 + 4 * B * spad + ((B + 3) & ~3) + 32 <= 40960


def test_fit_route_agrees_with_the_header():
    from srlz import ops, priorsfit as pf
    for D, S, B in ((200, 8, 256), (768, 5, 256), (1, 1, 1), (200, 1, 32), (3, 3, 32), (32, 3, 256)):
        assert _header_supported(D, S, B) and pf.fit_route_for(D, S, B) == "kernel", (D, S, B)
    for D, S, B in ((0, 3, 32), (3, 0, 32), (3, 3, 0), (-1, 3, 32), (1 << 30, 3, 32), (3, 1 << 30, 32), (3, 3, 1 << 30)):
        assert not ops.robotic_supported(D, S, B) and pf.fit_route_for(D, S, B) == "torch"
    # the edges: the largest D at (S, B), the largest B at (D, S), and S across a change of its padding
    for S, B in ((3, 32), (8, 256), (5, 256), (1, 1), (13, 64)):
        d = 1
        while _header_supported(d + 1, S, B):
            d += 1
        assert ops.robotic_supported(d, S, B) and not ops.robotic_supported(d + 1, S, B), (d, S, B)
    assert ops.robotic_supported(4983, 3, 32) and not ops.robotic_supported(4984, 3, 32)
    for D, S in ((200, 8), (768, 5), (12, 3)):
        b = 1
        while _header_supported(D, S, b + 1):
            b += 1
        assert ops.robotic_supported(D, S, b) and not ops.robotic_supported(D, S, b + 1), (D, S, b)
    for S in range(1, 30):
        for B in (31, 32, 33):
            assert ops.robotic_supported(768, S, B) == _header_supported(768, S, B), (S, B)
    assert ops.robotic_n_params(12, 3) == 39 and ops.robotic_n_params(0, 3) == 0


def test_fit_tables_are_the_learners_cut():
    from srlz import priorsfit as pf
    for case in ru.FIT_CASES:
        rec = ru.RECORDINGS[case["rec"]]
        _, _, starts = ru.recording(rec)
        mlist, val_ids, orders = pf.minibatch_list(starts, rec["B"], case["seed"], case["val_size"], case["epochs"])
        ref = ru.fit_tables(rec, case["seed"], case["val_size"], case["epochs"])
        g = gu.load("robotic_kats")
        np.testing.assert_array_equal(np.stack(mlist), np.stack(ref[0]))
        np.testing.assert_array_equal(np.stack(mlist), g["fit/%s/minibatches" % case["name"]])
        np.testing.assert_array_equal(val_ids, g["fit/%s/val_ids" % case["name"]])
        np.testing.assert_array_equal(np.stack(orders), g["fit/%s/orders" % case["name"]])
        # the cut is the learner's: the stream of np.random.seed(seed) + np.random.shuffle
        np.testing.assert_array_equal(np.stack(mlist), np.stack(ru.minibatch_list(dict(rec, seed=case["seed"]), starts)))
        assert len(val_ids) == int(np.round(case["val_size"] * len(mlist))) == 3
        for o in orders:
            assert sorted(o.tolist() + val_ids.tolist()) == list(range(len(mlist)))
        assert any(not np.array_equal(orders[0], o) for o in orders[1:])


def test_initial_parameters_are_nn_linears():
    import torch
    from srlz import priorsfit as pf
    g = gu.load("robotic_kats")
    case = ru.FIT_CASES[0]
    torch.manual_seed(123)
    before = torch.rand(3)
    torch.manual_seed(123)
    w, b = pf.initial_parameters(case["D"], case["S"], case["seed"])
    assert torch.equal(torch.rand(3), before)  # (the caller's RNG state is untouched)
    np.testing.assert_array_equal(w, g["fit/%s/init_weight" % case["name"]])
    np.testing.assert_array_equal(b, g["fit/%s/init_bias" % case["name"]])


def test_check_fit_priors():
    from srlz import priorsfit as pf
    rec = ru.RECORDINGS[0]
    actions, rewards, starts = ru.recording(rec)
    x = ru.fit_features(ru.FIT_CASES[0])
    cfg = pf.check_fit_priors(x, actions, rewards, starts, 3, batch_size=16, epochs=2, seed=0)
    assert cfg["route"] == "kernel" and cfg["n_actions"] == rec["A"] and len(cfg["minibatches"]) == 14 and len(cfg["orders"]) == 2
    assert cfg["weight"].shape == (3, 12) and cfg["bias"].shape == (3,)

    def bad(match, **kw):
        args = dict(features=x, actions=actions, rewards=rewards, episode_starts=starts, state_dim=3, batch_size=16)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            pf.check_fit_priors(**args)
    nan = x.copy()
    nan[5, 2] = np.nan
    bad("finite", features=nan)
    inf = x.copy()
    inf[0, 0] = np.inf
    bad("finite", features=inf)
    bad("floating point", features=x.astype(np.int32))
    bad("one entry per frame", actions=actions[:-1])
    bad("one entry per frame", rewards=rewards[:-1])
    bad("one entry per frame", episode_starts=starts[:-1])
    bad("state_dim", state_dim=0)
    bad("larger than", batch_size=235)
    bad("at least 1", batch_size=0)
    bad("at least 1", epochs=0)
    bad("lr", lr=0.0)
    bad("lr", lr=float("nan"))
    bad("keep", keep="first")
    bad("route", route="cpu")
    bad("actions must lie", n_actions=2)
    bad("holds out", val_size=0.0)
    bad("init must be", init=(np.zeros((3, 11), np.float32), np.zeros(3, np.float32)))
    bad("holds out", batch_size=234)  # (all 234 transitions in one minibatch: none can be held out)
