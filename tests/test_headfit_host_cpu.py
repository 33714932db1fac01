"""The host side of the reward-head fit (srlz/headfit.py), the predicates of csrc/headfit.hip and the --fit-reward flags of
evaluation.predict_forward: nothing here needs a GPU."""
import numpy as np
import pytest
import torch

import headfit_util as hu
import reward_util as ru

NEW = ("srlz_headfit_supported", "srlz_headfit_n_params", "srlz_headfit_chunk_rows", "srlz_headfit_fit", "srlz_headfit_eval_workspace",
       "srlz_headfit_eval")


def _chunk_rows(S, H):
    """include/srlz.h, restated: the rows that fit beside parameters, gradient and Adam's table in 160 KB, at most 128, at least 16."""
    if not (1 <= S <= 512 and 1 <= H <= 32):
        return 0
    K, HPAD = 2 * S, ((H + 3) & ~3) | 4
    PL = (K + H + 4) * HPAD + 4
    room = 40956 - 2 * PL - 512
    r = room // ((K | 1) + 4 * HPAD + 7) if room >= 0 else 0
    return 0 if r < 16 else min(r, 128)


def test_abi_and_exported_names(cabi):
    assert cabi.ABI_VERSION == 104 and cabi.version() == 104
    for name in NEW:
        assert name in cabi.EXPORTED, name


def test_predicates_answer_on_the_host_and_follow_the_header():
    from srlz import ops, headfit
    for S in range(1, 201):
        for H in range(1, 17):
            assert ops.headfit_supported(S, H), (S, H)  # the reference head at every state dimension this project quotes
    for S, H in ((0, 16), (-1, 16), (3, 0), (3, -2), (513, 1), (1, 33), (512, 16), (512, 32), (342, 16), (202, 32)):
        assert not ops.headfit_supported(S, H), (S, H)
        assert ops.headfit_chunk_rows(S, H) == 0
    for S, H in ((512, 4), (489, 12), (341, 16), (256, 24), (201, 32), (1, 32), (1, 1)):
        assert ops.headfit_supported(S, H), (S, H)
    rs = np.random.RandomState(0)
    shapes = [(int(s), int(h)) for s, h in zip(rs.randint(-2, 520, 400), rs.randint(-2, 36, 400))]
    for S, H in shapes + [(S, H) for S in (1, 3, 200, 341, 342, 512) for H in (1, 4, 5, 12, 13, 16, 17, 32)]:
        rows = ops.headfit_chunk_rows(S, H)
        assert rows == _chunk_rows(S, H), (S, H)
        assert (rows == 0) == (not ops.headfit_supported(S, H))
        assert headfit.fit_route_for(S, H) == ("kernel" if ops.headfit_supported(S, H) else "torch")
        if S >= 1 and H >= 1:
            assert ops.headfit_n_params(S, H) == 2 * S * H + H + H * H + H + 2 * H + 2 == hu.n_params(S, H)
    assert ops.headfit_n_params(0, 4) == 0 and ops.headfit_n_params(4, 0) == 0
    assert ops.headfit_chunk_rows(3, 16) == 128 and ops.headfit_chunk_rows(200, 16) == 48


def test_eval_workspace_is_a_function_of_the_rows(cabi):
    assert cabi.headfit_eval_workspace(1, 1) == 8 and cabi.headfit_eval_workspace(2, 64) == 16 and cabi.headfit_eval_workspace(3, 43) == 24
    assert cabi.headfit_eval_workspace(0, 8) == 0 and cabi.headfit_eval_workspace(8, 0) == 0
    assert cabi.headfit_eval_workspace(1 << 16, 1 << 15) == 0


def test_wrappers_refuse_to_run_without_a_gpu():
    from srlz import ops, _cabi
    if torch.cuda.is_available():
        return  # (a machine with a GPU has nothing to refuse)
    with pytest.raises(_cabi.SrlzError):
        ops.reward_probe_data(np.zeros((4, 3), np.float32), np.zeros(4, np.int64))
    states, rewards, es, _ = hu.case_recording(hu.CASES[1])
    from srlz import headfit
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the learner's own refusal, as fit_forward raises it)
        headfit.fit_reward(states, rewards, es, epochs=1)


def _recording():
    return hu.case_recording(hu.CASES[1])[:3]


def test_every_value_error_is_raised_on_the_host():
    from srlz import headfit
    x, r, es = _recording()
    S, H = x.shape[1], 16
    ok = headfit.check_fit_reward(x, r, es)
    assert (ok["hidden"], ok["epochs"], ok["batch_size"], ok["lr"], ok["route"], ok["keep"]) == (16, 30, 32, 0.005, "kernel", "best")
    assert ok["init"].shape == (hu.n_params(S, H),) and ok["init"].dtype == np.float32 and ok["labels"].dtype == np.int32
    bad = x.copy()
    bad[5, 1] = np.nan
    init = headfit.initial_parameters(S, H, 0)
    short = dict(init)
    short["2.weight"] = torch.zeros(H, H + 1)
    lacking = {k: v for k, v in init.items() if k != "4.bias"}
    one_episode = np.zeros(len(es), bool)
    one_episode[0] = True
    for kw, match in ((dict(states=x[0]), "N,S"), (dict(states=x.astype(np.int32)), "floating"), (dict(states=bad), "finite"),
                      (dict(states=list(x)), "numpy array"), (dict(rewards=r[:-1]), "one entry per frame"),
                      (dict(episode_starts=es[:-1]), "one entry per frame"), (dict(rewards=np.where(np.arange(len(r)) == 7, 2.0, r)), "two classes"),
                      (dict(epochs=0), "at least 1"), (dict(batch_size=0), "at least 1"), (dict(hidden=0), "at least 1"),
                      (dict(lr=0.0), "lr"), (dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"),
                      (dict(init=short), "shape"), (dict(init=lacking), "lacks"),
                      (dict(keep="first"), "keep"), (dict(route="gram"), "route"),
                      (dict(route="kernel", hidden=40), "kernel"), (dict(starts=np.zeros(0, np.int64)), "no transition"),
                      (dict(val_starts=np.zeros(0, np.int64)), "no transition"), (dict(starts=np.array([len(r) - 1])), "starts must lie"),
                      (dict(val_starts=np.array([-1])), "val_starts must lie"), (dict(starts=np.array([0.5])), "integer"),
                      (dict(starts=np.array([1, 2, 3]), val_starts=np.array([3, 4])), "share 1 transitions"),
                      (dict(episode_starts=one_episode), "at least 2 episodes")):
        args = dict(states=x, rewards=r, episode_starts=es)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            headfit.fit_reward(**args)  # (raised before the GPU is asked for: this machine may have none)
    assert headfit.check_fit_reward(x, r, es, hidden=40)["route"] == "torch"  # a shape the kernel refuses takes the other route


def test_default_split_and_tables_follow_the_seed_alone():
    from srlz import headfit, dynfit
    x, r, es = _recording()
    a, b = headfit.check_fit_reward(x, r, es, seed=3), headfit.check_fit_reward(x, r, es, seed=3)
    tr, va = dynfit.split_episodes(es, 0.2, 3)
    assert np.array_equal(a["train"], tr) and np.array_equal(a["val"], va) and np.array_equal(a["train"], b["train"])
    t2, v2 = hu.split(es, 0.2, 3)  # the restatement the fixtures were recorded with
    assert np.array_equal(tr, t2) and np.array_equal(va, v2)
    assert not np.array_equal(headfit.check_fit_reward(x, r, es, seed=4)["val"], va)
    assert np.array_equal(a["init"], b["init"]) and not np.array_equal(a["init"], headfit.check_fit_reward(x, r, es, seed=4)["init"])
    starts = set(np.flatnonzero(es).tolist())
    for seed in (0, 3):
        tabs = headfit.minibatch_tables(tr, 4, 8, seed)
        again = headfit.minibatch_tables(tr, 4, 8, seed)
        ref = hu.train_tables(tr, 4, 8, seed)
        assert len(tabs) == 4
        for e, t in enumerate(tabs):
            assert t.dtype == np.int32 and t.shape == (len(tr) // 8, 8) and t.flags["C_CONTIGUOUS"]
            assert np.array_equal(t, again[e]) and np.array_equal(t, ref[e])
            assert np.array_equal(t.reshape(-1), np.random.RandomState(seed + e).permutation(tr)[:t.size])
            assert not (set((t.reshape(-1) + 1).tolist()) & starts) and t.max() <= len(es) - 2  # no pair crosses an episode boundary
            assert len(set(t.reshape(-1).tolist())) == t.size
        assert not np.array_equal(tabs[0], tabs[1])
    assert not np.array_equal(headfit.minibatch_tables(tr, 1, 8, 0)[0], headfit.minibatch_tables(tr, 1, 8, 1)[0])
    # fewer transitions than a batch: the batch shrinks to them
    few = headfit.minibatch_tables(tr[:5], 2, 8, 0)
    assert few[0].shape == (1, 5) and sorted(few[0][0].tolist()) == sorted(tr[:5].tolist())
    full, tail = headfit.validation_tables(va[::-1], 8)
    ref = hu.val_tables(va, 8)
    assert np.array_equal(full, ref[0]) and np.array_equal(np.concatenate((full.reshape(-1), tail.reshape(-1))), np.sort(va))
    assert tail.shape == (1, len(va) % 8) and np.array_equal(tail, ref[1])
    full, tail = headfit.validation_tables(va[:16], 8)
    assert full.shape == (2, 8) and tail is None
    full, tail = headfit.validation_tables(va[:3], 8)
    assert full.shape == (1, 3) and tail is None


def test_split_starts_cuts_a_list_of_transitions_by_whole_episodes():
    from srlz import headfit, dynfit
    x, r, es = _recording()
    tr, va = dynfit.split_episodes(es, 0.2, 0)
    ids = dynfit.episode_ids(es)
    a, b = headfit.split_starts(tr, es, 0.2, 0)
    assert a.dtype == np.int32 and np.array_equal(np.sort(np.concatenate((a, b))), tr) and not set(ids[a]) & set(ids[b])
    assert len(set(ids[b])) == 2 and len(set(ids[a])) == 6  # ceil(0.2 * 8) of the 8 training episodes
    assert np.array_equal(headfit.split_starts(tr[::-1], es, 0.2, 0)[1], b) and not np.array_equal(headfit.split_starts(tr, es, 0.2, 1)[1], b)
    with pytest.raises(ValueError, match="at least 2 episodes"):
        headfit.split_starts(tr[ids[tr] == ids[tr][0]], es)
    with pytest.raises(ValueError, match="val_fraction"):
        headfit.split_starts(tr, es, 1.0)
    # what check_fit_reward then takes: the two sides are disjoint
    cfg = headfit.check_fit_reward(x, r, es, starts=a, val_starts=b)
    assert np.array_equal(cfg["train"], a) and np.array_equal(cfg["val"], b)


def test_initial_parameters_are_the_head_own_and_leave_the_rng_alone():
    from srlz import headfit
    from models.forward_inverse import BaseRewardModel
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    init = headfit.initial_parameters(5, 7, 9)
    assert torch.equal(torch.random.get_rng_state(), before)
    torch.manual_seed(9)
    head = BaseRewardModel()
    head.initRewardNet(5, n_hidden=7)
    assert list(init) == list(hu.KEYS) == list(head.reward_net.state_dict())
    for k, v in head.reward_net.state_dict().items():
        assert torch.equal(init[k], v), k
    flat = headfit.flatten(init, 5, 7)
    assert flat.shape == (hu.n_params(5, 7),) and np.array_equal(flat, hu.flatten_state_dict(init).astype(np.float32))
    back = headfit.unflatten(flat, 5, 7)
    assert all(torch.equal(back[k], init[k]) for k in hu.KEYS)


def test_the_restatement_gradient_is_the_autograd_one():
    """tests/headfit_util.py against torch autograd in float64, at a width that is no multiple of 4."""
    S, H, B = 3, 5, 6
    rs = np.random.RandomState(1)
    flat = hu.random_params(S, H, 2).astype(np.float64)
    X, y = rs.randn(B, 2 * S), rs.randint(0, 2, B)
    loss, g, z = hu.loss_and_grad(flat, X, y, H)
    t = torch.tensor(flat, requires_grad=True)
    w1, b1, w2, b2, w3, b3 = [torch.reshape(p, s) for p, s in zip(torch.split(t, [int(np.prod(s)) for s in hu.shapes(S, H)]), hu.shapes(S, H))]
    f = torch.nn.functional
    zt = f.linear(f.relu(f.linear(f.relu(f.linear(torch.tensor(X), w1, b1)), w2, b2)), w3, b3)
    lt = f.cross_entropy(zt, torch.tensor(y))
    lt.backward()
    assert abs(loss - float(lt.detach())) < 1e-12 and np.abs(g - t.grad.numpy()).max() < 1e-12 and np.abs(z - zt.detach().numpy()).max() < 1e-12


def test_fit_reward_flags_parse_and_the_old_invocations_keep_their_defaults():
    from evaluation import predict_forward as pf
    a = pf.build_parser().parse_args(["--log-folder", "logs/ds/run/"])
    assert (a.log_folder, a.data_folder, a.input_file, a.horizon, a.training_set_size, a.no_cuda) == ("logs/ds/run/", "", "", 10, -1, False)
    assert a.fit is False and a.ground_truth is False and a.fit_reward is False
    assert (a.reward_epochs, a.reward_batch_size, a.reward_lr) == (None, None, None)
    a = pf.build_parser().parse_args(["--log-folder", "logs/ds/run", "--data-folder", "data/ds", "-i", "x.npz", "--horizon", "4",
                                      "--training-set-size", "100"])
    assert (a.data_folder, a.input_file, a.horizon, a.training_set_size, a.fit) == ("data/ds", "x.npz", 4, 100, False)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit"])
    assert a.fit is True and (a.ridge, a.val_fraction, a.seed, a.ground_truth) == (1e-6, 0.2, 0, False)
    assert a.fit_reward is False and (a.reward_epochs, a.reward_batch_size, a.reward_lr) == (None, None, None)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--ridge", "1e-3", "--val-fraction", "0.5", "--seed", "7", "--ground-truth"])
    assert (a.ridge, a.val_fraction, a.seed, a.ground_truth) == (1e-3, 0.5, 7, True)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--fit-reward"])
    assert a.fit_reward is True and (a.reward_epochs, a.reward_batch_size, a.reward_lr) == (30, 32, 0.005)
    assert (a.ridge, a.val_fraction, a.seed) == (1e-6, 0.2, 0)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--fit-reward", "--reward-epochs", "2", "--reward-batch-size", "8",
                                      "--reward-lr", "0.01"])
    assert (a.reward_epochs, a.reward_batch_size, a.reward_lr) == (2, 8, 0.01)
    with pytest.raises(SystemExit):
        pf.build_parser().parse_args(["--log-folder", "l", "--fit-reward"])
    for extra in (["--reward-epochs", "2"], ["--reward-batch-size", "8"], ["--reward-lr", "0.01"]):
        with pytest.raises(SystemExit):
            pf.build_parser().parse_args(["--log-folder", "l", "--fit"] + extra)
        with pytest.raises(SystemExit):
            pf.build_parser().parse_args(["--log-folder", "l"] + extra)
    for extra in (["--ground-truth"], ["--ridge", "1e-6"], ["--val-fraction", "0.2"], ["--seed", "0"]):
        with pytest.raises(SystemExit):
            pf.build_parser().parse_args(["--log-folder", "l"] + extra)
    with pytest.raises(SystemExit):
        pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--ground-truth", "-i", "x.npz"])
    assert pf.OUTPUT == "forward_horizon.json" and pf.OUTPUT_FIT == "forward_horizon_fit.json"
    assert pf.FIT_KEYS == ("ridge", "count", "val_fraction", "seed", "route", "state_dim", "n_actions")


def test_fixture_is_data_of_the_cases():
    fx, spread = hu.load_fixture(), hu.load_spread()
    assert spread["refused_above"] == 1e-3 and "float64 restatement" in spread["metric"]
    for case in hu.CASES:
        pre = case["name"] + "/"
        train, val, tables, vtabs = hu.case_tables(case)
        assert np.array_equal(fx[pre + "train"], train) and np.array_equal(fx[pre + "val"], val)
        assert np.array_equal(fx[pre + "tables"], np.stack(tables)) and np.array_equal(fx[pre + "eval_states/idx"], vtabs[0][0])
        assert fx[pre + "loss"].shape == (case["epochs"], 2) and fx[pre + "counts"].shape == (case["epochs"], 2, 5)
        for k, shp in zip(hu.KEYS, hu.shapes(case["S"], case["H"])):
            assert fx[pre + "init/" + k].shape == shp and fx[pre + "init/" + k].dtype == np.float32
        states, rewards, es, actions = hu.case_recording(case)
        assert states.shape == (300, case["S"]) and actions.max() == 5 and 0.1 < rewards.mean() < 0.3
        assert max(spread["cases"][case["name"]][k] for k in ("param", "eval_states", "loss")) <= 1e-3
