"""The host side of the inverse-head fit (srlz/invfit.py), the predicates of csrc/invfit.hip and the --fit-inverse flags of
evaluation.predict_forward: nothing here needs a GPU."""
import os

import numpy as np
import pytest
import torch

import headfit_util as hu
import invfit_util as iu

NEW = ("srlz_invfit_supported", "srlz_invfit_n_params", "srlz_invfit_chunk_rows", "srlz_invfit_fit", "srlz_invfit_eval_workspace",
       "srlz_invfit_eval")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_names(cabi):
    for name in NEW:
        assert name in cabi.EXPORTED, name


def test_predicate_on_both_sides_of_its_edge_follows_the_header():
    from srlz import ops, invfit
    assert ops.invfit_supported(200, 6) and ops.invfit_chunk_rows(200, 6) == 74 == iu.chunk_rows(200, 6)
    assert ops.invfit_chunk_rows(3, 6) == 128
    # the edge in S at A = 6 and A = 16, and in A at S = 1: the last shape inside keeps a chunk of at least 16 rows
    for A, s_max in ((6, 501), (16, 356), (4, 839)):
        assert ops.invfit_supported(s_max, A) and ops.invfit_chunk_rows(s_max, A) >= 16, (A, s_max)
        assert not ops.invfit_supported(s_max + 1, A) and ops.invfit_chunk_rows(s_max + 1, A) == 0
    assert ops.invfit_supported(1, 1676) and ops.invfit_chunk_rows(1, 1676) == 16 and not ops.invfit_supported(1, 1677)
    for S, A in ((0, 6), (-1, 6), (3, 1), (3, 0), (3, -2), (1 << 20, 6), (3, 1 << 20), (1 << 30, 1 << 30)):
        assert not ops.invfit_supported(S, A) and ops.invfit_chunk_rows(S, A) == 0, (S, A)
    rs = np.random.RandomState(0)
    shapes = [(int(s), int(a)) for s, a in zip(rs.randint(-2, 900, 400), rs.randint(-2, 40, 400))]
    shapes += [(1, int(a)) for a in rs.randint(2, 2000, 100)]
    for S, A in shapes + [(S, A) for S in (1, 3, 200, 356, 357, 501, 502) for A in (2, 4, 5, 6, 8, 9, 16, 17)]:
        rows = ops.invfit_chunk_rows(S, A)
        assert rows == iu.chunk_rows(S, A), (S, A)
        assert (rows == 0) == (not ops.invfit_supported(S, A))
        if S >= 1 and A >= 2:
            assert invfit.fit_route_for(S, A) == ("kernel" if rows else "torch")
            assert ops.invfit_n_params(S, A) == 2 * S * A + A == iu.n_params(S, A)
    assert ops.invfit_n_params(0, 4) == 0 and ops.invfit_n_params(4, 1) == 0
    assert ops.INVFIT_COUNTS == ("rows", "correct", "bad") and ops.invfit_n_counts(6) == 15


def test_fit_route_for_linear_in_mlp_and_over_size_to_torch():
    from srlz import invfit
    assert invfit.fit_route_for(200, 6) == "kernel" and invfit.fit_route_for(200, 6, "linear") == "kernel"
    assert invfit.fit_route_for(200, 6, "mlp") == "torch" and invfit.fit_route_for(3, 6, "mlp") == "torch"
    assert invfit.fit_route_for(502, 6) == "torch" and invfit.fit_route_for(2000, 6) == "torch"
    with pytest.raises(ValueError, match="inverse_model_type"):
        invfit.fit_route_for(3, 6, "resnet")


def test_eval_workspace_is_a_function_of_the_rows(cabi):
    assert cabi.invfit_eval_workspace(1, 1) == 8 and cabi.invfit_eval_workspace(2, 64) == 16 and cabi.invfit_eval_workspace(3, 43) == 24
    assert cabi.invfit_eval_workspace(0, 8) == 0 and cabi.invfit_eval_workspace(8, 0) == 0
    assert cabi.invfit_eval_workspace(1 << 16, 1 << 15) == 0


def _recording():
    return iu.case_recording(iu.CASES[0])


def test_tables_and_split_equal_the_fixture():
    from srlz import invfit, headfit, dynfit
    assert invfit.minibatch_tables is headfit.minibatch_tables and invfit.validation_tables is headfit.validation_tables
    assert invfit.split_starts is headfit.split_starts  # imported, not copied
    fx = iu.load_fixture()
    for case in iu.CASES:
        pre = case["name"] + "/"
        x, a, es = iu.case_recording(case)
        cfg = invfit.check_fit_inverse(x, a, es, seed=case["seed"], epochs=case["epochs"], batch_size=case["bs"], lr=case["lr"])
        assert np.array_equal(cfg["train"], fx[pre + "train"]) and np.array_equal(cfg["val"], fx[pre + "val"])
        assert cfg["n_actions"] == case["A"] and cfg["route"] == "kernel"
        tables = invfit.minibatch_tables(cfg["train"], case["epochs"], case["bs"], case["seed"])
        assert np.array_equal(np.stack(tables), fx[pre + "tables"])
        full, tail = invfit.validation_tables(cfg["val"], case["bs"])
        assert np.array_equal(full[0], fx[pre + "eval_states/idx"])
        # no pair crosses an episode boundary: the transitions are dynfit.transitions
        assert np.array_equal(np.sort(np.concatenate((cfg["train"], cfg["val"]))), dynfit.transitions(es))
        assert not set((np.stack(tables).reshape(-1) + 1).tolist()) & set(np.flatnonzero(es).tolist())
        # the label of transition i is actions[i]
        used = np.concatenate((cfg["train"], cfg["val"]))
        assert np.array_equal(cfg["labels"][used], a[used]) and cfg["labels"].dtype == np.int32


def test_initial_parameters_leave_the_rng_alone_and_equal_the_fixture():
    from srlz import invfit
    from models.forward_inverse import BaseInverseModel
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    init = invfit.initial_parameters(5, 7, 9)
    assert torch.equal(torch.random.get_rng_state(), before)
    torch.manual_seed(9)
    head = BaseInverseModel()
    head.initInverseNet(5, 7)
    assert list(init) == list(iu.KEYS) == list(head.inverse_net.state_dict())
    for k, v in head.inverse_net.state_dict().items():
        assert torch.equal(init[k], v), k
    flat = invfit.flatten(init, 5, 7)
    assert flat.shape == (iu.n_params(5, 7),) and np.array_equal(flat, iu.flatten_state_dict(init).astype(np.float32))
    back = invfit.unflatten(flat, 5, 7)
    assert all(torch.equal(back[k], init[k]) for k in iu.KEYS)
    fx = iu.load_fixture()
    for case in iu.CASES:
        mine = invfit.initial_parameters(case["S"], case["A"], case["seed"])
        for k in iu.KEYS:
            assert np.array_equal(mine[k].numpy(), fx[case["name"] + "/init/" + k]), (case["name"], k)
    mlp = invfit.initial_parameters(3, 6, 0, "mlp")
    assert list(mlp) == list(invfit.KEYS["mlp"]) and tuple(mlp["0.weight"].shape) == (128, 6) and tuple(mlp["4.weight"].shape) == (6, 128)
    assert invfit.flatten(mlp, 3, 6, "mlp").size == 128 * 6 + 128 + 128 * 128 + 128 + 6 * 128 + 6


def test_every_value_error_is_raised_on_the_host():
    from srlz import invfit
    x, a, es = _recording()
    S, A = x.shape[1], 6
    ok = invfit.check_fit_inverse(x, a, es)
    assert (ok["n_actions"], ok["epochs"], ok["batch_size"], ok["lr"], ok["route"], ok["keep"]) == (6, 30, 32, 0.005, "kernel", "best")
    assert ok["init"].shape == (iu.n_params(S, A),) and ok["init"].dtype == np.float32
    bad = x.copy()
    bad[5, 1] = np.nan
    init = invfit.initial_parameters(S, A, 0)
    short = dict(init)
    short["weight"] = torch.zeros(A, 2 * S + 1)
    lacking = {k: v for k, v in init.items() if k != "bias"}
    one_episode = np.zeros(len(es), bool)
    one_episode[0] = True
    out_of_range = a.copy()
    out_of_range[7] = 6
    negative = a.copy()
    negative[7] = -1
    for kw, match in ((dict(states=x[0]), "N,S"), (dict(states=x.astype(np.int32)), "floating"), (dict(states=bad), "finite"),
                      (dict(states=list(x)), "numpy array"), (dict(actions=a[:-1]), "one entry per frame"),
                      (dict(episode_starts=es[:-1]), "one entry per frame"), (dict(actions=a + 0.5), "integers"),
                      (dict(n_actions=1), "at least 2"), (dict(n_actions=0), "at least 2"), (dict(actions=np.zeros_like(a)), "at least 2"),
                      (dict(actions=out_of_range, n_actions=6), r"\[0, 6\)"), (dict(actions=negative), r"\[0, 6\)"),
                      (dict(n_actions=5), r"\[0, 5\)"),
                      (dict(epochs=0), "at least 1"), (dict(batch_size=0), "at least 1"),
                      (dict(lr=0.0), "lr"), (dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"),
                      (dict(init=short), "shape"), (dict(init=lacking), "lacks"),
                      (dict(keep="first"), "keep"), (dict(route="gram"), "route"), (dict(inverse_model_type="resnet"), "inverse_model_type"),
                      (dict(route="kernel", inverse_model_type="mlp"), "kernel"),
                      (dict(starts=np.zeros(0, np.int64)), "no transition"),
                      (dict(val_starts=np.zeros(0, np.int64)), "no transition"), (dict(starts=np.array([len(a) - 1])), "starts must lie"),
                      (dict(val_starts=np.array([-1])), "val_starts must lie"), (dict(starts=np.array([0.5])), "integer"),
                      (dict(starts=np.array([1, 2, 3]), val_starts=np.array([3, 4])), "share 1 transitions"),
                      (dict(val_fraction=1.0), "val_fraction"), (dict(episode_starts=one_episode), "at least 2 episodes")):
        args = dict(states=x, actions=a, episode_starts=es)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            invfit.fit_inverse(**args)  # (raised before the GPU is asked for: this machine may have none)
    wide = np.zeros((len(a), 502), np.float32)
    assert invfit.check_fit_inverse(wide, a, es)["route"] == "torch"  # a shape the kernel refuses takes the other route
    with pytest.raises(ValueError, match="kernel"):
        invfit.check_fit_inverse(wide, a, es, route="kernel")
    assert invfit.check_fit_inverse(x, a, es, inverse_model_type="mlp")["route"] == "torch"
    # an action outside the range on a frame no transition starts at is never read, and does not count
    last = a.copy()
    last[np.flatnonzero(es)[1] - 1] = 99  # the last frame of the first episode
    assert invfit.check_fit_inverse(x, last, es)["n_actions"] == 6


def test_inverse_fit_without_meaning_is_refused_before_any_gpu_work():
    from srlz.deploy import LatentDynamics
    x, a, es = _recording()
    for bad in (True, "best", 30, []):
        with pytest.raises(ValueError, match="inverse_fit must be None or a dict"):
            LatentDynamics.from_recording(x, a, es, inverse_fit=bad)


def test_fit_inverse_flags_parse_and_the_old_invocations_keep_their_defaults():
    from evaluation import predict_forward as pf
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit"])
    assert a.fit_inverse is False and (a.inverse_epochs, a.inverse_batch_size, a.inverse_lr) == (None, None, None)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--fit-inverse"])
    assert a.fit_inverse is True and (a.inverse_epochs, a.inverse_batch_size, a.inverse_lr) == (30, 32, 0.005)
    assert a.fit_reward is False and (a.reward_epochs, a.reward_batch_size, a.reward_lr) == (None, None, None)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--fit-inverse", "--inverse-epochs", "2", "--inverse-batch-size", "8",
                                      "--inverse-lr", "0.01", "--fit-reward"])
    assert (a.inverse_epochs, a.inverse_batch_size, a.inverse_lr, a.reward_epochs) == (2, 8, 0.01, 30)
    with pytest.raises(SystemExit):
        pf.build_parser().parse_args(["--log-folder", "l", "--fit-inverse"])  # --fit-inverse without --fit
    for extra in (["--inverse-epochs", "2"], ["--inverse-batch-size", "8"], ["--inverse-lr", "0.01"]):
        with pytest.raises(SystemExit):
            pf.build_parser().parse_args(["--log-folder", "l", "--fit"] + extra)
        with pytest.raises(SystemExit):
            pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--fit-reward"] + extra)
    assert pf.INVERSE_KEYS[:6] == ("accuracy", "majority_accuracy", "recall", "count", "best_epoch", "route")


def test_header_cites_the_reference_lines_and_states_the_formula():
    with open(os.path.join(REPO, "include", "srlz.h")) as f:
        text = f.read()
    section = text[text.index("The inverse head fitted on a recording"):text.index("int srlz_invfit_supported")]
    for cite in ("models/forward_inverse.py inverseModel", "losses/losses.py:117-129", "the learner's Adam loop"):
        assert cite in section, cite
    assert "min(128, floor((40444 - 2 * (K + 2) * APAD) / ((K | 1) + APAD + 3)))" in section
    assert "GLOBAL memory" in section  # where the Adam moments live
    for name in NEW:
        assert name + "(" in text, name


def test_the_restatement_gradient_is_the_autograd_one():
    """tests/invfit_util.py against torch autograd in float64, at a class count that is no multiple of 4; a row with a label out of
    range adds nothing."""
    S, A, B = 3, 5, 6
    rs = np.random.RandomState(1)
    flat = iu.random_params(S, A, 2).astype(np.float64)
    X, y = rs.randn(B, 2 * S), rs.randint(0, A, B)
    loss, g, z = iu.loss_and_grad(flat, X, y, A)
    t = torch.tensor(flat, requires_grad=True)
    zt = torch.nn.functional.linear(torch.tensor(X), t[:2 * S * A].reshape(A, 2 * S), t[2 * S * A:])
    lt = torch.nn.functional.cross_entropy(zt, torch.tensor(y))
    lt.backward()
    assert abs(loss - float(lt.detach())) < 1e-12 and np.abs(g - t.grad.numpy()).max() < 1e-12 and np.abs(z - zt.detach().numpy()).max() < 1e-12
    y_bad = y.copy()
    y_bad[2] = A
    keep = np.arange(B) != 2
    l2, g2, _ = iu.loss_and_grad(flat, X, y_bad, A)
    l3, g3, _ = iu.loss_and_grad(flat, X[keep], y[keep], A)
    assert abs(l2 * B - l3 * (B - 1)) < 1e-12 and np.abs(g2 * B - g3 * (B - 1)).max() < 1e-12
    c = iu.count(z, y_bad)
    assert c[0] == B and c[2] == 1 and c[3:3 + A].sum() == B - 1 and c[3 + A:].sum() == c[1]


def test_fixture_is_data_of_the_cases():
    fx, spread = iu.load_fixture(), iu.load_spread()
    assert spread["refused_above"] == 1e-3 and "float64 restatement" in spread["metric"]
    assert [(c["S"], c["A"], c["epochs"], c["bs"]) for c in iu.CASES] == [(3, 6, 5, 8), (12, 4, 5, 8)]
    for case in iu.CASES:
        pre = case["name"] + "/"
        train, val, tables, vtabs = iu.case_tables(case)
        assert np.array_equal(fx[pre + "train"], train) and np.array_equal(fx[pre + "val"], val)
        assert np.array_equal(fx[pre + "tables"], np.stack(tables)) and np.array_equal(fx[pre + "eval_states/idx"], vtabs[0][0])
        assert fx[pre + "loss"].shape == (case["epochs"], 2) and fx[pre + "counts"].shape == (case["epochs"], 2, iu.n_counts(case["A"]))
        assert fx[pre + "init/weight"].shape == (case["A"], 2 * case["S"]) and fx[pre + "init/weight"].dtype == np.float32
        states, actions, es = iu.case_recording(case)
        assert states.shape == (300, case["S"]) and actions.max() == case["A"] - 1 and es.sum() == 10
        assert max(spread["cases"][case["name"]][k] for k in ("param", "eval_states", "loss")) <= 1e-3
        # the cap on soft rows holds on the float64 side: a condition of the fixture
        f64 = iu.float64_run(case, iu.flatten_state_dict({k: fx[pre + "init/" + k] for k in iu.KEYS}))
        for ph, rows in zip(f64["phases"][-1], (tables[0].size, len(val))):
            assert ph.bounds()[2] <= 0.01 * rows
