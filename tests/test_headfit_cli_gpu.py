"""evaluation.predict_forward --fit --fit-reward on a generated dataset (tests/reward_util.write_dataset: no frames are read), and
--fit without the new flag, which writes what it wrote before."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest

import reward_util as ru

pytestmark = pytest.mark.gpu

EPISODES, EP_LEN, S = 10, 30, 5


def _setup(tmp_path):
    root = str(tmp_path)
    arrays = ru.dataset_arrays(EPISODES, EP_LEN, n_actions=4, seed=31)
    name = ru.write_dataset(root, "tiny_headfit", arrays)
    log = os.path.join(root, "logs", name, "run")
    os.makedirs(log)
    with open(os.path.join(log, "exp_config.json"), "w") as f:
        json.dump(OrderedDict([("data-folder", name), ("state-dim", S)]), f)
    np.savez(os.path.join(log, "states_rewards.npz"), states=ru.latent_states(arrays, S, 32), rewards=arrays["rewards"])
    return root, name, log, arrays


def test_fit_without_the_new_flag_writes_what_it_wrote(tmp_path, monkeypatch, capsys):
    """The JSON of --fit against the same computation made by hand the way run_fit made it before --fit-reward existed."""
    from evaluation import predict_forward as pf
    from srlz import dynfit
    from srlz.deploy import LatentDynamics
    root, name, log, arrays = _setup(tmp_path)
    monkeypatch.chdir(root)
    out = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "3", "--fit"])
    text = capsys.readouterr().out
    assert "Reward head" not in text and "reward acc" not in text
    states = np.asarray(np.load(os.path.join(log, "states_rewards.npz"))["states"], np.float32)
    actions, es = arrays["actions"], arrays["episode_starts"]
    train, val = dynfit.split_episodes(es, 0.2, 0)
    n_actions = int(actions[np.concatenate((train, val))].max()) + 1
    dyn = LatentDynamics.from_recording(states, actions, es, n_actions=n_actions, ridge=1e-6, starts=train, max_horizon=32)
    before = dyn.horizon_error(states, actions, es, 3, starts=val).as_dict()
    before["train"] = dyn.horizon_error(states, actions, es, 3, starts=train).as_dict()
    fit = dyn.fit
    before["fit"] = {"ridge": fit.ridge, "count": fit.count, "val_fraction": 0.2, "seed": 0, "route": fit.route, "state_dim": fit.state_dim,
                     "n_actions": fit.n_actions}
    assert out == before  # key for key, value for value
    assert tuple(sorted(out["fit"])) == tuple(sorted(pf.FIT_KEYS)) and "reward_fit" not in out
    assert tuple(sorted(out)) == tuple(sorted(pf.KEYS + ("train", "fit")))
    assert out["reward_accuracy"] is None and out["train"]["reward_accuracy"] is None
    assert json.load(open(os.path.join(log, pf.OUTPUT_FIT))) == json.loads(json.dumps(before))


def test_fit_reward_adds_the_reward_head(tmp_path, monkeypatch, capsys):
    from evaluation import predict_forward as pf
    from srlz import dynfit, headfit
    root, name, log, arrays = _setup(tmp_path)
    monkeypatch.chdir(root)
    out = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "3", "--fit", "--fit-reward", "--reward-epochs", "2"])
    text = capsys.readouterr().out
    train, val = dynfit.split_episodes(arrays["episode_starts"], 0.2, 0)
    # the head is fitted on four fifths of the training episodes and its epoch picked on the fifth: the validation episodes are held out
    fit_side, select_side = headfit.split_starts(train, arrays["episode_starts"], 0.2, 0)
    assert len(fit_side) == 6 * (EP_LEN - 1) and len(select_side) == 2 * (EP_LEN - 1) and not set(select_side) & set(val)
    assert out["count"][0] == len(val) and out["fit"]["count"] == len(train)
    assert tuple(sorted(out)) == tuple(sorted(pf.KEYS + ("train", "fit", "reward_fit")))
    assert tuple(sorted(out["fit"])) == tuple(sorted(pf.FIT_KEYS))
    rf = out["reward_fit"]
    assert sorted(rf) == sorted(["route", "hidden", "epochs", "batch_size", "lr", "seed", "best_epoch", "count", "val_count", "train_loss",
                                 "val_loss", "train_accuracy", "val_accuracy"])
    assert (rf["route"], rf["hidden"], rf["epochs"], rf["batch_size"], rf["lr"], rf["seed"]) == ("kernel", 16, 2, 32, 0.005, 0)
    assert rf["count"] == len(fit_side) and rf["val_count"] == len(select_side) and rf["best_epoch"] in (0, 1)
    for k in ("train_loss", "val_loss", "train_accuracy", "val_accuracy"):
        assert len(rf[k]) == 2 and all(np.isfinite(v) for v in rf[k])
    assert rf["best_epoch"] == int(np.argmin(rf["val_loss"]))
    for side in (out, out["train"]):
        assert len(side["reward_accuracy"]) == 3 and len(side["majority_accuracy"]) == 3
        assert all(v is not None and 0.0 <= v <= 1.0 for v in side["reward_accuracy"] + side["majority_accuracy"])
    assert text.count("reward acc") == 3 and "Reward head fitted on %d transitions: route kernel" % len(fit_side) in text
    assert json.load(open(os.path.join(log, pf.OUTPUT_FIT))) == json.loads(json.dumps(out))
    # the forward side is what --fit alone reports
    plain = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "3", "--fit"])
    for k in ("count", "mse", "baseline_mse", "ratio"):
        assert plain[k] == out[k] and plain["train"][k] == out["train"][k]
    assert plain["fit"] == out["fit"]
    # another batch size and rate reach the fit
    other = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "2", "--fit", "--fit-reward", "--reward-epochs", "1",
                     "--reward-batch-size", "8", "--reward-lr", "0.01", "--seed", "3"])
    assert (other["reward_fit"]["batch_size"], other["reward_fit"]["lr"], other["reward_fit"]["seed"], other["reward_fit"]["epochs"]) == (8, 0.01, 3, 1)
