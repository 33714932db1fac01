"""evaluation.predict_forward --fit --fit-inverse on a tiny generated log folder (tests/dataset_util.make_dataset), and --fit
without the new flag, whose file has no `inverse_fit`."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest

import dataset_util
import reward_util as ru

pytestmark = pytest.mark.gpu

EPISODES, EP_LEN, S, A = 10, 12, 5, 4
INVERSE = ["--fit-inverse", "--inverse-epochs", "3", "--inverse-batch-size", "8"]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """One dataset and one log folder for the module: (root, log folder relative to it, actions, episode_starts)."""
    root = str(tmp_path_factory.mktemp("invfit_cli"))
    name, _, actions, rewards, starts = dataset_util.make_dataset(root, "tiny_invfit", n_episodes=EPISODES, ep_len=EP_LEN, n_actions=A,
                                                                  seed=41)
    log = os.path.join(root, "logs", name, "run")
    os.makedirs(log)
    with open(os.path.join(log, "exp_config.json"), "w") as f:
        json.dump(OrderedDict([("data-folder", name), ("state-dim", S)]), f)
    arrays = ru.dataset_arrays(EPISODES, EP_LEN, n_actions=A, seed=41)  # the arrays make_dataset stored, without its frames
    assert np.array_equal(arrays["actions"], actions)
    np.savez(os.path.join(log, "states_rewards.npz"), states=ru.latent_states(arrays, S, 42), rewards=rewards)
    return root, os.path.join("logs", name, "run"), actions, starts


def test_fit_inverse_writes_the_inverse_fit_and_a_second_run_repeats_it(folder, monkeypatch, capsys):
    from evaluation import predict_forward as pf
    from srlz import dynfit, headfit
    root, log, actions, es = folder
    monkeypatch.chdir(root)
    out = pf.main(["--log-folder", log, "--horizon", "2", "--fit"] + INVERSE)
    text = capsys.readouterr().out
    train, val = dynfit.split_episodes(es, 0.2, 0)
    fit_side, select_side = headfit.split_starts(train, es, 0.2, 0)  # the validation episodes take no part in the fit
    assert not set(select_side) & set(val) and not set(fit_side) & set(val)
    assert tuple(sorted(out)) == tuple(sorted(pf.KEYS + ("train", "fit", "inverse_fit")))
    inv = out["inverse_fit"]
    assert tuple(sorted(inv)) == tuple(sorted(pf.INVERSE_KEYS))
    assert (inv["route"], inv["epochs"], inv["batch_size"], inv["lr"], inv["seed"]) == ("kernel", 3, 8, 0.005, 0)
    assert inv["count"] == len(val) and inv["fit_count"] == len(fit_side) and inv["select_count"] == len(select_side)
    assert inv["best_epoch"] in (0, 1, 2) and 0.0 <= inv["accuracy"] <= 1.0
    assert inv["majority_accuracy"] == np.bincount(actions[val], minlength=A).max() / len(val)
    assert len(inv["recall"]) == A and all(r is None or 0.0 <= r <= 1.0 for r in inv["recall"])
    assert text.count("Inverse head fitted on %d transitions: route kernel" % len(fit_side)) == 1 and "action acc" in text
    assert json.load(open(os.path.join(root, log, pf.OUTPUT_FIT))) == json.loads(json.dumps(out))
    # a second run gives identical numbers
    again = pf.main(["--log-folder", log, "--horizon", "2", "--fit"] + INVERSE)
    assert again == out
    # the forward side is what --fit alone reports
    plain = pf.main(["--log-folder", log, "--horizon", "2", "--fit"])
    for k in ("count", "mse", "baseline_mse", "ratio"):
        assert plain[k] == out[k] and plain["train"][k] == out["train"][k]
    assert plain["fit"] == out["fit"]
    # the other settings reach the fit, and the reward head beside it
    other = pf.main(["--log-folder", log, "--horizon", "2", "--fit", "--fit-inverse", "--inverse-epochs", "1", "--inverse-lr", "0.01",
                     "--seed", "3", "--fit-reward", "--reward-epochs", "1"])
    assert (other["inverse_fit"]["batch_size"], other["inverse_fit"]["lr"], other["inverse_fit"]["seed"], other["inverse_fit"]["epochs"]) \
        == (32, 0.01, 3, 1)
    assert "reward_fit" in other and other["reward_accuracy"] is not None


def test_without_the_flag_the_file_has_no_inverse_fit(folder, monkeypatch, capsys):
    from evaluation import predict_forward as pf
    root, log, actions, es = folder
    monkeypatch.chdir(root)
    out = pf.main(["--log-folder", log, "--horizon", "2", "--fit"])
    text = capsys.readouterr().out
    assert "inverse_fit" not in out and "Inverse head" not in text and "action acc" not in text
    assert tuple(sorted(out)) == tuple(sorted(pf.KEYS + ("train", "fit")))
    written = json.load(open(os.path.join(root, log, pf.OUTPUT_FIT)))
    assert "inverse_fit" not in written and written == json.loads(json.dumps(out))


def test_fit_inverse_without_fit_is_an_argparse_error(folder, capsys):
    from evaluation import predict_forward as pf
    root, log, actions, es = folder
    with pytest.raises(SystemExit):
        pf.main(["--log-folder", log, "--fit-inverse"])
    assert "--fit-inverse only with --fit" in capsys.readouterr().err
