"""Host side of evaluation.predict_reward (no GPU): the reference's command line, the split and skip-short-batch bookkeeping against
the runs recorded from the unmodified reference, the reward-to-class cast, the refusal to run without a GPU, the spread file's own
conditions, the new C symbols."""
import numpy as np
import pytest
import torch

import reward_util as ru


@pytest.fixture(scope="module")
def pr():
    from evaluation import predict_reward
    return predict_reward


@pytest.fixture(scope="module")
def fixture():
    return ru.load_fixture()


def test_parser_has_the_references_flags_and_defaults(pr):
    a = pr.build_parser().parse_args(["--data-folder", "data/x"])
    assert (a.epochs, a.seed, a.batch_size, a.training_set_size, a.learning_rate, a.no_cuda, a.data_folder, a.input_file) == \
        (10, 1, 32, -1, 0.005, False, "data/x", "")
    a = pr.build_parser().parse_args(["--epochs", "3", "--seed", "7", "-bs", "8", "--training-set-size", "100", "-lr", "0.01",
                                      "--no-cuda", "--data-folder", "d", "-i", "s.npz"])
    assert (a.epochs, a.seed, a.batch_size, a.training_set_size, a.learning_rate, a.no_cuda, a.data_folder, a.input_file) == \
        (3, 7, 8, 100, 0.01, True, "d", "s.npz")
    a = pr.build_parser().parse_args(["--batch-size", "4", "--learning-rate", "0.1", "--input-file", "t.npz", "--data-folder", "d"])
    assert (a.batch_size, a.learning_rate, a.input_file) == (4, 0.1, "t.npz")
    with pytest.raises(SystemExit):
        pr.build_parser().parse_args([])  # --data-folder is required


@pytest.mark.parametrize("case", ru.CASES, ids=[c["name"] for c in ru.CASES])
def test_split_and_minibatch_bookkeeping(pr, fixture, case, tmp_path, monkeypatch, capsys):
    pre = case["name"] + "/"
    argv = ru.write_case(str(tmp_path), case)
    monkeypatch.chdir(tmp_path)
    args = pr.build_parser().parse_args(argv)
    states, classes, indices = pr.prepare(args)
    out = capsys.readouterr().out
    assert "%d samples" % (case["n_episodes"] * case["ep_len"] - 1) in out
    assert ("Using ground truth" in out) == (not case["latent"])
    assert classes.dtype == np.int64 and set(classes.tolist()) <= {0, 1}
    assert states.shape == (case["n_episodes"] * case["ep_len"], case["latent"] or 3)
    assert np.array_equal(indices, fixture[pre + "indices"])
    starts = ru.case_arrays(case)["episode_starts"]
    assert not starts[indices + 1].any() and len(indices) == len(starts) - case["n_episodes"]

    torch.manual_seed(case["seed"])
    x_train, x_val = pr.splitIndices(indices, case["seed"])
    assert [len(x_train), len(x_val)] == fixture[pre + "phase_sizes"].tolist()
    datasets, loaders = pr.makeLoaders(x_train, x_val, case["bs"])
    replay = ru.replay_tables(indices, case["seed"], case["bs"], case["epochs"])  # reseeds torch
    torch.manual_seed(case["seed"])
    for e in range(case["epochs"]):
        for j, phase in enumerate(pr.PHASES):
            tab = pr.phaseTable(loaders[phase], case["bs"])
            assert tab.dtype == torch.int32 and tab.is_contiguous() and tab.device.type == "cpu"
            assert len(tab) == fixture[pre + "n_batches"][e, j] == len(datasets[phase]) // case["bs"]
            assert np.array_equal(tab.numpy(), replay[e][j])
    assert len(datasets["train"]) % case["bs"] != 0, "the case must leave a short minibatch to skip"


def test_training_set_size_truncates(pr, tmp_path, monkeypatch, capsys):
    case = ru.CASES[0]
    argv = ru.write_case(str(tmp_path), case) + ["--training-set-size", "100"]
    monkeypatch.chdir(tmp_path)
    states, classes, indices = pr.prepare(pr.build_parser().parse_args(argv))
    assert len(states) == len(classes) == 100 and "99 samples" in capsys.readouterr().out
    assert indices.max() <= 98 and 39 not in indices and 79 not in indices and 38 in indices


def test_reward_classes(pr):
    assert pr.rewardClasses(np.array([0.0, 1.0, -1.0, 1.0])).tolist() == [0, 1, 0, 1]      # floats, as the test datasets store them
    assert pr.rewardClasses(np.array([-5, 0, 1])).tolist() == [0, 0, 1]                      # every negative reward counts as 0
    assert pr.rewardClasses(np.array([0.5, 1.9])).tolist() == [0, 1]                         # .long() truncates
    raw = np.array([-1.0, 1.0])
    pr.rewardClasses(raw)
    assert raw.tolist() == [-1.0, 1.0], "the caller's array is not touched"
    with pytest.raises(ValueError, match=r"the reward head has two classes.*found classes \[0, 1, 2\]"):
        pr.rewardClasses(np.array([0, 1, 2]))


def test_phase_table_skips_short_minibatches(pr):
    from torch.utils.data import TensorDataset, DataLoader
    loader = DataLoader(TensorDataset(torch.arange(10)), batch_size=4, shuffle=False)
    assert pr.phaseTable(loader, 4).tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    short = DataLoader(TensorDataset(torch.arange(3)), batch_size=4, shuffle=False)
    tab = pr.phaseTable(short, 4)
    assert tuple(tab.shape) == (0, 4) and tab.dtype == torch.int32


def test_no_cuda_raises(pr, tmp_path, monkeypatch):
    from srlz._cabi import SrlzError
    case = ru.CASES[0]
    argv = ru.write_case(str(tmp_path), case)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SrlzError, match="no CPU fallback"):
        pr.main(argv + ["--no-cuda"])
    if not torch.cuda.is_available():
        with pytest.raises(SrlzError, match="no CPU fallback"):
            pr.main(argv)


def test_parameter_container(pr):
    from models.forward_inverse import BaseRewardModel
    model = BaseRewardModel()
    model.initRewardNet(5, n_rewards=2, n_hidden=4)
    assert list(model.state_dict().keys()) == list(ru.KEYS)
    flat = pr.flatParameters(model)
    assert flat.dtype == torch.float32 and flat.numel() == ru.n_params(5)
    assert np.array_equal(flat.numpy().astype(np.float64), ru.flatten_state_dict(model.state_dict()))
    pr.storeParameters(model, flat + 1)
    assert np.array_equal(pr.flatParameters(model).numpy(), (flat + 1).numpy())


def test_spread_file(fixture):
    spread = ru.load_spread()
    assert spread["refused_above"] == 1e-3 and "endpoint_errors" in spread["metric"]
    assert set(spread["cases"]) == {c["name"] for c in ru.CASES}
    for case in ru.CASES:
        s = spread["cases"][case["name"]]
        for k in ("param", "eval_states", "loss"):
            assert 0 < s[k] <= spread["refused_above"], (case["name"], k, s[k])
        loss = fixture[case["name"] + "/loss"][:, 0]
        assert s["loss_first_last"] == [loss[0], loss[-1]]
        assert loss[-1] < 0.8 * loss[0], "training must visibly move in the recorded case"


def test_float64_restatement_reproduces_the_recorded_losses(fixture):
    """The restatement the GPU tests measure against, over the replayed minibatch order, lands on the reference's own losses."""
    case = ru.CASES[0]
    pre = case["name"] + "/"
    flat = ru.flatten_state_dict({k: fixture[pre + "init/" + k] for k in ru.KEYS})
    states = np.asarray(ru.case_states(case), dtype=np.float32)
    labels = np.maximum(ru.case_arrays(case)["rewards"], 0).astype(np.int64)
    m, v, t = np.zeros_like(flat), np.zeros_like(flat), 0
    for e, (train, val) in enumerate(ru.replay_tables(fixture[pre + "indices"], case["seed"], case["bs"], 2)):
        flat, m, v, ph, _ = ru.fit(flat, m, v, t, states, labels, train, case["lr"])
        t += len(train)
        assert abs(ph.running_loss / fixture[pre + "phase_sizes"][0] - fixture[pre + "loss"][e, 0]) <= 1e-6 * fixture[pre + "loss"][e, 0]
        assert np.array_equal(ph.counts(), fixture[pre + "counts"][e, 0])


def test_exported_symbols(cabi):
    for name in ("srlz_reward_probe_fit", "srlz_reward_probe_eval", "srlz_reward_probe_eval_workspace", "srlz_reward_probe_chunk_rows"):
        assert name in cabi.EXPORTED
    assert cabi.ABI_VERSION == 104
    assert cabi.reward_probe_chunk_rows(200) >= 32, "the reference's minibatch of 32 is one chunk at S = 200"
    assert cabi.reward_probe_chunk_rows(513) == 0 and cabi.reward_probe_chunk_rows(0) == 0
    assert cabi.reward_probe_eval_workspace(300, 8) >= 8 * ((300 * 8 + 63) // 64)
