"""The ground-truth correlation after a real training run (GPU): train.py leaves gt_correlation.json, `python -m
plotting.representation_plot --correlation --print-corr` rewrites it, pipeline.correlationCall fails as the reference's does without
states_rewards.npz, and `python -m evaluation.gather_results` puts it beside the KNN-MSE into results.csv.  One `train.py` run serves
the whole module; every child process runs in a session of its own under a time limit, and at most two of them hold the GPU at once
(train.py waiting for its evaluation child)."""
import functools
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import gtc_util as gu
from dataset_util import make_dataset

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "srl-zoo_amd")
CHILD_SECONDS = 300


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def _run(cmd, cwd):
    """The command and whatever it starts, ended together at the time limit. :return: its output"""
    proc = subprocess.Popen(cmd, cwd=cwd, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        raise
    out = out.decode("utf-8", "replace")
    assert proc.returncode == 0, out[-3000:]
    return out


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """:return: (root, log folder, dataset name, train.py's output) after
    `train.py --losses autoencoder --state-dim 10 -bs 8 --epochs 1 --seed 0`"""
    root = str(tmp_path_factory.mktemp("gtccli"))
    name = make_dataset(root, n_episodes=3, ep_len=20)[0]
    log = os.path.join(root, "logs", "cli_gtc", "run")
    out = _run([sys.executable, os.path.join(PKG, "train.py"), "--no-display-plots", "--data-folder", name, "--losses", "autoencoder",
                "--state-dim", "10", "-bs", "8", "--epochs", "1", "--seed", "0", "--log-folder", log], root)
    cwd = os.getcwd()
    os.chdir(root)
    yield root, log, name, out
    os.chdir(cwd)


def _numpy_gtc(root, log, name):
    """The reference's arithmetic in extended precision on the run's own files. :return: (gt_corr [6], mean)"""
    states = np.load(os.path.join(log, "states_rewards.npz"))["states"]
    gt = np.load(os.path.join(root, "data", name, "ground_truth.npz"))
    starts = np.load(os.path.join(root, "data", name, "preprocessed_data.npz"))["episode_starts"]
    per_frame_target = gt["target_positions"][np.cumsum(starts) - 1]
    out = []
    for x in (gt["ground_truth_states"], per_frame_target):
        x = x[:len(states)]
        corr = np.corrcoef(x + 1e-12, states + 1e-12, rowvar=0, dtype=np.longdouble)
        for i in range(x.shape[1]):
            corr[i, i] = 0.0
            out.append(float(np.abs(corr[i]).max()))
    return np.array(out), sum(out) / len(out)


def test_train_leaves_the_ground_truth_correlation(trained):
    root, log, name, out = trained
    assert os.path.isfile(os.path.join(log, "gt_correlation.json")), os.listdir(log)
    got = json.load(open(os.path.join(log, "gt_correlation.json")))
    assert sorted(got) == ["gt_corr", "gt_corr_mean"] and len(got["gt_corr"]) == 6
    states = np.load(os.path.join(log, "states_rewards.npz"))["states"]
    assert states.shape == (60, 10)
    want, want_mean = _numpy_gtc(root, log, name)
    err = np.abs(np.array(got["gt_corr"]) - want)
    print("worst error %.3e (bound %.3e)" % (err.max(), gu.bound(60)))
    assert np.isfinite(want).all() and (err <= gu.bound(60)).all(), (got["gt_corr"], want.tolist())
    assert abs(got["gt_corr_mean"] - want_mean) <= gu.bound(60)
    assert "Max correlation vector (GTC)" in out and "End of correlationCall" in out
    assert not [f for f in os.listdir(log) if f.endswith(".png")]


def test_command_line_rewrites_the_file(trained):
    root, log, name, _ = trained
    path = os.path.join(log, "gt_correlation.json")
    first = json.load(open(path))
    os.remove(path)
    out = _run([sys.executable, "-m", "plotting.representation_plot", "-i", os.path.join(log, "states_rewards.npz"),
                "--data-folder", "data/" + name, "--correlation", "--print-corr"], root)
    assert json.load(open(path)) == first  # the same sums in the same order: bit for bit
    assert "Max correlation vector (GTC)" in out and " Mean : {:.2f}".format(first["gt_corr_mean"]) in out
    assert not [f for f in os.listdir(log) if f.endswith(".png")]


def test_correlation_call_fails_without_states(trained, tmp_path, monkeypatch):
    root, log, name, _ = trained
    import pipeline
    empty = str(tmp_path / "no_states")
    os.makedirs(empty)
    monkeypatch.setattr(subprocess, "call", functools.partial(subprocess.call, timeout=CHILD_SECONDS))
    with pytest.raises(RuntimeError):
        pipeline.correlationCall({"log-folder": empty, "data-folder": name}, plot=False)
    assert not os.path.exists(os.path.join(empty, "gt_correlation.json"))


def test_gather_results_after_training(trained):
    root, log, name, _ = trained
    logs = os.path.dirname(log)
    out = _run([sys.executable, "-m", "evaluation.gather_results", "-i", logs], root)  # computes the missing knn_mse.json on its way
    rows = gu.read_csv(os.path.join(logs, "results.csv"))
    assert len(rows) == 2 and "Found 1 experiments" in out
    row = dict(zip(rows[0], rows[1]))
    corr = json.load(open(os.path.join(log, "gt_correlation.json")))
    knn = json.load(open(os.path.join(log, "knn_mse.json")))
    assert row["experiments"] == "run" and float(row["state-dim"]) == 10 and float(row["seed"]) == 0
    assert float(row["gt_mean"]) == corr["gt_corr_mean"] and json.loads(row["gt_corr"]) == corr["gt_corr"]
    assert float(row["knn_mse"]) == knn["knn_mse"] and knn["knn_mse"] >= 0
