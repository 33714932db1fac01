"""`python -m srl_baselines.pca` as a child process on the generated dataset (GPU), against the reference's own script run recorded in
tests/golden/loop_pca.npz (tools/make_golden_pca.py): folder and file names, exp_config.json, the states, the fields of pca.pkl, one
decode per frame — then `python -m evaluation.knn_images` on that log folder.  One run serves the whole module.

Bound on the states and the pickled fields: max(1e-4, 10 x the largest spread recorded in pca_spread.json) of each quantity's scale,
as in tests/test_pca_fit_gpu.py (the dataset's own spread is not recorded; its frames are smooth and its three kept singular values
well separated)."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import pca_util as pu
from dataset_util import make_dataset

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "srl-zoo_amd")


def _run(cmd, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    proc = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = proc.stdout.decode("utf-8", "replace")
    assert proc.returncode == 0, out[-3000:]
    return out


@pytest.fixture(scope="module")
def golden():
    return gu.load("loop_pca")


@pytest.fixture(scope="module")
def fitted(tmp_path_factory, golden):
    """:return: (root, log folder relative to root, the child's output)"""
    cfg = json.loads(str(golden["config"]))
    root = str(tmp_path_factory.mktemp("pcacli"))
    name = make_dataset(root, n_episodes=cfg["n_episodes"], ep_len=cfg["ep_len"])[0]
    out = _run([sys.executable, "-m", "srl_baselines.pca", "--data-folder", name, "--state-dim", str(cfg["state_dim"]),
                "--no-display-plots"], root)
    return root, cfg["log_folder"], out


def _tol():
    return max(pu.tolerance(s) for s in pu.load_spread().values())


def test_files_and_folder_names_are_the_reference_s(fitted, golden):
    root, log, out = fitted
    assert log == "logs/tiny_test/baselines/pca_ST_DIM3"
    assert sorted(os.listdir(os.path.join(root, log))) == [str(f) for f in golden["files"]]
    assert os.path.isdir(os.path.join(root, log, "NearestNeighbors"))
    assert json.load(open(os.path.join(root, log, "exp_config.json"))) == json.loads(str(golden["exp_config"]))
    assert "batch_size = 16" in out and "Fitting PCA with n_components=3" in out


def test_states_match_the_recorded_reference_run(fitted, golden):
    root, log, _ = fitted
    z = np.load(os.path.join(root, log, "states_rewards.npz"))
    want = golden["states"]
    assert z["states"].shape == want.shape == (72, 3) and z["rewards"].shape == (72,)
    err = float(np.abs(z["states"] - want).max() / np.abs(want).max())
    print("states vs the reference's run: %.2e of scale (bound %.1e)" % (err, _tol()))
    assert err <= _tol()
    table = json.load(open(os.path.join(root, log, "image_to_state.json")))
    paths = np.load(os.path.join(root, "data", "tiny_test", "ground_truth.npz"))["images_path"]
    assert sorted(table) == sorted(paths) and len(table[paths[0]]) == 3


def test_pickle_holds_the_reference_s_fields(fitted, golden):
    root, log, _ = fitted
    with open(os.path.join(root, log, "pca.pkl"), "rb") as f:
        ipca = pickle.load(f)
    tol = _tol()
    for f in ("singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_"):
        want = golden["pkl/" + f]
        got = np.asarray(getattr(ipca, f))
        assert got.shape == want.shape and got.dtype == want.dtype, f
        assert np.abs(got - want).max() <= tol * np.abs(want).max(), f
    assert ipca.n_samples_seen_ == int(golden["pkl/n_samples_seen_"]) == 72 and ipca.n_components_ == int(golden["pkl/n_components_"]) == 3
    for f in ("components_", "mean_", "var_"):
        assert getattr(ipca, f).dtype == np.float64
        gu.check_digest(getattr(ipca, f), golden, "pkl/" + f, rtol=tol)
    # the unpickled object transforms on the host
    states = np.load(os.path.join(root, log, "states_rewards.npz"))["states"]
    rs = np.random.RandomState(0)
    x = rs.randn(2, ipca.mean_.shape[0]).astype(np.float32)
    assert ipca.transform(x).shape == (2, 3) and states.dtype == np.float32


def test_every_frame_was_decoded_once(fitted):
    _, _, out = fitted
    m = re.search(r"Decoded (\d+) frames for (\d+) observations \(store: (\w+)\)", out)
    assert m, out[-2000:]
    assert (int(m.group(1)), int(m.group(2)), m.group(3)) == (72, 72, "device")


def test_knn_images_on_the_pca_log_folder(fitted):
    root, log, _ = fitted
    _run([sys.executable, "-m", "evaluation.knn_images", "--log-folder", log, "-n", "20", "--n-to-plot", "0"], root)
    got = json.load(open(os.path.join(root, log, "knn_mse.json")))
    assert sorted(got) == ["images", "knn_mse"] and len(got["images"]) == 20 and got["knn_mse"] > 0
