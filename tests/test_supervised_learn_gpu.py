"""The supervised baseline through its public surface (GPU): SupervisedLearning.learn() on the generated dataset against the UNMODIFIED
reference loop (tools/make_golden_supervised.py loop_sup_cnn / loop_sup_mlp: forked loaders, sklearn's split, ragged minibatches taken
in order (the reference's loader resets its shuffle flag), eval-mode validation, best-epoch checkpoint, states of the reloaded model), with the bounds tests/test_loop_gpu.py
holds the other loops to; and the command line in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from dataset_util import make_dataset
from supervised_util import best_epoch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "srl-zoo_amd")
HIST_RTOL, STATE_RTOL, PARAM_TOL = 1e-3, 2e-2, 2e-2  # as tests/test_loop_gpu.py (chaos-limited after 10-20 Adam steps)


@pytest.mark.parametrize("name", ["loop_sup_cnn", "loop_sup_mlp"])
@pytest.mark.timeout(600)
def test_learn_loop_follows_reference(name, tmp_path):
    import preprocessing.preprocess as pre
    import srl_baselines.supervised as sup
    from utils import loadData
    g = gu.load(name)
    cfg = json.loads(str(g["config"]))
    ds = make_dataset(str(tmp_path), n_episodes=cfg["n_episodes"], ep_len=cfg["ep_len"])[0]
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    saved = (sup.DISPLAY_PLOTS, sup.N_EPOCHS, sup.BATCH_SIZE, sup.TEST_BATCH_SIZE)
    try:
        os.makedirs("logs/run", exist_ok=True)
        pre.N_CHANNELS = 3
        sup.DISPLAY_PLOTS, sup.N_EPOCHS, sup.BATCH_SIZE, sup.TEST_BATCH_SIZE = False, cfg["n_epochs"], cfg["bs"], cfg["test_bs"]
        training_data, ground_truth, true_states, _ = loadData(ds)
        srl = sup.SupervisedLearning(true_states.shape[1], model_type=cfg["model_type"], seed=cfg["seed"], log_folder="logs/run",
                                     learning_rate=cfg["lr"], cuda=True)
        states = srl.learn(true_states, ground_truth["images_path"], training_data["rewards"])
        sd = torch.load("logs/run/srl_supervised_model.pth", map_location="cpu")
        with np.load("logs/run/loss.npz") as z:
            hist = {"train": np.asarray(z["train"], dtype=np.float64), "val": np.asarray(z["val"], dtype=np.float64)}
    finally:
        sup.DISPLAY_PLOTS, sup.N_EPOCHS, sup.BATCH_SIZE, sup.TEST_BATCH_SIZE = saved
        os.chdir(cwd)
    for nm in ("train", "val"):
        got, ref = hist[nm], g["loss/" + nm]
        assert got.shape == ref.shape, (nm, got.shape, ref.shape)
        print(name, nm, "worst rel err %.2e" % float(np.abs(got - ref).max() / np.abs(ref).max()))
        assert abs(got[0, 0] - ref[0, 0]) <= HIST_RTOL * abs(ref[0, 0]), (nm, got, ref)
        assert float(np.abs(got - ref).max() / np.abs(ref).max()) <= 5 * HIST_RTOL, (nm, got, ref)
    assert srl.best_epoch == int(g["best_epoch"]) == best_epoch(hist["val"])
    ref_states = g["states/full"]
    assert states.shape == ref_states.shape
    assert float(np.abs(states - ref_states).max() / np.abs(ref_states).max()) <= STATE_RTOL
    assert list(sd.keys()) == [str(k) for k in g["final/names"]] and all(not v.is_cuda for v in sd.values())
    steps = (int(g["best_epoch"]) + 1) * g["loss/train"].shape[1]
    for k, ref_sum, ref_abs in zip(g["final/names"], g["final/sums"], g["final/abss"]):
        k = str(k)
        v = sd[k].double()
        if "num_batches_tracked" in k:
            assert int(v) == int(ref_sum), k
        else:
            e = max(abs(float(v.sum()) - ref_sum), abs(float(v.abs().sum()) - ref_abs)) / (ref_abs + cfg["lr"] * steps * v.numel())
            assert e <= PARAM_TOL, (k, e)


@pytest.mark.timeout(600)
def test_command_line_writes_the_reference_files(tmp_path):
    make_dataset(str(tmp_path), name="tiny_sup", n_episodes=3, ep_len=20)
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG + os.pathsep + env.get("PYTHONPATH", "")
    args = ["timeout", "-k", "10", "500", sys.executable, "-m", "srl_baselines.supervised", "--data-folder", "data/tiny_sup/",
            "--no-display-plots", "--epochs", "1", "--model-type", "custom_cnn", "-bs", "8", "-lr", "0.001"]
    r = subprocess.run(args, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode("utf-8", "replace")
    assert r.returncode == 0, text[-4000:]
    folder = os.path.join(str(tmp_path), "logs", "tiny_sup", "baselines", "supervised_custom_cnn_SEED1_EPOCHS1_BS8")
    for f in ("loss.npz", "srl_supervised_model.pth", "states_rewards.npz", "image_to_state.json", "exp_config.json"):
        assert os.path.exists(os.path.join(folder, f)), (f, text[-2000:])
    assert not os.path.exists(os.path.join(folder, "learned_states.png"))
    with open(os.path.join(folder, "exp_config.json")) as f:
        cfg = json.load(f)
    assert cfg["losses"] == ["supervised"] and cfg["model-type"] == "custom_cnn" and cfg["state-dim"] == 3 and cfg["batch-size"] == 8
    with np.load(os.path.join(folder, "loss.npz")) as z:
        # 60 frames -> 40 for training = 5 minibatches of 8 (the sixth slice is empty and dropped), 20 for validation = 1 minibatch
        assert z["train"].shape == (1, 5) and z["val"].shape == (1, 1) and np.isfinite(z["train"]).all()
    with np.load(os.path.join(folder, "states_rewards.npz")) as z:
        assert z["states"].shape == (60, 3) and np.isfinite(z["states"]).all() and z["rewards"].shape == (60,)
    with open(os.path.join(folder, "image_to_state.json")) as f:
        assert len(json.load(f)) == 60
    from models import CustomCNN
    sd = torch.load(os.path.join(folder, "srl_supervised_model.pth"), map_location="cpu")
    assert all(not v.is_cuda for v in sd.values()) and sd["conv_layers.0.weight"].shape == (64, 3, 7, 7) and sd["fc.weight"].shape == (3, 2304)
    CustomCNN(3).load_state_dict(sd, strict=True)
