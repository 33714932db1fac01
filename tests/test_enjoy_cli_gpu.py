"""`python -m evaluation.enjoy_latent --sheet-dir` after real training runs (GPU): the decoder sheet of an auto-encoder, tile by tile
against getImage, and the nearest-frame sheet of an inverse model against knnImageIndex on the run's own image_to_state.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dataset_util import make_dataset

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "srl-zoo_amd")
STEPS = 3


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def _run(cmd, cwd):
    proc = subprocess.run(cmd, cwd=cwd, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = proc.stdout.decode("utf-8", "replace")
    assert proc.returncode == 0, out[-3000:]
    return out


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("enjoycli"))
    name = make_dataset(root, n_episodes=3, ep_len=20)[0]
    cwd = os.getcwd()
    os.chdir(root)
    yield root, name
    os.chdir(cwd)


def _train_and_sheet(root, name, losses, tag):
    log = os.path.join(root, "logs", tag)
    _run([sys.executable, os.path.join(PKG, "train.py"), "--no-display-plots", "--data-folder", name, "--losses", losses,
          "--state-dim", "4", "-bs", "8", "--epochs", "1", "--seed", "0", "--log-folder", log], root)
    out = os.path.join(root, "out_" + tag)
    _run([sys.executable, "-m", "evaluation.enjoy_latent", "--log-dir", log + "/", "--sheet-dir", out, "--steps", str(STEPS)], root)
    with open(os.path.join(out, "traversal.json")) as f:
        record = json.load(f)
    return log, out, record


def _tiles(sheet, rows, cols, h, w, gap):
    return [[sheet[gap + r * (h + gap):gap + r * (h + gap) + h, gap + c * (w + gap):gap + c * (w + gap) + w] for c in range(cols)]
            for r in range(rows)]


def test_decoder_sheet_after_training(workdir):
    from PIL import Image
    import torch
    from evaluation import enjoy_latent as enjoy
    from models.learner import SRL4robotics
    root, name = workdir
    log, out, record = _train_and_sheet(root, name, "autoencoder", "cli_ae")
    assert os.listdir(out).count("Decoder_for_autoencoder.png") == 1 and sorted(os.listdir(out)) == ["Decoder_for_autoencoder.png",
                                                                                                      "traversal.json"]
    assert len(record) == 1
    block = record[0]
    assert (block["name"], block["start"], block["end"], block["positions"]) == ("Decoder for autoencoder", 0, 4, [0, 50, 100])
    assert "images" not in block
    X, _ = enjoy.loadStates(log + "/")
    bound_min, bound_max = np.array(block["bound_min"]), np.array(block["bound_max"])
    assert np.array_equal(bound_min, X.min(axis=0)) and np.array_equal(bound_max, X.max(axis=0))

    gap = enjoy.SHEET_GAP
    with Image.open(os.path.join(out, "Decoder_for_autoencoder.png")) as f:
        assert f.mode == "RGB"
        sheet = np.asarray(f).copy()
    assert sheet.shape == (4 * 224 + 5 * gap, STEPS * 224 + (STEPS + 1) * gap, 3)
    tiles = _tiles(sheet, 4, STEPS, 224, 224, gap)
    picture = np.zeros(sheet.shape[:2], dtype=bool)
    for r in range(4):
        for c in range(STEPS):
            picture[gap + r * (224 + gap):gap + r * (224 + gap) + 224, gap + c * (224 + gap):gap + c * (224 + gap) + 224] = True
    assert (sheet[~picture] == enjoy.SHEET_FILL).all()
    # the centre column has every slider at 50: the same picture in every row
    for r in range(1, 4):
        assert np.array_equal(tiles[r][1], tiles[0][1])
    assert not np.array_equal(tiles[0][0], tiles[0][2])

    # tile (i, j) is getImage of the state traversal.json implies, on the model as the reference leaves it: in training mode
    srl, _ = SRL4robotics.loadSavedModel(log + "/", enjoy.VALID_MODELS, cuda=True)
    model = srl.model
    model.train()
    device = torch.device("cuda")
    for i in range(4):
        for j, p in enumerate(block["positions"]):
            sliders = [50] * 4
            sliders[i] = p
            full = enjoy.fullState(4, 0, 4, enjoy.sliderState(sliders, bound_min, bound_max))
            img = enjoy.getImage(model.model, full, device)
            want = np.rint(img[:, :, ::-1] * np.float32(255)).astype(np.uint8)
            assert np.array_equal(tiles[i][j], want), (i, j, np.abs(tiles[i][j].astype(int) - want.astype(int)).max())


def test_knn_sheet_after_training(workdir):
    from PIL import Image
    from evaluation import enjoy_latent as enjoy
    root, name = workdir
    log, out, record = _train_and_sheet(root, name, "inverse", "cli_inverse")
    assert sorted(os.listdir(out)) == ["KNN_on_inverse.png", "traversal.json"]
    block = record[0]
    assert (block["name"], block["start"], block["end"], block["positions"]) == ("KNN on inverse", 0, 4, [0, 50, 100])
    X, y = enjoy.loadStates(log + "/")
    assert X.shape == (60, 4)
    bound_min, bound_max = np.array(block["bound_min"]), np.array(block["bound_max"])
    want = []
    for i in range(4):
        for p in block["positions"]:
            sliders = [50] * 4
            sliders[i] = p
            want.append(enjoy.knnImagePath(y, enjoy.knnImageIndex(X, enjoy.sliderState(sliders, bound_min, bound_max))))
    assert block["images"] == want and all(os.path.exists(os.path.join(root, p)) for p in want)
    gap = enjoy.SHEET_GAP
    with Image.open(os.path.join(out, "KNN_on_inverse.png")) as f:
        sheet = np.asarray(f).copy()
    assert sheet.shape == (4 * 224 + 5 * gap, STEPS * 224 + (STEPS + 1) * gap, 3)
    tiles = _tiles(sheet, 4, STEPS, 224, 224, gap)
    for k, p in enumerate(want):
        with Image.open(os.path.join(root, p)) as f:
            assert np.array_equal(tiles[k // STEPS][k % STEPS], np.asarray(f.convert("RGB"))), p
