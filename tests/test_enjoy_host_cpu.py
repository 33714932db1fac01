"""evaluation.enjoy_latent without a GPU and without a window: the blocks of a configuration, the slider arithmetic bit for bit, the
figure names, the behaviour without cv2, and the two symbols of csrc/latent.hip in the binding."""
import builtins
import importlib
import sys
from collections import OrderedDict

import numpy as np
import pytest


@pytest.fixture(scope="module")
def enjoy():
    return importlib.import_module("evaluation.enjoy_latent")


@pytest.fixture
def no_cv2(monkeypatch):
    """`import cv2` fails, whether or not the machine has it."""
    monkeypatch.delitem(sys.modules, "cv2", raising=False)
    real = builtins.__import__

    def fake(name, *a, **k):
        if name == "cv2" or name.startswith("cv2."):
            raise ImportError("No module named 'cv2'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", fake)


def test_module_imports_without_cv2(no_cv2):
    for name in [m for m in sys.modules if m == "evaluation.enjoy_latent"]:
        del sys.modules[name]
    mod = importlib.import_module("evaluation.enjoy_latent")
    assert "cv2" not in sys.modules
    assert mod.VALID_MODELS == ["forward", "inverse", "reward", "priors", "episode-prior", "reward-prior", "triplet", "autoencoder",
                                "vae", "dae", "random"]
    assert mod.AUTOENCODERS == ['autoencoder', 'vae', 'dae']
    for name in ("getImage", "createFigureAndSlider", "main", "lossBlocks", "loadStates", "blockBounds", "sliderState", "fullState",
                 "knnImageIndex", "decodeStates"):
        assert callable(getattr(mod, name)), name


def test_loss_blocks_no_split(enjoy, capsys):
    blocks = enjoy.lossBlocks({"losses": ["inverse", "autoencoder"], "state-dim": 6})
    assert list(blocks.items()) == [("inverse", (0, 6))]  # the FIRST loss decides, whatever follows it
    assert capsys.readouterr().out == "['inverse', 'autoencoder']\n"
    assert list(enjoy.lossBlocks({"losses": ["autoencoder"], "state-dim": 3, "split-dimensions": -1}).items()) == [("autoencoder", (0, 3))]


def test_loss_blocks_split_with_shared_entry(enjoy, capsys):
    cfg = {"losses": ["autoencoder", "reward", "inverse"], "state-dim": 5,
           "split-dimensions": OrderedDict([("autoencoder", 2), ("reward", -1), ("inverse", 3)])}
    blocks = enjoy.lossBlocks(cfg)
    assert list(blocks.items()) == [("autoencoder", (0, 2)), ("inverse", (2, 5))]
    assert capsys.readouterr().out == "autoencoder 2\nreward -1\ninverse 3\n"


def test_loss_blocks_single_entry_split(enjoy):
    cfg = {"losses": ["vae"], "state-dim": 4, "split-dimensions": OrderedDict([("vae", 4)])}
    assert list(enjoy.lossBlocks(cfg).items()) == [("vae", (0, 4))]
    # a lone entry gives a block whatever its size (`loss_dim > 0 or len(split_dimensions) == 1`)
    cfg = {"losses": ["vae"], "state-dim": 4, "split-dimensions": OrderedDict([("vae", -1)])}
    assert list(enjoy.lossBlocks(cfg).items()) == [("vae", (0, -1))]


def test_loss_blocks_plain_dict_is_not_a_split(enjoy, capsys):
    cfg = {"losses": ["autoencoder", "inverse"], "state-dim": 4, "split-dimensions": {"autoencoder": 2, "inverse": 2}}
    assert list(enjoy.lossBlocks(cfg).items()) == [("autoencoder", (0, 4))]
    assert capsys.readouterr().out == "['autoencoder', 'inverse']\n"


def test_slider_and_full_state_bit_for_bit(enjoy):
    rs = np.random.RandomState(0)
    for dim in (1, 3, 7):
        X = rs.randn(30, dim + 2) * 3
        bound_min, bound_max = enjoy.blockBounds(X, 1, 1 + dim)
        assert np.array_equal(bound_min, np.min(X[:, 1:1 + dim], axis=0)) and np.array_equal(bound_max, np.max(X[:, 1:1 + dim], axis=0))
        for positions in ([0] * dim, [50] * dim, [100] * dim, [int(p) for p in rs.randint(0, 101, dim)]):
            want = (np.array(positions) / 100) * (bound_max - bound_min) + bound_min
            got = enjoy.sliderState(positions, bound_min, bound_max)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
            full_want = np.zeros(dim + 2)
            full_want[1:1 + dim] = want
            full = enjoy.fullState(dim + 2, 1, 1 + dim, got)
            assert full.dtype == np.float64 and full.tobytes() == full_want.tobytes()
    lo, hi = np.array([-1.0]), np.array([2.0])
    assert enjoy.sliderState([0], lo, hi)[0] == -1.0 and enjoy.sliderState([100], lo, hi)[0] == 2.0


def test_traversal_states(enjoy):
    bound_min, bound_max = np.array([0.0, -2.0]), np.array([1.0, 2.0])
    positions = np.round(np.linspace(0, 100, 3)).astype(int)
    assert list(positions) == [0, 50, 100]
    full, block = enjoy.traversalStates(5, 2, 4, bound_min, bound_max, positions)
    assert full.shape == (6, 5) and block.shape == (6, 2)
    assert np.array_equal(block, [[0, 0], [0.5, 0], [1, 0], [0.5, -2], [0.5, 0], [0.5, 2]])
    assert np.array_equal(full[:, 2:4], block) and not full[:, [0, 1, 4]].any()


def test_figure_names(enjoy):
    assert [enjoy.figureName(n) for n in ("autoencoder", "vae", "dae")] == ["Decoder for autoencoder", "Decoder for vae", "Decoder for dae"]
    assert [enjoy.figureName(n) for n in ("inverse", "reward-prior", "random")] == ["KNN on inverse", "KNN on reward-prior", "KNN on random"]
    assert enjoy.knnImagePath(["a/record_000/frame000001.jpg", "a/record_000/frame000002"], 0) == "data/a/record_000/frame000001.jpg"
    assert enjoy.knnImagePath(["a/record_000/frame000001.jpg", "a/record_000/frame000002"], 1) == "data/a/record_000/frame000002.jpg"


def test_knn_needs_five_rows(enjoy):
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit, but n_neighbors = 5, n_samples_fit = 3, n_samples = 1"):
        enjoy.knnImageIndex(np.zeros((3, 2)), np.zeros(2))


def test_host_sheet_layout(enjoy):
    images = [np.full((2, 3, 3), v, dtype=np.uint8) for v in (10, 20, 30)]
    sheet = enjoy.hostSheet(images, cols=2, gap=1, fill=255)
    assert sheet.shape == (2 * 2 + 3, 2 * 3 + 3, 3)
    assert (sheet[1:3, 1:4] == 10).all() and (sheet[1:3, 5:8] == 20).all() and (sheet[4:6, 1:4] == 30).all()
    assert (sheet[4:6, 5:8] == 255).all() and (sheet == 255).sum() == sheet.size - 3 * 18
    with pytest.raises(ValueError):
        enjoy.hostSheet([images[0], np.zeros((3, 3, 3), dtype=np.uint8)], cols=2)


def test_main_without_cv2_and_without_sheet_dir_exits_1(enjoy, no_cv2, capsys):
    with pytest.raises(SystemExit) as e:
        enjoy.main(["--log-dir", "logs/nowhere/"])
    assert e.value.code == 1
    out = capsys.readouterr().out
    assert "--sheet-dir" in out and "cv2" in out and len(out.strip().splitlines()) == 1


def test_command_line(enjoy):
    args = enjoy.build_parser().parse_args(["--log-dir", "x/"])
    assert (args.log_dir, args.no_cuda, args.batchnorm, args.sheet_dir, args.steps, args.cols) == ("x/", False, "reference", None, 11, None)
    args = enjoy.build_parser().parse_args(["--no-cuda", "--batchnorm", "running", "--sheet-dir", "out", "--steps", "3", "--cols", "2"])
    assert (args.no_cuda, args.batchnorm, args.sheet_dir, args.steps, args.cols) == (True, "running", "out", 3, 2)
    with pytest.raises(SystemExit):
        enjoy.build_parser().parse_args(["--batchnorm", "eval"])


def test_new_symbols_are_bound(cabi):
    assert "srlz_decoded_to_bgr" in cabi.EXPORTED and "srlz_decoded_to_sheet_u8" in cabi.EXPORTED
    assert callable(cabi.decoded_to_bgr) and callable(cabi.decoded_to_sheet_u8)


def test_rejections_need_no_gpu(cabi):
    """Every check comes before any launch: the statuses are returned on a machine without a GPU too."""
    import ctypes
    lib = cabi._lib
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected on the host
    assert lib.srlz_decoded_to_bgr(p, 0, 4, 4, p, None) == -1
    assert lib.srlz_decoded_to_bgr(None, 1, 4, 4, p, None) == -4
    assert lib.srlz_decoded_to_bgr(p, 1, 4, 4, None, None) == -4
    assert lib.srlz_decoded_to_bgr(p, 1 << 15, 1 << 8, 1 << 8, p, None) == -1  # 3 * 2^31 floats
    assert lib.srlz_decoded_to_sheet_u8(p, 2, 4, 4, 2, 1, 256, 1, p, 6, 11, None) == -1
    assert lib.srlz_decoded_to_sheet_u8(p, 2, 4, 4, 2, 1, 255, 1, p, 6, 12, None) == -1
    assert "inconsistent sheet size" in cabi.error_text()
    assert lib.srlz_decoded_to_sheet_u8(p, 2, 4, 4, 0, 1, 255, 1, p, 6, 11, None) == -1
    assert lib.srlz_decoded_to_sheet_u8(p, 2, 4, 4, 2, -1, 255, 1, p, 6, 11, None) == -1
    assert lib.srlz_decoded_to_sheet_u8(p, 2, 4, 4, 2, 1, 255, 1, None, 6, 11, None) == -4
    # the 2^31 limit of the sheet by arithmetic on the descriptor: 16 pictures of 1 x 1 with a gap of 6700 in one row are
    # (2 * 6700 + 1) x (17 * 6700 + 16) x 3 = 4.58e9 bytes, while the decoded tensor is 48 floats
    sh, sw = 2 * 6700 + 1, 17 * 6700 + 16
    assert sh * sw * 3 >= 2 ** 31 and 16 * 3 < 2 ** 31
    assert lib.srlz_decoded_to_sheet_u8(p, 16, 1, 1, 16, 6700, 255, 1, p, sh, sw, None) == -1
    assert "2^31" in cabi.error_text()
