"""The supervised baseline on the host side (no GPU): the numpy train / validation split against sklearn's recorded index arrays, the
ragged minibatch list and shuffled order of SupervisedDataLoader, the seeded initial parameters of CustomCNN and DenseNetwork against
the reference's (tools/make_golden_supervised.py), the command line, and the loud rejections."""
import numpy as np
import pytest
import torch

import golden_util as gu
from supervised_util import STATE_DIM


def _sup():
    import srl_baselines.supervised as sup
    return sup


def test_numpy_split_equals_sklearn_train_test_split():
    g = gu.load("sup_split")
    assert list(g["sizes"]) == [3, 10, 52, 78, 101] and list(g["seeds"]) == [0, 1, 7]
    for n in g["sizes"]:
        for seed in g["seeds"]:
            train, val = _sup().trainValSplit(int(n), int(seed))
            np.testing.assert_array_equal(train, g["n%d/seed%d/train" % (n, seed)])
            np.testing.assert_array_equal(val, g["n%d/seed%d/val" % (n, seed)])
            assert len(val) == int(np.ceil(0.33 * n)) and len(train) + len(val) == n


@pytest.mark.parametrize("n,bs,sizes", [(52, 8, [8] * 6 + [4]), (26, 16, [16, 10]), (16, 8, [8, 8]), (3, 8, [3]), (9, 1, [1] * 9)])
def test_minibatch_list_is_ragged_and_drops_empty_slices(n, bs, sizes):
    from preprocessing.data_loader import SupervisedDataLoader
    x = np.arange(100, 100 + n)
    y = np.arange(2 * n, dtype=np.float32).reshape(n, 2)
    mbs, targets = SupervisedDataLoader.createMinibatchList(x, y, bs)
    assert [len(m) for m in mbs] == sizes == [len(t) for t in targets]
    np.testing.assert_array_equal(np.concatenate(mbs), x)
    np.testing.assert_array_equal(np.concatenate(targets), y)


def test_shuffled_order_follows_numpy_permutation():
    """One np.random.permutation(n_minibatches) per epoch from the global state (reference data_loader.py:315-316); in order otherwise.
    The loader is built without starting its producer process."""
    from preprocessing.data_loader import SupervisedDataLoader
    x = np.arange(52)
    for shuffle in (True, False):
        loader = SupervisedDataLoader.__new__(SupervisedDataLoader)
        loader.minibatchlist, _ = SupervisedDataLoader.createMinibatchList(x, x, 8)
        loader.n_minibatches, loader.shuffle, loader._order_rng = len(loader.minibatchlist), shuffle, None
        loader.rank, loader.world_size, loader.val_indices = 0, 1, None
        np.random.seed(5)
        got = [loader._epochOrder() for _ in range(2)]
        np.random.seed(5)
        want = [np.random.permutation(7) for _ in range(2)] if shuffle else [np.arange(7)] * 2
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
            assert a.dtype == np.int64


def _build(kind, seed=1):
    from models import DenseNetwork, CustomCNN
    from preprocessing.preprocess import getInputDim
    np.random.seed(seed)
    torch.manual_seed(seed)
    return CustomCNN(STATE_DIM) if kind == "cnn" else DenseNetwork(getInputDim(), STATE_DIM)


@pytest.mark.parametrize("kind", ["cnn", "mlp"])
def test_seeded_construction_reproduces_reference_init(kind):
    g = gu.load("init_sup_" + kind)
    sd = _build(kind).state_dict()
    assert list(sd.keys()) == [str(n) for n in g["names"]]
    for i, (k, v) in enumerate(sd.items()):
        assert str(list(v.shape)).replace(" ", "") == str(g["shapes"][i]).replace(" ", ""), k
        assert abs(float(v.double().sum()) - g["sums"][i]) <= 1e-9 * max(1.0, g["abss"][i]), k
        assert abs(float(v.double().abs().sum()) - g["abss"][i]) <= 1e-9 * max(1.0, g["abss"][i]), k


def test_dense_network_surface():
    from models import DenseNetwork
    m = DenseNetwork(3 * 224 * 224, state_dim=5)
    assert list(m.state_dict().keys()) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert m.fc1.weight.shape == (64, 150528) and m.fc2.weight.shape == (5, 64) and m.drop_p == 0.5
    with pytest.raises(RuntimeError, match="no CPU"):  # there is no CPU fallback
        m(torch.zeros(1, 3, 224, 224))


def test_command_line_is_the_references():
    sup = _sup()
    a = sup.buildParser().parse_args(["--data-folder", "data/some_set/"])
    assert (a.epochs, a.seed, a.batch_size, a.learning_rate, a.no_cuda, a.no_display_plots, a.model_type, a.data_folder,
            a.training_set_size, a.relative_pos, a.log_folder) == (50, 1, 32, 0.005, False, False, "resnet", "data/some_set/", -1,
                                                                   False, "")
    a = sup.buildParser().parse_args(["--epochs", "3", "--seed", "7", "-bs", "16", "-lr", "0.01", "--no-cuda", "--no-display-plots",
                                      "--model-type", "custom_cnn", "--data-folder", "d", "--training-set-size", "40", "--relative-pos",
                                      "--log-folder", "logs/x"])
    assert (a.epochs, a.seed, a.batch_size, a.learning_rate, a.no_cuda, a.no_display_plots, a.model_type, a.training_set_size,
            a.relative_pos, a.log_folder) == (3, 7, 16, 0.01, True, True, "custom_cnn", 40, True, "logs/x")
    assert sup.getModelName(a) == "supervised_custom_cnn_SEED7_EPOCHS3_BS16"
    with pytest.raises(SystemExit):
        sup.buildParser().parse_args([])  # --data-folder is required
    assert (sup.DISPLAY_PLOTS, sup.EPOCH_FLAG, sup.BATCH_SIZE, sup.TEST_BATCH_SIZE) == (True, 1, 32, 256) and sup.N_EPOCHS > 0
    assert sup.SHUFFLE_MINIBATCHES is False  # the reference's loader resets its shuffle flag: it trains in order


def test_unsupported_models_are_rejected_before_anything_runs():
    sup = _sup()
    with pytest.raises(NotImplementedError, match="ResNet-18.*outside this build"):
        sup.SupervisedLearning(3, model_type="resnet", cuda=True)
    with pytest.raises(NotImplementedError):
        sup.SupervisedLearning(3, cuda=True)  # the reference's default model
    with pytest.raises(ValueError, match="Unknown model: foo"):
        sup.SupervisedLearning(3, model_type="foo", cuda=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sup.SupervisedLearning(3, model_type="mlp", cuda=False)


def test_mse_target_and_dropout_reject_bad_arguments_host_side(cabi):
    """Null pointers, zero sizes and B * S above 2^20 never reach a launch: a status code and an error text (no GPU needed)."""
    import ctypes
    p = ctypes.c_void_p(4096)  # never dereferenced: every case below is refused before the launch
    for args, text in (((None, p, 1, 1, p, p, None), "null"), ((p, p, 0, 1, p, p, None), "B = 0"), ((p, p, 1, 0, p, p, None), "S = 0"),
                       ((p, p, 1025, 1024, p, p, None), "exceeds"), ((p, p, 1 << 20, 2, p, p, None), "exceeds"),
                       ((ctypes.c_void_p(4100), p, 1, 1, p, p, None), "aligned")):
        with pytest.raises(cabi.SrlzError, match=text):
            cabi.mse_target_fwd(*args)
    for fn in (cabi.dropout_fwd, cabi.dropout_bwd):
        for args, text in (((p, None, 0.5, p, 1, 1, None), "null"), ((p, p, 0.5, p, 0, 1, None), "rows = 0"),
                           ((p, p, 0.0, p, 1, 1, None), "keep"), ((p, p, 1.5, p, 1, 1, None), "keep")):
            with pytest.raises(cabi.SrlzError, match=text):
                fn(*args)
