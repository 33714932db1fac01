"""--model-type mlp / linear on the host side (no GPU): seeded construction against the reference's initial parameters, the selection
table of SRLModules (reference models/modules.py:42-73) and its loud rejections, and the shape predicate every dense launcher checks
(csrc/dense.hip, srlz_dense_supported).  The flat index of the uint8 frames is held on the GPU (test_dense_kernels_gpu.py)."""
import numpy as np
import pytest
import torch

import golden_util as gu


def build(model_type, losses, C=3, S=200, A=6, seed=1):
    import preprocessing.preprocess as pre
    from models.modules import SRLModules
    pre.N_CHANNELS = C
    np.random.seed(seed)
    torch.manual_seed(seed)
    try:
        return SRLModules(state_dim=S, action_dim=A, cuda=False, model_type=model_type, losses=losses)
    finally:
        pre.N_CHANNELS = 3


@pytest.mark.parametrize("tag,model_type,losses,C", [
    ("mlp_ae_c3", "mlp", ["autoencoder"], 3), ("mlp_vae_c3", "mlp", ["vae"], 3), ("mlp_net_c3", "mlp", ["inverse", "forward"], 3),
    ("linear_ae_c3", "linear", ["autoencoder"], 3), ("linear_net_c3", "linear", ["inverse", "forward"], 3),
    ("mlp_ae_c6", "mlp", ["autoencoder"], 6)])
def test_seeded_dense_construction_reproduces_reference_init(tag, model_type, losses, C):
    """Heads, then the conv stacks of BaseModelAutoEncoder (built, never run), then the dense layers: the reference's RNG order, names,
    shapes and values."""
    g = gu.load("init_" + tag)
    sd = build(model_type, losses, C=C).state_dict()
    assert list(sd.keys()) == [str(n) for n in g["names"]]
    for i, (k, v) in enumerate(sd.items()):
        assert str(list(v.shape)).replace(" ", "") == str(g["shapes"][i]).replace(" ", ""), k
        assert abs(float(v.double().sum()) - g["sums"][i]) <= 1e-9 * max(1.0, g["abss"][i]), k
        assert abs(float(v.double().abs().sum()) - g["abss"][i]) <= 1e-9 * max(1.0, g["abss"][i]), k


@pytest.mark.parametrize("model_type,losses,cls", [
    ("mlp", ["autoencoder"], "DenseAutoEncoder"), ("mlp", ["dae"], "DenseAutoEncoder"), ("mlp", ["autoencoder", "inverse"], "DenseAutoEncoder"),
    ("mlp", ["vae"], "DenseVAE"), ("mlp", ["vae", "forward"], "DenseVAE"), ("mlp", ["inverse"], "SRLDenseNetwork"),
    ("mlp", ["forward", "reward"], "SRLDenseNetwork"), ("linear", ["autoencoder"], "LinearAutoEncoder"),
    ("linear", ["dae", "inverse"], "LinearAutoEncoder"), ("linear", ["inverse", "forward"], "SRLLinear"),
    ("linear", ["reward"], "SRLLinear")])
def test_selection_table(model_type, losses, cls):
    m = build(model_type, losses, S=8)
    assert type(m.model).__name__ == cls
    assert m.model.__class__.__module__.split(".")[-1] == {"DenseAutoEncoder": "autoencoders", "LinearAutoEncoder": "autoencoders",
                                                           "DenseVAE": "vae", "SRLDenseNetwork": "priors", "SRLLinear": "priors"}[cls]


def test_input_dim_follows_the_channels():
    assert build("mlp", ["autoencoder"], C=6, S=8).model.encoder[0].weight.shape == (50, 301056)
    assert build("linear", ["inverse"], C=3, S=8).model.fc.weight.shape == (8, 150528)
    assert build("mlp", ["vae"], C=6, S=8).model.decoder[4].weight.shape == (301056, 50)


def test_unsupported_dense_combinations_are_rejected_loudly():
    from collections import OrderedDict
    from models.modules import SRLModulesSplit
    for mt, losses in (("linear", ["vae"]), ("mlp", ["vae", "perceptual"]), ("linear", ["autoencoder", "perceptual"]),
                       ("mlp", ["inverse", "triplet"]), ("linear", ["triplet"])):
        with pytest.raises(NotImplementedError):
            build(mt, losses, S=8)
    for mt in ("mlp", "linear"):
        with pytest.raises(NotImplementedError):
            SRLModulesSplit(state_dim=8, model_type=mt, losses=["autoencoder", "inverse"],
                            split_dimensions=OrderedDict([("autoencoder", 4), ("inverse", 4)]))


def test_dense_launcher_shape_predicate(cabi):
    P = 224 * 224
    ok = cabi.dense_supported
    assert ok(1, 50, 3 * P, P) == 1          # M = 1
    assert ok(7, 2, 3 * P, P) == 1           # odd M
    assert ok(1024, 200, 6 * P, P) == 1      # K of six channels
    assert ok(512, 256, 3 * P, P) == 1
    assert ok(0, 50, 3 * P, P) == 0 and "M = 0" in cabi.error_text()
    assert ok(4, 257, 3 * P, P) == 0         # n beyond the tiles' 256
    assert ok(4, 50, 3 * P + 1, P) == 0      # K not whole planes
    assert ok(4, 50, 9 * P, P) == 0          # nine channels: not a dense model's input
    # past the 32-bit offsets: M * K >= 2^31
    assert ok(7200, 50, 6 * P, P) == 0 and "32-bit" in cabi.error_text()
    assert ok(7100, 50, 6 * P, P) == 1
    assert cabi.dense_in_workspace(512, 50, 3 * P) > 0
    assert cabi.dense_out_bwd_workspace(512, 50, 3 * P) >= 512 * 3 * P * 4
    assert cabi.dense_out_fwd_loss_workgroups(512, 3 * P) == 8 * (3 * P // 64)
