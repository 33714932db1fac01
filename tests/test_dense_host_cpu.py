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


# (M, n, plane, C, Z): the smallest shapes at which each edge of the tile kernel exists (K = C * plane), with the number Z of split-K
# partials that in_split() of csrc/dense.hip takes there.  test_dense_entry_gpu.py runs the kernels at exactly these.
#   1 x 1, K 3          everything at its minimum
#   7 x 50, K 105       channel boundaries at k = 35, 70 inside the first tile and r-steps; last chunk 9 long
#   33 x 63, K 126      six planes (the channel wraps 0,1,2,0,1,2); the ones column is lane 63 of tile 0; M = one r-step + 1
#   64 x 64, K 384      every edge exact; the ones column opens a tile of its own
#   65 x 65, K 8223     four output tiles, two r-steps per chunk (rchunk 64), last chunk 31 long; a row and a column behind a full tile
#   130 x 256, K 33     n at its limit; K = one r-step + 1; three i-tiles, the last of 2 rows; the ones column alone in a fifth tile
#   96 x 200, K 600     M = exactly three r-steps as the reduction
DENSE_EDGE_SHAPES = [(1, 1, 1, 3, 1), (7, 50, 35, 3, 4), (33, 63, 21, 6, 4), (64, 64, 64, 6, 12), (65, 65, 2741, 3, 129),
                     (130, 256, 11, 3, 2), (96, 200, 100, 6, 19)]


def replay_in_split(M, n, K):
    """in_split() / rchunk_for() of csrc/dense.hip: (Z, rchunk)."""
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731
    tiles = cdiv(M, 64) * cdiv(n, 64)
    want = 1 if tiles >= 1024 else cdiv(1024, tiles)
    steps = cdiv(K, 32)
    rchunk = cdiv(steps, min(want, steps)) * 32
    return cdiv(K, rchunk), rchunk


def assert_dense_split_table(cabi, M, n, plane, C, Z):
    """The queries of the library against the table (and against the replay): a case written for Z partials cannot test another split."""
    K = C * plane
    assert cabi.dense_supported(M, n, K, plane) == 1
    assert replay_in_split(M, n, K)[0] == Z
    assert cabi.dense_in_workspace(M, n, K) == Z * M * n * 4
    assert cabi.dense_out_bwd_workspace(M, n, K) == Z * M * n * 4 + M * K * 4
    assert cabi.dense_out_fwd_loss_workgroups(M, K) == ((M + 63) // 64) * ((K + 63) // 64)


@pytest.mark.parametrize("M,n,plane,C,Z", DENSE_EDGE_SHAPES)
def test_dense_split_of_the_edge_shapes(cabi, M, n, plane, C, Z):
    assert_dense_split_table(cabi, M, n, plane, C, Z)


def test_dense_edge_shapes_reach_what_they_are_listed_for():
    rc = {s[:2]: replay_in_split(s[0], s[1], s[2] * s[3])[1] for s in DENSE_EDGE_SHAPES}
    assert rc[(65, 65)] == 64 and 8223 % 64 == 31            # two r-steps per chunk, a short last chunk
    assert rc[(7, 50)] == 32 and 105 % 32 == 9
    assert all(v == 32 for k, v in rc.items() if k != (65, 65))
    assert replay_in_split(512, 50, 3 * 224 * 224) == (128, 1184)  # the workload's split, for comparison


def test_dense_supported_at_the_32_bit_edges(cabi):
    """Every offset of the kernels is a 32-bit int: M * K, (n + 1) * K (W with the ones column) and Z * M * n must stay below 2^31."""
    ok = cabi.dense_supported
    # M * K: K = 3 (one pixel per plane), Z = 1, n = 1
    assert 715827882 * 3 < 2 ** 31 <= 715827883 * 3
    assert ok(715827882, 1, 3, 1) == 1
    assert ok(715827883, 1, 3, 1) == 0 and "32-bit" in cabi.error_text()
    # (n + 1) * K at n = 256
    assert 257 * 8355966 < 2 ** 31 <= 257 * 8355969
    assert ok(1, 256, 8355966, 2785322) == 1
    assert ok(1, 256, 8355969, 2785323) == 0 and "32-bit" in cabi.error_text()
    # Z * M * n: Z = 1 at K = 3, M * n = 2^31 - 4 and 2^31 while M * K stays below
    assert replay_in_split(536870911, 4, 3)[0] == 1 and 536870912 * 3 < 2 ** 31
    assert ok(536870911, 4, 3, 1) == 1
    assert ok(536870912, 4, 3, 1) == 0 and "split-K" in cabi.error_text()
    # the workspace queries answer 0 to a shape that is none
    assert cabi.dense_in_workspace(0, 4, 3) == 0 and cabi.dense_out_bwd_workspace(4, 0, 3) == 0
    assert cabi.dense_out_fwd_loss_workgroups(0, 3) == -1 and cabi.dense_out_fwd_loss_workgroups(4, 0) == -1
