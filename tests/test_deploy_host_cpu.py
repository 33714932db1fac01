"""The deployment encoder on the host side (no GPU): the descriptor predicate of csrc/infer.hip and its pooled sizes, the route table
of srlz.deploy by model class, the loud rejections of a call's frames, and the constructor without a GPU."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import deploy_util as du
from test_dense_host_cpu import build


def _nhwc(hi, wi):
    return (hi * wi * 64, 1, wi * 64, 64)


def test_supported_accepts_and_rejects_the_right_descriptors():
    from srlz import ops
    ok = [ops.infer_desc(0, 1, 3, 224, 224), ops.infer_desc(0, 32, 6, 224, 224), ops.infer_desc(1, 4, 64, 56, 56),
          ops.infer_desc(2, 4, 64, 27, 27), ops.infer_desc(0, 2, 3, 20, 12, strides=(12 * 20 * 3, 1, 3, 20 * 3)),  # camera frames
          ops.infer_desc(1, 1, 64, 3, 3), ops.infer_desc(2, 1, 64, 5, 5), ops.infer_desc(0, 1, 3, 1, 1),  # pooled 1 x 1
          ops.infer_desc(2, 2, 64, 27, 27, pool_pad=1, out_nchw=False)]
    for d in ok:
        assert ops.infer_supported(d), (d.kind, d.c_in, d.hi, d.wi)
    bad = [ops.infer_desc(0, 1, 4, 224, 224), ops.infer_desc(0, 1, 9, 224, 224), ops.infer_desc(0, 1, 64, 224, 224),  # c_in of "in"
           ops.infer_desc(1, 1, 3, 56, 56), ops.infer_desc(2, 1, 32, 27, 27),                                          # c_in of a 64-channel kind
           ops.infer_desc(1, 1, 64, 2, 56), ops.infer_desc(1, 1, 64, 56, 2), ops.infer_desc(2, 1, 64, 4, 27),           # pooled size < 1
           ops.infer_desc(0, 1, 3, 224, 224, pool_pad=0, strides=(1, 1, 1, 1)),                                         # elements share a byte
           ops.infer_desc(0, 2, 3, 20, 12, strides=(100, 1, 3, 60)),                                                    # frames overlap
           ops.infer_desc(0, 1, 3, 20, 12, strides=(720, 0, 3, 60)),                                                    # a zero stride
           ops.infer_desc(1, 1, 64, 9, 9, strides=(9 * 9 * 64, 1, 9 * 64, 32)),                                         # not NHWC
           ops.infer_desc(1, 1, 64, 9, 9, strides=(9 * 9 * 64, 9 * 9, 9, 1)),                                           # planar floats
           ops.infer_desc(3, 1, 64, 9, 9), ops.infer_desc(1, 0, 64, 9, 9), ops.infer_desc(1, 1, 64, 9, 9, pool_pad=2)]
    for d in bad:
        assert not ops.infer_supported(d), (d.kind, d.c_in, d.hi, d.wi)
        with pytest.raises(Exception) as e:
            ops.infer_out_dims(d)
        assert "infer_block" in str(e.value)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_pooled_sizes_follow_the_floor_formula(kind):
    from srlz import ops
    k, s, p = du.GEO[kind]
    c = 3 if kind == 0 else 64
    seen = 0
    for hi in range(1, 40):
        for wi in (hi, 2 * hi + 1, 224):
            for pp in (0, 1):
                hc, wc = (hi + 2 * p - k) // s + 1, (wi + 2 * p - k) // s + 1
                hp, wp = (hc + 2 * pp - 3) // 2 + 1, (wc + 2 * pp - 3) // 2 + 1
                d = ops.infer_desc(kind, 2, c, hi, wi, pool_pad=pp)
                if hi + 2 * p < k or wi + 2 * p < k or hc + 2 * pp < 3 or wc + 2 * pp < 3:
                    assert not ops.infer_supported(d)
                    continue
                assert ops.infer_supported(d) and ops.infer_out_dims(d) == (hc, wc, hp, wp), (kind, hi, wi, pp)
                assert (hc, wc, hp, wp) == du.out_dims(kind, hi, wi, pp)
                seen += 1
    assert seen > 150
    # the reference's chain at 224 x 224: 112 -> 56 -> 56 -> 27 -> 14 -> 6 (models/models.py:47-63)
    assert ops.infer_out_dims(ops.infer_desc(0, 1, 3, 224, 224)) == (112, 112, 56, 56)
    assert ops.infer_out_dims(ops.infer_desc(1, 1, 64, 56, 56)) == (56, 56, 27, 27)
    assert ops.infer_out_dims(ops.infer_desc(2, 1, 64, 27, 27)) == (14, 14, 6, 6)


def test_tile_and_packed_sizes(cabi):
    assert cabi.infer_tile() >= 1
    assert cabi.infer_packed_floats(0, 3) == 64 * 160 and cabi.infer_packed_floats(0, 6) == 64 * 304  # K = 49 C in whole groups of 16
    assert cabi.infer_packed_floats(1, 64) == cabi.infer_packed_floats(2, 64) == 64 * 576
    assert cabi.infer_packed_floats(0, 4) == 0 and cabi.infer_packed_floats(1, 3) == 0 and cabi.infer_packed_floats(5, 64) == 0


def _split():
    import preprocessing.preprocess as pre
    from models.modules import SRLModulesSplit
    pre.N_CHANNELS = 3
    torch.manual_seed(1)
    return SRLModulesSplit(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=["autoencoder", "inverse"],
                           split_dimensions=OrderedDict([("autoencoder", 4), ("inverse", 4)]))


def test_route_table_by_model_class():
    from srlz import deploy
    table = [("custom_cnn", ["inverse"], "CustomCNN", "blocks"), ("custom_cnn", ["autoencoder"], "CNNAutoEncoder", "blocks"),
             ("custom_cnn", ["dae", "inverse"], "CNNAutoEncoder", "blocks"), ("custom_cnn", ["vae"], "CNNVAE", "blocks"),
             ("mlp", ["autoencoder"], "DenseAutoEncoder", "model"), ("mlp", ["vae"], "DenseVAE", "model"),
             ("mlp", ["inverse"], "SRLDenseNetwork", "model"), ("linear", ["autoencoder"], "LinearAutoEncoder", "model"),
             ("linear", ["inverse"], "SRLLinear", "model")]
    for model_type, losses, cls, route in table:
        m = build(model_type, losses, S=8)
        assert type(m.model).__name__ == cls
        assert deploy.route_for(m) == route, (model_type, losses)
        assert deploy.route_for(m.model) == route, (model_type, losses)  # the bare network
    m = _split()
    assert deploy.route_for(m) == "blocks"
    # the head is the layer getStates ends in: encoder_fc (AE), encoder_fc1 = mu (VAE), fc (CustomCNN)
    ae, vae, cnn = build("custom_cnn", ["autoencoder"], S=8), build("custom_cnn", ["vae"], S=8), build("custom_cnn", ["inverse"], S=8)
    assert deploy.encoder_parts(ae)[1] is ae.model.encoder_fc[0] and deploy.encoder_parts(ae)[0] is ae.model.encoder_conv
    assert deploy.encoder_parts(vae)[1] is vae.model.encoder_fc1
    assert deploy.encoder_parts(cnn)[1] is cnn.model.fc and deploy.encoder_parts(cnn)[0] is cnn.model.conv_layers
    assert deploy.encoder_parts(build("mlp", ["autoencoder"], S=8)) is None  # (it owns a conv stack, which never runs)


def test_triplet_embedding_net_takes_the_model_route():
    from srlz import deploy
    from models.triplet import EmbeddingNet
    assert deploy.encoder_parts(EmbeddingNet.__new__(EmbeddingNet)) is None


def test_bad_layout_dtype_and_channels_raise_value_error():
    from srlz import deploy
    fr = np.zeros((2, 224, 224, 3), np.uint8)
    assert deploy.check_frames(fr, "nhwc", 3, (224, 224)) == (2, False)
    assert deploy.check_frames(fr[0], "nhwc", 3, (224, 224)) == (1, True)
    assert deploy.check_frames(torch.zeros((4, 6, 224, 224), dtype=torch.uint8), "planar", 6) == (4, False)
    with pytest.raises(ValueError, match="frame_layout"):
        deploy.check_frames(fr, "nchw", 3)
    with pytest.raises(ValueError, match="frame_layout"):
        deploy.StateEncoder(build("custom_cnn", ["inverse"], S=3), frame_layout="hwc")  # judged before anything touches a GPU
    with pytest.raises(ValueError, match="uint8"):
        deploy.check_frames(fr.astype(np.float32), "nhwc", 3)
    with pytest.raises(ValueError, match="uint8"):
        deploy.check_frames(torch.zeros((1, 224, 224, 3)), "nhwc", 3)
    with pytest.raises(ValueError, match="channels"):
        deploy.check_frames(fr, "nhwc", 6)
    with pytest.raises(ValueError, match="channels"):
        deploy.check_frames(fr, "planar", 3)  # the stated layout decides what the axes mean: never guessed from the shape
    with pytest.raises(ValueError, match="shape"):
        deploy.check_frames(fr[0, 0], "nhwc", 3)
    with pytest.raises(ValueError, match="built for"):
        deploy.check_frames(np.zeros((1, 200, 224, 3), np.uint8), "nhwc", 3, (224, 224))


def test_constructor_without_a_gpu_raises_the_product_message(monkeypatch):
    from srlz import deploy
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (so the test says the same on a machine that has one)
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.StateEncoder(build("custom_cnn", ["inverse"], S=3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.StateEncoder.from_log_folder("logs/none/")
