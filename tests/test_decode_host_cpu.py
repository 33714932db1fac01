"""The deployment decoder on the host side (no GPU): the descriptor predicate of csrc/infer_dec.hip and its output sizes, every
rejection, the route table of srlz.deploy.FrameDecoder by model class, the loud rejections of a call's states, the constructor without
a GPU — and the fp64 restatement of decode_util against the golden lattice and plane sums recorded from the unmodified reference
(tests/golden/decode_kats.npz), which is what lets the GPU tests trust the restatement for the full image."""
import json
import os

import numpy as np
import pytest
import torch

import decode_util as dd
import deploy_util as du
import golden_util as gu
from test_dense_host_cpu import build

FIRST, MID, OUT = 0, 1, 2


def test_supported_accepts_the_decoder_chain_and_both_byte_layouts():
    from srlz import ops
    ok = [ops.infer_dec_desc(FIRST, 1, 6, 6), ops.infer_dec_desc(MID, 32, 13, 13), ops.infer_dec_desc(MID, 4, 27, 27),
          ops.infer_dec_desc(MID, 1, 55, 55), ops.infer_dec_desc(OUT, 1, 111, 111), ops.infer_dec_desc(OUT, 2, 111, 111, c_out=6),
          ops.infer_dec_desc(FIRST, 3, 1, 1), ops.infer_dec_desc(MID, 1, 3, 2), ops.infer_dec_desc(OUT, 1, 1, 1),
          ops.infer_dec_desc(OUT, 2, 111, 111, out_u8=True),                                                     # planar bytes
          ops.infer_dec_desc(OUT, 2, 111, 111, out_u8=True, bgr=True, out_strides=(224 * 224 * 3, 1, 3, 224 * 3)),  # camera frames
          ops.infer_dec_desc(OUT, 1, 5, 7, c_out=6, out_u8=True, out_strides=(12 * 16 * 6, 1, 6, 12 * 6)),
          ops.infer_dec_desc(OUT, 1, 5, 7, out_u8=True, out_strides=(1, 12 * 16, 16, 1))]  # (n = 1: its stride is never stepped along)
    for d in ok:
        assert ops.infer_dec_supported(d), (d.kind, d.c_out, d.hi, d.wi)


def test_every_rejection_is_said_by_the_predicate_and_raised_by_out_dims():
    from srlz import ops
    bad = [ops.infer_dec_desc(3, 1, 6, 6), ops.infer_dec_desc(-1, 1, 6, 6),                                  # unknown kind
           ops.infer_dec_desc(MID, 1, 6, 6, c_in=32), ops.infer_dec_desc(OUT, 1, 6, 6, c_in=3),              # c_in != 64
           ops.infer_dec_desc(MID, 1, 6, 6, c_out=3), ops.infer_dec_desc(FIRST, 1, 6, 6, c_out=32),          # c_out of a block
           ops.infer_dec_desc(OUT, 1, 6, 6, c_out=64), ops.infer_dec_desc(OUT, 1, 6, 6, c_out=4),            # c_out of the out layer
           ops.infer_dec_desc(MID, 0, 6, 6), ops.infer_dec_desc(MID, 1, 0, 6), ops.infer_dec_desc(OUT, 1, 6, 0),  # empty
           ops.infer_dec_desc(FIRST, 1, 6, 6, in_strides=(6 * 6 * 64, 1, 6 * 64, 64)),                       # first reads [N,64,hi,wi]
           ops.infer_dec_desc(MID, 1, 6, 6, in_strides=(64 * 36, 36, 6, 1)),                                 # mid reads NHWC
           ops.infer_dec_desc(OUT, 1, 6, 6, in_strides=(6 * 6 * 64, 1, 6 * 64, 32)),
           ops.infer_dec_desc(OUT, 1, 5, 7, out_u8=True, out_strides=(1, 1, 1, 1)),                          # elements share a byte
           ops.infer_dec_desc(OUT, 2, 5, 7, out_u8=True, out_strides=(100, 12 * 16, 16, 1)),                 # frames overlap
           ops.infer_dec_desc(OUT, 1, 5, 7, out_u8=True, out_strides=(576, 0, 16, 1)),                       # a zero stride
           ops.infer_dec_desc(OUT, 1, 5, 7, out_u8=True, out_strides=(576, 1, 3, 35)),                       # nhwc rows too short
           ops.infer_dec_desc(MID, 1, 6, 6, out_u8=True),                                                    # bytes from a block
           ops.infer_dec_desc(MID, 1, 1 << 30, 6),                                                           # counts beyond 2^31 - 1
           ops.infer_dec_desc(MID, 1 << 30, 1 << 10, 1 << 10),
           ops.infer_dec_desc(OUT, 1, 20000, 20000, out_u8=True)]
    for d in bad:
        assert not ops.infer_dec_supported(d), (d.kind, d.c_in, d.c_out, d.hi, d.wi)
        with pytest.raises(Exception) as e:
            ops.infer_dec_out_dims(d)
        assert "infer_dec" in str(e.value)


@pytest.mark.parametrize("kind", [FIRST, MID, OUT])
def test_out_dims_follow_2h_plus_1_and_2h_plus_2(kind):
    from srlz import ops
    add = 2 if kind == OUT else 1
    seen = 0
    for hi in range(1, 40):
        for wi in (hi, 2 * hi + 1, 111):
            d = ops.infer_dec_desc(kind, 2, hi, wi)
            assert ops.infer_dec_supported(d) and ops.infer_dec_out_dims(d) == (2 * hi + add, 2 * wi + add), (kind, hi, wi)
            seen += 1
    assert seen == 117
    # the reference's chain: 6 -> 13 -> 27 -> 55 -> 111 -> 224 (models/models.py:65-83)
    h = 6
    for k in (FIRST, MID, MID, MID, OUT):
        h = ops.infer_dec_out_dims(ops.infer_dec_desc(k, 1, h, h))[0]
    assert h == 224


def test_tile_and_packed_sizes(cabi):
    assert cabi.infer_dec_tile(FIRST) == cabi.infer_dec_tile(MID) >= 1 and cabi.infer_dec_tile(OUT) >= 1 and cabi.infer_dec_tile(7) == 0
    assert cabi.infer_dec_packed_floats(FIRST, 64) == cabi.infer_dec_packed_floats(MID, 64) == 64 * 576
    assert cabi.infer_dec_packed_floats(OUT, 3) >= 64 * 3 * 16 and cabi.infer_dec_packed_floats(OUT, 6) >= 64 * 6 * 16
    assert cabi.infer_dec_packed_floats(MID, 3) == 0 and cabi.infer_dec_packed_floats(OUT, 64) == 0 and cabi.infer_dec_packed_floats(5, 64) == 0


def test_route_table_by_model_class():
    from srlz import deploy
    table = [("custom_cnn", ["autoencoder"], "CNNAutoEncoder", "blocks"), ("custom_cnn", ["dae", "inverse"], "CNNAutoEncoder", "blocks"),
             ("custom_cnn", ["vae"], "CNNVAE", "blocks"), ("mlp", ["autoencoder"], "DenseAutoEncoder", "model"),
             ("mlp", ["vae"], "DenseVAE", "model"), ("linear", ["autoencoder"], "LinearAutoEncoder", "model")]
    for model_type, losses, cls, route in table:
        m = build(model_type, losses, S=8)
        assert type(m.model).__name__ == cls
        assert deploy.decode_route_for(m) == route, (model_type, losses)
        assert deploy.decode_route_for(m.model) == route, (model_type, losses)  # the bare network
    import models.modules as modules
    import preprocessing.preprocess as pre
    assert deploy.decode_route_for(du.build_case("split_ae_inverse", modules, pre)) == "blocks"
    ae = build("custom_cnn", ["autoencoder"], S=8)
    fc, stack = deploy.decoder_parts(ae)
    assert fc is ae.model.decoder_fc[0] and stack is ae.model.decoder_conv
    assert deploy.decoder_parts(build("mlp", ["autoencoder"], S=8)) is None  # (it owns a conv decoder, which never runs)


def test_a_model_without_a_decoder_raises_value_error_naming_the_class():
    from srlz import deploy
    from models.triplet import EmbeddingNet
    for model_type, losses, cls in (("custom_cnn", ["inverse"], "CustomCNN"), ("mlp", ["inverse"], "SRLDenseNetwork"),
                                    ("linear", ["inverse"], "SRLLinear")):
        m = build(model_type, losses, S=8)
        assert type(m.model).__name__ == cls
        for fn in (deploy.decode_route_for, deploy.decoder_parts, deploy.FrameDecoder):  # (judged before anything asks for a GPU)
            with pytest.raises(ValueError, match=cls):
                fn(m)
    with pytest.raises(ValueError, match="EmbeddingNet"):
        deploy.decoder_parts(EmbeddingNet.__new__(EmbeddingNet))


def test_bad_states_raise_value_error():
    from srlz import deploy
    z = np.zeros((2, 8), np.float32)
    assert deploy.check_states(z, 8) == (2, False)
    assert deploy.check_states(z[0], 8) == (1, True)
    assert deploy.check_states(torch.zeros((4, 3), dtype=torch.float64), 3) == (4, False)
    with pytest.raises(ValueError, match="wide"):
        deploy.check_states(z, 3)
    with pytest.raises(ValueError, match="wide"):
        deploy.check_states(z[0], 2)
    with pytest.raises(ValueError, match="floating"):
        deploy.check_states(z.astype(np.int32), 8)
    with pytest.raises(ValueError, match="floating"):
        deploy.check_states(torch.zeros((2, 8), dtype=torch.uint8), 8)
    with pytest.raises(ValueError, match="no state"):
        deploy.check_states(np.zeros((0, 8), np.float32), 8)
    with pytest.raises(ValueError, match="shape"):
        deploy.check_states(np.zeros((1, 2, 8), np.float32), 8)
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        deploy.check_states([[0.0] * 8], 8)
    with pytest.raises(ValueError, match="frame_layout"):
        deploy.FrameDecoder(build("custom_cnn", ["autoencoder"], S=8), frame_layout="hwc")


def test_constructor_without_a_gpu_raises_the_product_message(monkeypatch):
    from srlz import deploy
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (so the test says the same on a machine that has one)
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.FrameDecoder(build("custom_cnn", ["autoencoder"], S=8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.FrameDecoder(build("mlp", ["autoencoder"], S=8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.FrameDecoder.from_log_folder("logs/none/")


def test_byte_expression_rounds_clips_and_orders_channels():
    d = np.zeros((1, 6, 2, 3), np.float32)
    d[0, :, 0, 0] = [np.nan, 50.0, -50.0, 0.0, 0.1, -0.1]
    by = dd.bytes_expr(d)
    assert by.shape == (1, 6, 2, 3) and list(by[0, :3, 0, 0]) == [0, 255, 0]
    one = np.float32(0.0) * dd.STD[0] + dd.MEAN[0]
    assert by[0, 3, 0, 0] == int(np.rint(one * np.float32(255)))
    cam = dd.bytes_expr(d, "nhwc", bgr=True)
    assert cam.shape == (1, 3, 2, 6)
    for c in range(6):
        assert np.array_equal(cam[0, :, :, 3 * (c // 3) + 2 - c % 3], by[0, c].T)


@pytest.mark.parametrize("name", dd.CASES)
def test_fp64_restatement_matches_the_reference_on_the_golden_lattice_and_plane_sums(name):
    """This build's model classes, seeded as the reference's were (checksums), restated in fp64 from the state_dict alone."""
    import models.modules as modules
    import preprocessing.preprocess as pre
    with np.load(os.path.join(gu.GOLDEN_DIR, "decode_kats.npz"), allow_pickle=False) as z:
        kats = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
    with open(os.path.join(gu.GOLDEN_DIR, "decode_spread.json")) as f:
        assert 0.0 < json.load(f)[name] < 1e-5
    model = dd.build_case(name, modules, pre)
    names, sums, abss = du.checksums(model.state_dict())
    assert names == [str(n) for n in kats["names"]]
    for i, k in enumerate(names):
        if not k.endswith("num_batches_tracked"):
            tol = 1e-6 * max(1.0, kats["abss"][i])
            assert abs(sums[i] - kats["sums"][i]) <= tol and abs(abss[i] - kats["abss"][i]) <= tol, k
    d64 = dd.ref_decode(model.state_dict(), dd.case_states(name)).numpy()
    assert d64.shape == (dd.N_STATES, du.CASES[name]["channels"], 224, 224)
    scale = np.abs(kats["lattice64"]).max()
    assert set(range(4)) | set(range(220, 224)) <= set(dd.LATTICE.tolist())
    assert np.abs(dd.lattice(d64) - kats["lattice64"]).max() <= 1e-10 * scale
    s1, s2 = dd.plane_sums(d64)
    npix = 224 * 224
    assert np.abs(s1 - kats["plane_sum"]).max() <= 1e-10 * scale * npix
    assert np.abs(s2 - kats["plane_sumsq"]).max() <= 1e-10 * scale * scale * npix
