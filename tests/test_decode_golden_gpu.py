"""srlz.deploy.FrameDecoder against the UNMODIFIED reference: tests/golden/decode_kats.npz holds the eval-mode decode of the
reference's own model classes on the CPU (tools/make_golden_decode.py) for four seeded models with closed-form BatchNorm parameters
(negative gammas, variances over two decades) on three integer-formula states — the fp64 tensor on a pixel lattice that includes the
four outermost rows and columns at every edge; decode_spread.json the reference's own fp32-to-fp64 spread.  The full image is checked
against the fp64 restatement of decode_util, which tests/test_decode_host_cpu.py holds to the golden lattice and plane sums at 1e-10.
Bound: max(1e-4, 10 x that spread) of the output's scale; every byte b satisfies |b - 255 v64| <= 0.5 + 255 x that bound, with no
pixel excluded (v64 = the fp64 denormalised value, which never clips for these models).

Checked per model: the seeded construction reproduces the reference's parameters (checksums); N = 1, 2, 3 states, a bare state, host and
device states, both layouts; no side effect on the model or on torch's RNG; the "model" route (an mlp auto-encoder, N > max_batch)
equal to the model's own eval decode; refresh(); reconstruct()."""
import json
import os

import numpy as np
import pytest
import torch

import decode_util as dd
import deploy_util as du
import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(gu.GOLDEN_DIR, "decode_kats.npz"), allow_pickle=False) as z:
        kats = {k: z[k] for k in z.files}
    with open(os.path.join(gu.GOLDEN_DIR, "decode_spread.json")) as f:
        spread = json.load(f)
    return kats, spread


_MODELS = {}


def _model(name):
    """The case's model on the GPU (built once per session, in train mode as a learner leaves it), its states, and the fp64
    restatement of its decode over the full image (computed once, never changed)."""
    if name not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        assert torch.cuda.is_available()
        m = dd.build_case(name, modules, pre)
        z = dd.case_states(name)
        ref = dd.ref_decode(m.state_dict(), z).numpy()
        ref.setflags(write=False)
        m = m.to(torch.device("cuda", 0))
        m.train()
        _MODELS[name] = (m, z, ref)
    return _MODELS[name]


def _own_decode(model, z_dev):
    """This build's decode in eval mode (the route a caller takes without the decoder), modes put back."""
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            return model.model.decode(z_dev).clone()
    finally:
        for m, was in modes:
            m.training = was


def _bound(spread, name):
    return max(1e-4, 10.0 * spread[name])


@pytest.mark.parametrize("name", dd.CASES)
def test_seeded_construction_has_the_reference_parameters(golden, name):
    kats, _ = golden
    model, _, _ = _model(name)
    names, sums, abss = du.checksums(model.state_dict())
    assert names == [str(n) for n in kats[name + "/names"]]
    for i, k in enumerate(names):
        if k.endswith("num_batches_tracked"):
            continue
        tol = 1e-6 * max(1.0, kats[name + "/abss"][i])
        assert abs(sums[i] - kats[name + "/sums"][i]) <= tol and abs(abss[i] - kats[name + "/abss"][i]) <= tol, k


@pytest.mark.parametrize("layout", ["nhwc", "planar"])
@pytest.mark.parametrize("name", dd.CASES)
def test_frame_decoder_against_the_reference(golden, name, layout):
    from srlz import deploy
    kats, spread = golden
    model, z, ref = _model(name)
    c = du.CASES[name]["channels"]
    lat = kats[name + "/lattice64"]
    scale, bound = np.abs(ref).max(), _bound(spread, name)
    dec = deploy.FrameDecoder(model, max_batch=4, frame_layout=layout)
    assert dec.route == "blocks" and dec.channels == c and dec.state_dim == du.CASES[name]["state_dim"] and dec.frame_size == (224, 224)
    v64 = dd.denormalize64(ref)
    assert v64.min() > 0.0 and v64.max() < 1.0  # nothing clips: the byte bound below needs no excluded pixel
    v64 = v64 if layout == "planar" else v64.transpose(0, 3, 2, 1)
    byte_bound = 0.5 + 255.0 * bound
    for n in (1, 2, 3):
        got = dec.decoded(z[:n]).cpu().numpy()                        # host states, through the pinned buffer
        got_dev = dec.decoded(torch.from_numpy(z[:n]).cuda()).cpu().numpy()  # device states, read in place
        assert dec.route == "blocks" and got.shape == (n, c, 224, 224) and got.dtype == np.float32
        assert np.array_equal(got, got_dev)
        e_lat = np.abs(dd.lattice(got) - lat[:n]).max() / scale
        e_ref = np.abs(got - ref[:n]).max() / scale
        frames = dec(z[:n]).cpu().numpy()
        frames_dev = dec(torch.from_numpy(z[:n]).cuda()).cpu().numpy()
        assert frames.dtype == np.uint8 and frames.shape == ((n, 224, 224, c) if layout == "nhwc" else (n, c, 224, 224))
        e_byte = np.abs(frames.astype(np.float64) - 255.0 * v64[:n]).max()
        print("%s %s N=%d: vs golden lattice %.3e, vs fp64 restatement %.3e of the scale (bound %.1e); bytes off by at most %.4f "
              "(bound %.4f), byte std %.1f" % (name, layout, n, e_lat, e_ref, bound, e_byte, byte_bound, frames.std()))
        assert e_lat <= bound and e_ref <= bound
        assert e_byte <= byte_bound
        assert np.array_equal(frames, frames_dev)
        assert np.array_equal(frames, dd.bytes_expr(got, layout))     # exactly the expression on the decoder's own floats
        assert np.array_equal(dec.numpy(z[:n]), frames)
    one = dec(z[1])
    assert one.shape == frames.shape[1:] and torch.equal(one.cpu(), dec(z[1:2])[0].cpu())  # a bare state -> one frame; same bits
    assert dec.decoded(z[1]).shape == (c, 224, 224)
    own = _own_decode(model, torch.from_numpy(z).cuda()).double().cpu().numpy()
    e_own = np.abs(own - ref).max() / scale
    print("%s: own eval decode vs fp64 restatement %.3e of the scale" % (name, e_own))
    assert e_own <= bound


def test_bgr_reverses_each_camera():
    from srlz import deploy
    model, z, _ = _model("ae_c6")
    rgb = deploy.FrameDecoder(model, max_batch=2)(z[:2]).cpu().numpy()
    bgr = deploy.FrameDecoder(model, max_batch=2, bgr=True)(z[:2]).cpu().numpy()
    assert np.array_equal(bgr, rgb[..., [2, 1, 0, 5, 4, 3]])


def test_a_call_leaves_the_model_and_the_rng_alone():
    from srlz import deploy
    model, z, _ = _model("vae")
    assert model.training
    dec = deploy.FrameDecoder(model, max_batch=2)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    f = dec(z[:2])
    d = dec.decoded(torch.from_numpy(z[:1]).cuda())
    assert not d.requires_grad and d.grad_fn is None and f.dtype == torch.uint8
    dec.numpy(z[:1])
    dec(z)  # N = 3 > max_batch: route "model"
    assert dec.route == "model"
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    assert model.training and all(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    for k, v in after.items():  # parameters, running statistics and num_batches_tracked
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in model.parameters())


def test_more_states_than_max_batch_take_the_model_route():
    from srlz import deploy
    model, z, _ = _model("ae")
    for layout in ("nhwc", "planar"):
        dec = deploy.FrameDecoder(model, max_batch=2, frame_layout=layout)
        dev = torch.from_numpy(z).cuda()
        got = dec.decoded(dev)
        assert dec.route == "model" and model.training
        own = _own_decode(model, dev)
        assert torch.equal(got, own)
        frames = dec(z)
        assert dec.route == "model" and np.array_equal(frames.cpu().numpy(), dd.bytes_expr(own.cpu().numpy(), layout))
        assert np.array_equal(dec.numpy(z), frames.cpu().numpy())
        dec(z[:2])
        assert dec.route == "blocks"


def test_a_dense_auto_encoder_takes_the_model_route():
    from srlz import deploy
    from test_dense_host_cpu import build
    model = build("mlp", ["autoencoder"], S=8).to(torch.device("cuda", 0))
    z = dd.states(2, 8)
    own = _own_decode(model, torch.from_numpy(z).cuda())
    assert own.shape == (2, 3 * 224 * 224)
    own = own.view(2, 3, 224, 224)
    for layout in ("nhwc", "planar"):
        dec = deploy.FrameDecoder(model, frame_layout=layout, bgr=True)
        assert dec.route == "model" and dec.state_dim == 8
        got = dec.decoded(z)
        assert dec.route == "model" and model.training and torch.equal(got, own)
        frames = dec(z)
        assert np.array_equal(frames.cpu().numpy(), dd.bytes_expr(own.cpu().numpy(), layout, bgr=True))
        assert np.array_equal(dec.numpy(z[0]), frames[0].cpu().numpy())


def test_refresh_picks_up_changed_weights(golden):
    from srlz import deploy
    _, spread = golden
    model, z, _ = _model("ae")
    dec = deploy.FrameDecoder(model, max_batch=4)
    first = dec.decoded(z).clone()
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        with torch.no_grad():
            model.model.decoder_conv[6].weight.mul_(1.25)
            model.model.decoder_conv[10].running_mean.add_(0.1)
        stale = dec.decoded(z).clone()
        assert torch.equal(stale, first)  # the packed weights and the records are the decoder's own copies
        dec.refresh()
        fresh = dec.decoded(z).clone()
        own = _own_decode(model, torch.from_numpy(z).cuda())
        scale = own.abs().max().item()
        assert (fresh - own).abs().max().item() / scale <= _bound(spread, "ae")
        assert (fresh - first).abs().max().item() / scale > 1e-2
    finally:
        model.load_state_dict(saved)


def test_reconstruct_is_the_two_calls_bit_for_bit():
    from srlz import deploy
    model, _, _ = _model("split_ae_inverse")
    frames = du.frames_nhwc(2, 224, 224, 3)
    enc = deploy.StateEncoder(model, max_batch=2)
    dec = deploy.FrameDecoder(model, max_batch=2)
    both = deploy.reconstruct(enc, dec, frames).clone()
    assert enc.route == "blocks" and dec.route == "blocks" and both.shape == (2, 224, 224, 3) and both.dtype == torch.uint8
    states = enc(frames).cpu().numpy()   # through the host
    apart = dec(states)
    assert torch.equal(both, apart)
    assert np.array_equal(dec.numpy(states), both.cpu().numpy())
