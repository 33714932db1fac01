"""srlz.deploy.StateEncoder against the UNMODIFIED reference: tests/golden/deploy_kats.npz holds the eval-mode getStates of the
reference's own model classes on the CPU (tools/make_golden_deploy.py) for five seeded models with closed-form BatchNorm parameters
(deploy_util.bn_formula: negative gammas, variances over two decades) on three integer-formula frames; deploy_spread.json the
reference's own fp32-to-fp64 spread.  Bound: max(1e-4, 10 x that spread) of the states' scale — the PCA test's rule.

Checked per model: the seeded construction reproduces the reference's parameters (checksums); StateEncoder for N = 1, 2, 3 frames, a
bare frame, both byte layouts, device and host frames; the same bound against this build's own getStates in eval mode; no side effect
on the model or on torch's RNG; the "model" route (an mlp model, N > max_batch) bit-identical to getStates; refresh()."""
import json
import os

import numpy as np
import pytest
import torch

import deploy_util as du
import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(gu.GOLDEN_DIR, "deploy_kats.npz"), allow_pickle=False) as z:
        kats = {k: z[k] for k in z.files}
    with open(os.path.join(gu.GOLDEN_DIR, "deploy_spread.json")) as f:
        spread = json.load(f)
    return kats, spread


_MODELS = {}


def _model(name):
    """The case's model on the GPU (built once per session, in train mode as a learner leaves it) and its frames."""
    if name not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        assert torch.cuda.is_available()
        m = du.build_case(name, modules, pre).to(torch.device("cuda", 0))
        m.train()
        _MODELS[name] = (m, du.case_frames(name))
    return _MODELS[name]


def _own_states(model, frames_dev):
    """This build's getStates in eval mode on the normalised frames (the route the RL side takes without the encoder)."""
    from srlz import ops
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            return model.getStates(ops.normalize_u8(frames_dev)).clone()
    finally:
        model.train(was)


def _bound(spread, name):
    return max(1e-4, 10.0 * spread[name])


@pytest.mark.parametrize("name", list(du.CASES))
def test_seeded_construction_has_the_reference_parameters(golden, name):
    kats, _ = golden
    model, _ = _model(name)
    names, sums, abss = du.checksums(model.state_dict())
    assert names == [str(n) for n in kats[name + "/names"]]
    for i, k in enumerate(names):
        if k.endswith("num_batches_tracked"):
            continue
        tol = 1e-6 * max(1.0, kats[name + "/abss"][i])  # (fp32 parameters summed in fp64: equal weights give equal sums)
        assert abs(sums[i] - kats[name + "/sums"][i]) <= tol and abs(abss[i] - kats[name + "/abss"][i]) <= tol, k


@pytest.mark.parametrize("layout", ["nhwc", "planar"])
@pytest.mark.parametrize("name", list(du.CASES))
def test_state_encoder_against_the_reference_and_own_getstates(golden, name, layout):
    from srlz import deploy
    kats, spread = golden
    model, frames = _model(name)
    ref = torch.from_numpy(kats[name + "/states64"])
    scale, bound = ref.abs().max().item(), _bound(spread, name)
    enc = deploy.StateEncoder(model, max_batch=4, frame_layout=layout)
    assert enc.route == "blocks" and enc.channels == du.CASES[name]["channels"] and enc.state_dim == du.CASES[name]["state_dim"]
    own = _own_states(model, torch.from_numpy(frames).cuda()).double().cpu()
    e_own = (own - ref).abs().max().item() / scale
    print("%s: own getStates vs reference fp64 %.3e of the scale (bound %.1e)" % (name, e_own, bound))
    assert e_own <= bound
    given = frames if layout == "nhwc" else du.to_planar(frames)
    for n in (1, 2, 3):
        host = enc(given[:n]).double().cpu()          # numpy frames, through the pinned buffer
        dev = enc(torch.from_numpy(given[:n]).cuda()).double().cpu()  # device frames, read in place
        assert enc.route == "blocks" and host.shape == (n, enc.state_dim)
        assert torch.equal(host, dev)
        e_ref = (host - ref[:n]).abs().max().item() / scale
        e_get = (host - own[:n]).abs().max().item() / scale
        print("%s %s N=%d: vs reference fp64 %.3e, vs own getStates %.3e of the scale" % (name, layout, n, e_ref, e_get))
        assert e_ref <= bound and e_get <= bound
        assert np.array_equal(enc.numpy(given[:n]), host.float().numpy())
    one = enc(given[1])
    assert one.shape == (enc.state_dim,) and torch.equal(one.cpu(), enc(given[1:2])[0].cpu())  # a bare frame -> [S]; same bits


def test_a_call_leaves_the_model_and_the_rng_alone():
    from srlz import deploy
    model, frames = _model("vae")
    assert model.training
    enc = deploy.StateEncoder(model, max_batch=4)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    s = enc(frames)
    assert not s.requires_grad and s.grad_fn is None
    enc.numpy(frames[:1])
    enc(torch.from_numpy(frames[:2]).cuda())
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    assert model.training and all(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    for k, v in after.items():  # parameters, running statistics and num_batches_tracked
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in model.parameters())


def test_more_frames_than_max_batch_take_the_model_route_bit_for_bit():
    from srlz import deploy
    model, frames = _model("ae")
    enc = deploy.StateEncoder(model, max_batch=2)
    dev = torch.from_numpy(frames).cuda()
    got = enc(dev)
    assert enc.route == "model" and model.training
    assert torch.equal(got, _own_states(model, dev))
    enc(frames[:2])
    assert enc.route == "blocks"


def test_a_model_without_a_conv_encoder_takes_the_model_route_bit_for_bit():
    from srlz import deploy
    from test_dense_host_cpu import build
    model = build("mlp", ["autoencoder"], S=8).to(torch.device("cuda", 0))
    frames = du.frames_nhwc(2, 224, 224, 3)
    for layout, given in (("nhwc", frames), ("planar", du.to_planar(frames))):
        enc = deploy.StateEncoder(model, frame_layout=layout)
        assert enc.route == "model"
        got = enc(given)
        assert enc.route == "model" and model.training and got.shape == (2, 8)
        assert torch.equal(got, _own_states(model, torch.from_numpy(frames).cuda()))
        assert np.array_equal(enc.numpy(given), got.cpu().numpy())


def test_refresh_picks_up_changed_weights(golden):
    from srlz import deploy
    _, spread = golden
    model, frames = _model("cnn_inverse")
    enc = deploy.StateEncoder(model, max_batch=4)
    first = enc(frames).clone()
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        with torch.no_grad():
            model.model.conv_layers[4].weight.mul_(1.25)
            model.model.conv_layers[9].running_mean.add_(0.1)
        stale = enc(frames).clone()
        assert torch.equal(stale, first)  # the packed weights and the records are the encoder's own copies
        enc.refresh()
        fresh = enc(frames).clone()
        own = _own_states(model, torch.from_numpy(frames).cuda())
        scale = own.abs().max().item()
        assert (fresh - own).abs().max().item() / scale <= _bound(spread, "cnn_inverse")
        assert (fresh - first).abs().max().item() / scale > 1e-2
    finally:
        model.load_state_dict(saved)
