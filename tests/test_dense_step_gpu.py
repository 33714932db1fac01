"""Training steps of the mlp / linear models through the product's route (SRL4robotics.trainStep: the loader's uint8 frames, the two frames
as one batched call, the reconstruction / generation loss inside the output layer, the flat gradient bucket) against an fp64 restatement
of the reference's dense models (models/autoencoders.py:6-81, vae.py:6-40, priors.py:71-125) plugged into the oracle's train step:
loss terms, states and every gradient of the bucket (the conv stacks the dense models build but never run get exactly zero)."""
import contextlib
import io
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---- fp64 restatement of the dense models, in the oracle's (sd, x, training, ...) signatures --------------------------------------
def _seq(sd, p, x, idx, act):
    for j, i in enumerate(idx):
        x = F.linear(x, sd["%s.%d.weight" % (p, i)], sd["%s.%d.bias" % (p, i)])
        if j < len(idx) - 1:
            x = act(x)
    return x


def dense_ae_forward(sd, x, training, taps=None, pins=None, split=None):
    flat = x.reshape(x.size(0), -1)
    if "model.encoder.2.weight" in sd:  # DenseAutoEncoder
        s = _seq(sd, "model.encoder", flat, (0, 2, 4), torch.tanh)
        d = _seq(sd, "model.decoder", s, (0, 2, 4), torch.tanh)
    else:  # LinearAutoEncoder
        s = _seq(sd, "model.encoder", flat, (0,), None)
        d = _seq(sd, "model.decoder", s, (0,), None)
    return s, d.view(x.size())


def dense_vae_encode(sd, x, training, pins=None):
    h = torch.relu(F.linear(x.reshape(x.size(0), -1), sd["model.encoder_fc1.weight"], sd["model.encoder_fc1.bias"]))
    return (F.linear(h, sd["model.encoder_fc21.weight"], sd["model.encoder_fc21.bias"]),
            F.linear(h, sd["model.encoder_fc22.weight"], sd["model.encoder_fc22.bias"]))


def dense_vae_forward(sd, x, training, eps=None, pins=None, split=None):
    mu, logvar = dense_vae_encode(sd, x, training)
    z = eps * torch.exp(0.5 * logvar) + mu if training else mu
    return _seq(sd, "model.decoder", z, (0, 2, 4), torch.relu).view(x.size()), mu, logvar


def dense_net_forward(sd, x, training, pins=None):
    flat = x.reshape(x.size(0), -1)
    if "model.fc.0.weight" in sd:  # SRLDenseNetwork (its 1e-6 training noise is below the tolerance)
        return _seq(sd, "model.fc", flat, (0, 2), torch.relu)
    return F.linear(flat, sd["model.fc.weight"], sd["model.fc.bias"])  # SRLLinear


@pytest.fixture
def twin(monkeypatch):
    from oracle import torch_twin as T
    monkeypatch.setattr(T, "ae_forward", dense_ae_forward)
    monkeypatch.setattr(T, "vae_encode", dense_vae_encode)
    monkeypatch.setattr(T, "vae_forward", dense_vae_forward)
    monkeypatch.setattr(T, "cnn_forward", dense_net_forward)
    return T


def u8_frames(B, C, seed):
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.randint(0, 256, (2 * B, C, 224, 224)).astype(np.uint8))


def learner(model_type, losses, C, S=200, lr=1e-4, l1_reg=0.0, l2_reg=0.0):
    import preprocessing.preprocess as pre
    from models.learner import SRL4robotics
    pre.N_CHANNELS = C
    with contextlib.redirect_stdout(io.StringIO()):
        return SRL4robotics(S, model_type=model_type, seed=1, learning_rate=lr, cuda=True, losses=losses, n_actions=6,
                            log_folder="/tmp", l1_reg=l1_reg, l2_reg=l2_reg)


def bucket_grads(srl):
    flat = srl.flat_params
    named = [(n, p) for n, p in srl.model.named_parameters() if p.requires_grad]
    return OrderedDict((n, flat.grad[off:off + p.numel()].view(p.shape).double().cpu()) for (n, p), off in zip(named, flat.offsets))


CASES = [("mlp_ae", "mlp", ["autoencoder"], 3), ("mlp_dae", "mlp", ["dae"], 3), ("mlp_vae", "mlp", ["vae"], 3),
         ("linear_ae", "linear", ["autoencoder"], 3), ("mlp_if", "mlp", ["inverse", "forward"], 3),
         ("linear_if", "linear", ["inverse", "forward"], 3), ("mlp_ae_c6", "mlp", ["autoencoder"], 6),
         ("mlp_ae_if", "mlp", ["autoencoder", "inverse", "forward"], 3), ("mlp_vae_if", "mlp", ["vae", "inverse"], 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,model_type,losses,C", CASES)
@pytest.mark.parametrize("n_steps", [1, 3])
def test_dense_step_matches_fp64_restatement(twin, name, model_type, losses, C, n_steps):
    from losses.losses import LossManager
    from srlz import ops
    import preprocessing.preprocess as pre
    T = twin
    B, S = 2, 200
    if n_steps > 1 and name not in ("mlp_ae", "mlp_vae", "linear_ae"):
        pytest.skip("Adam traces on three models")
    try:
        srl = learner(model_type, losses, C, S=S)
        sd = T.clone_state(OrderedDict((k, v.detach().double()) for k, v in srl.model.state_dict().items()))
        adam = T.TwinAdam(sd, 1e-4)
        tiny = {}
        for step in range(n_steps):
            frames = u8_frames(B, C, 100 + step)
            actions = torch.from_numpy(np.random.RandomState(7 + step).randint(0, 6, (B,)).astype(np.int64))
            o, no = srl._toDevicePair(frames[:B], frames[B:])
            assert o.dtype == (torch.float32 if "dae" in losses else torch.uint8)  # the byte route where it applies
            obs = ops.frames_as_float(frames[:B].cuda()).double().cpu()
            next_obs = ops.frames_as_float(frames[B:].cuda()).double().cpu()
            kw = {}
            noisy = (None, None)
            if "dae" in losses:
                g = torch.Generator().manual_seed(11 + step)
                noisy = tuple(t * (torch.rand(t.shape, generator=g, dtype=torch.float64) > 0.3).double() for t in (obs, next_obs))
                kw = dict(noisy_obs=noisy[0].float().cuda(), next_noisy_obs=noisy[1].float().cuda())
            eps = None
            if "vae" in losses:
                g = torch.Generator().manual_seed(21 + step)
                eps = [torch.randn((B, S), generator=g, dtype=torch.float64) for _ in range(2)]
                it = iter([e.float().cuda() for e in eps])
                srl.model.model.eps_fn = lambda mu: next(it)
            lm = LossManager(srl.model, None)
            loss = srl.trainStep(o, no, actions.view(-1, 1).cuda(), lm, **kw)
            torch.cuda.synchronize()
            ref = T.train_step(sd, losses, obs, next_obs, actions, eps=eps[0] if eps else None, next_eps=eps[1] if eps else None,
                               noisy=noisy)
            assert abs(float(loss.detach()) - ref["total"]) <= 1e-4 * abs(ref["total"]), (step, float(loss.detach()), ref["total"])
            for k, (nm, v) in enumerate(ref["losses"].items()):
                assert abs(float(lm.losses[k]) - v) <= 1e-4 * max(abs(v), 1e-6), (step, nm)
            grads = bucket_grads(srl)
            for k, g in grads.items():
                r = ref["grads"].get(k)
                if r is None:  # unused parameters (the never-run conv stacks, heads without a loss): None in torch, zero in the bucket
                    assert not g.abs().max().item(), k
                else:
                    assert rel(g, r) < 1e-4, (step, k, rel(g, r))
            for k, r in ref["grads"].items():
                if r is not None:  # elements whose gradient is near zero at some step (relative to the tensor's largest)
                    near = r.abs() < 1e-3 * r.abs().max()
                    tiny[k] = near if k not in tiny else (tiny[k] | near)
            adam.step(sd)
        # parameters after the Adam steps: where the gradient was well away from zero at every step, the update is the twin's to 1 % of
        # lr; an element whose gradient is near zero moves by +-lr with a sign set by its last bits, so there only Adam's own bound (at
        # most lr per step from the twin) holds; parameters without a gradient must not move at all
        lr = 1e-4
        for k, v in srl.model.state_dict().items():
            if k in sd and sd[k].requires_grad:
                diff = (v.double().cpu() - sd[k].detach()).abs()
                if k not in tiny:
                    assert diff.max().item() == 0.0, k
                    continue
                assert diff.max().item() <= 2.0 * lr * n_steps * 1.01, (k, diff.max().item())
                firm = ~tiny[k]
                if firm.any():
                    assert diff[firm].max().item() <= 1e-2 * lr * n_steps, (k, diff[firm].max().item())
        with torch.no_grad():
            srl.model.eval()
            states = srl.model.getStates(ops.frames_as_float(frames[:B].cuda()))
        fwd = {"mlp_vae": lambda: dense_vae_encode(sd, obs, False)[0], "mlp_vae_if": lambda: dense_vae_encode(sd, obs, False)[0]}
        ref_states = fwd[name]() if name in fwd else (dense_ae_forward(sd, obs, False)[0] if ("autoencoder" in losses or "dae" in losses)
                                                      else dense_net_forward(sd, obs, False))
        assert rel(states, ref_states.detach()) < 1e-4
    finally:
        pre.N_CHANNELS = 3


@pytest.mark.gpu
def test_dense_eval_forward_returns_decoded_frames():
    from srlz import ops
    srl = learner("mlp", ["autoencoder"], 3, S=20)
    x = ops.frames_as_float(u8_frames(1, 3, 5).cuda())
    srl.model.eval()
    with torch.no_grad():
        states, decoded = srl.model(x)
    assert states.shape == (2, 20) and decoded.shape == x.shape and torch.isfinite(decoded).all()
    vae = learner("mlp", ["vae"], 3, S=20)
    vae.model.eval()
    with torch.no_grad():
        dec, mu, logvar = vae.model(x)
    assert dec.shape == x.shape and mu.shape == (2, 20)


@pytest.mark.gpu
def test_dense_noise_layer_train_and_eval():
    """GaussianNoiseVariant(1e-6) on SRLDenseNetwork's output in train mode only (reference custom_layers.py:31-51)."""
    from srlz import ops
    srl = learner("mlp", ["inverse"], 3, S=200)
    x = ops.frames_as_float(u8_frames(16, 3, 6).cuda())
    m = srl.model.model
    with torch.no_grad():
        m.train()
        a, b = m(x), m(x)
        d = (a - b).double()
        std = d.std().item() / np.sqrt(2.0)
        assert 0.5e-6 <= std <= 2e-6, std
        m.eval()
        assert torch.equal(m(x), m(x))


def _fp64_full_grads(sd, obs, losses):
    """The reconstruction loss's gradient over all images in fp64 on the GPU."""
    sd = OrderedDict((k, v.detach().double().cuda().requires_grad_(True)) for k, v in sd.items() if v.is_floating_point())
    half = obs.shape[0] // 2
    s, d = dense_ae_forward(sd, obs, True)
    loss = ((d[:half] - obs[:half]) ** 2).sum() / obs[:half].numel() + ((d[half:] - obs[half:]) ** 2).sum() / obs[half:].numel()
    loss.backward()
    return float(loss), {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("model_type", ["mlp", "linear"])
def test_fullsize_dense_ae_bucket(model_type):
    """bs = 256: the whole gradient bucket of one step (512 images) against the fp64 backward over all of them."""
    from losses.losses import LossManager
    from srlz import ops
    srl = learner(model_type, ["autoencoder"], 3, S=200)
    init = OrderedDict((k, v.detach().clone()) for k, v in srl.model.state_dict().items())
    B = 256
    frames = u8_frames(B, 3, 31)
    o, no = srl._toDevicePair(frames[:B], frames[B:])
    lm = LossManager(srl.model, None)
    loss = srl.trainStep(o, no, torch.zeros((B, 1), dtype=torch.int64, device="cuda"), lm)
    torch.cuda.synchronize()
    grads = bucket_grads(srl)
    del srl, o, no
    obs = ops.frames_as_float(frames.cuda()).double()
    ref_loss, ref = _fp64_full_grads(init, obs, ["autoencoder"])
    assert abs(float(loss) - ref_loss) <= 1e-4 * ref_loss
    for k, r in ref.items():
        assert rel(grads[k], r) < 1e-4, (k, rel(grads[k], r))


# ---- against the UNMODIFIED reference (tools/make_golden.py step_case on the reference's dense models, CPU fp32) ---------------------
GOLDEN = [("step_mlp_ae_b2", "mlp", ["autoencoder"], 3, 1, 0.0, 0.0), ("step_mlp_dae_b2", "mlp", ["dae"], 3, 1, 0.0, 0.0),
          ("step_mlp_vae_b2", "mlp", ["vae"], 3, 1, 0.0, 0.0), ("step_linear_ae_b2", "linear", ["autoencoder"], 3, 1, 0.0, 0.0),
          ("step_mlp_if_b2", "mlp", ["inverse", "forward"], 3, 1, 0.0, 0.0),
          ("step_linear_if_b2", "linear", ["inverse", "forward"], 3, 1, 0.0, 0.0),
          ("step_mlp_ae_c6_b2", "mlp", ["autoencoder"], 6, 1, 0.0, 0.0),
          ("trace_mlp_ae_b2", "mlp", ["autoencoder"], 3, 3, 0.0, 0.0), ("trace_mlp_vae_b2", "mlp", ["vae"], 3, 3, 0.0, 0.0),
          ("trace_linear_ae_b2", "linear", ["autoencoder"], 3, 3, 0.0, 0.0),
          ("trace_mlp_ae_l1l2_b2", "mlp", ["autoencoder"], 3, 3, 1e-5, 1e-4)]
RTOL = 1e-4


def _thin(sub):
    """The samples tools/make_golden.py keeps of a dense model's digest: v[::ceil(len / 4096)]."""
    return sub[::max(1, -(-len(sub) // 4096))]


def _check_digest(t, g, prefix, rtol=RTOL):
    import golden_util as gu
    d = gu.tensor_digest(t)
    ref_sub = g[prefix + "/sub"]
    sub = _thin(d["sub"])
    assert sub.shape == ref_sub.shape, prefix
    assert np.abs(sub - ref_sub).max() <= rtol * max(np.abs(ref_sub).max(), 1e-30), prefix
    l2 = float(g[prefix + "/l2"])
    assert abs(float(d["l2"]) - l2) <= rtol * max(l2, 1e-30), prefix
    assert abs(float(d["sum"]) - float(g[prefix + "/sum"])) <= rtol * max(float(g[prefix + "/abs"]), 1e-30), prefix


@pytest.mark.gpu
@pytest.mark.parametrize("name,model_type,losses,C,n_steps,l1,l2", GOLDEN)
def test_dense_step_matches_reference_golden(name, model_type, losses, C, n_steps, l1, l2):
    """trainStep (the product's route, the reference's own synthetic frames) against the reference's numbers: loss terms, states,
    reconstructions and every gradient of the first step; the losses of every step of an Adam trace and the parameters it ends at.
    With l1 / l2 the conv stacks the dense models never run get the regularisers' gradients and Adam moves them, as in torch."""
    import golden_util as gu
    import preprocessing.preprocess as pre
    from losses.losses import LossManager
    g = gu.load(name)
    B, S, lr = 2, 200, 1e-4
    try:
        srl = learner(model_type, losses, C, S=S, lr=lr, l1_reg=l1, l2_reg=l2)
        init = OrderedDict((k, v.detach().clone()) for k, v in srl.model.state_dict().items())
        obs0 = torch.from_numpy(gu.golden_inputs(B, C, 6, seed=1234)[0]).cuda()

        def eval_states():
            with torch.no_grad():
                srl.model.eval()
                return srl.model.getStates(obs0)
        # the reference's "learned states" of a step case are those of the initial model (no optimiser there), of a trace the final one
        st0 = eval_states() if n_steps == 1 else None
        trace = []
        for step in range(n_steps):
            obs_np, next_np, actions = gu.golden_inputs(B, C, 6, seed=1234 + step)
            o, no = srl._toDevicePair(torch.from_numpy(obs_np), torch.from_numpy(next_np))
            kw = {}
            if "dae" in losses:
                kw = dict(noisy_obs=torch.from_numpy(gu.golden_noisy(obs_np, seed=1234 + step)).cuda(),
                          next_noisy_obs=torch.from_numpy(gu.golden_noisy(next_np, seed=4321 + step)).cuda())
            if "vae" in losses:
                torch.manual_seed(99 + step)  # the reference's two draws of this step (std.new(...).normal_())
                it = iter([torch.randn(B, S).cuda(), torch.randn(B, S).cuda()])
                srl.model.model.eps_fn = lambda mu: next(it)
            if step == 0:
                with torch.no_grad():
                    srl.model.train()
                    x, nx = (kw["noisy_obs"], kw["next_noisy_obs"]) if kw else (o, no)  # (the DAE encodes the occluded frames)
                    states = srl.model.getStates(x)
                    next_states = srl.model.getStates(nx)
                    dec = srl.model(o)[1] if ("autoencoder" in losses or "dae" in losses) and not kw else None
                    if hasattr(srl.model.model, "forgetRecent"):
                        srl.model.model.forgetRecent()
                    if "vae" in losses:  # the draws above were consumed by nothing: redo them for the step
                        torch.manual_seed(99 + step)
                        it = iter([torch.randn(B, S).cuda(), torch.randn(B, S).cuda()])
            lm = LossManager(srl.model, None)
            loss = srl.trainStep(o, no, torch.from_numpy(actions).view(-1, 1).cuda(), lm, **kw)
            torch.cuda.synchronize()
            rec = dict(zip(lm.names, [float(v) for v in lm.losses]))
            rec["total"] = float(loss.detach())
            trace.append(rec)
            if step == 0:
                for k in [f for f in g.files if f.startswith("loss/")]:
                    nm, v = k[len("loss/"):], float(g[k])
                    assert abs(rec[nm] - v) <= RTOL * max(abs(v), 1e-6), (k, rec[nm], v)
                _check_digest(states, g, "states")
                _check_digest(next_states, g, "next_states")
                if dec is not None:
                    _check_digest(dec, g, "decoded")
                for k, gr in bucket_grads(srl).items():
                    if ("grad/" + k + "/none") in g.files:
                        assert not gr.abs().max().item(), k  # None in torch: an exact zero in the bucket
                    else:
                        _check_digest(gr, g, "grad/" + k)
        if n_steps > 1:
            names = [str(n) for n in g["trace/names"]]
            for step, row in enumerate(g["trace/values"]):
                for nm, v in zip(names, row):
                    assert abs(trace[step][nm] - v) <= 1e-3 * max(abs(v), 1e-6), (step, nm, trace[step][nm], v)
            sd = srl.model.state_dict()
            for k, ref_sum, ref_abs in zip(g["final/names"], g["final/sums"], g["final/abss"]):
                k = str(k)
                v = sd[k].double().cpu()
                if "num_batches_tracked" in k:
                    assert int(v) == int(ref_sum), k
                    continue
                moved = not torch.equal(sd[k].cpu(), init[k].cpu())
                if l1 == 0 and l2 == 0 and (".encoder_conv." in k or ".decoder_conv." in k):
                    assert not moved, k  # no gradient, no update (torch's Adam skips them; the bucket's zero moment gives zero)
                e = max(abs(float(v.sum()) - ref_sum), abs(float(v.abs().sum()) - ref_abs)) / (ref_abs + lr * n_steps * v.numel())
                assert e <= 2e-2, (k, e)
                if l1 > 0 and ("encoder_conv" in k or "decoder_conv" in k) and k.endswith("weight"):
                    assert moved, k  # the regularisers reach the unused stacks
        st = st0 if st0 is not None else eval_states()
        ref = g["eval_states/full"]
        assert np.abs(st.double().cpu().numpy() - ref).max() <= (RTOL if n_steps == 1 else 2e-2) * np.abs(ref).max()
    finally:
        pre.N_CHANNELS = 3
