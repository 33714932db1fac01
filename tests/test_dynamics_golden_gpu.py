"""srlz.deploy.LatentDynamics against the UNMODIFIED reference: tests/golden/dynamics_kats.npz holds the forwardModel / rewardModel
composition of the reference's own model classes on the CPU (tools/make_golden_dynamics.py) for four seeded models — S = 3, S = 8 with
an mlp inverse head, S = 200, and S = 200 with forward_net.weight x 20, an expanding recurrence — on sine-formula states and
integer-formula plans (N = 3, K = 4, T = 7, gamma = 0.9), in fp32 and fp64; dynamics_spread.json the reference's own fp32-to-fp64
spread.  Bound: max(1e-4, 10 x that spread) of each quantity's scale, trajectory and logits per step.

Checked: route "rollout" against the fixtures and against this build's own step-by-step composition; route "model" bit-identical to
that composition (a split model, a call beyond max_rows); host and device inputs; step; best and act on a tie; no side effects; act
chained behind a StateEncoder; imagine against the decoder on the trajectory's rows."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import deploy_util as du
import dynamics_util as dy
import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(gu.GOLDEN_DIR, "dynamics_kats.npz"), allow_pickle=False) as z:
        kats = {k: z[k] for k in z.files}
    with open(os.path.join(gu.GOLDEN_DIR, "dynamics_spread.json")) as f:
        spread = json.load(f)["cases"]
    return kats, spread


_MODELS = {}


def _dev():
    return torch.device("cuda", 0)


def _model(name):
    """The case's model on the GPU (built once per session, in train mode as a learner leaves it) and its inputs."""
    if name not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        m = dy.build_case(name, modules).to(_dev())
        m.train()
        _MODELS[name] = (m,) + dy.case_inputs(name)
    return _MODELS[name]


def _ae_model():
    """An auto-encoder with trained-by-name forward and reward heads: what act(enc(frames)) and imagine need."""
    if "ae" not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        torch.manual_seed(5)
        m = modules.SRLModules(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=["autoencoder", "forward", "reward"])
        _MODELS["ae"] = m.to(_dev())
    return _MODELS["ae"]


def _split_model():
    if "split" not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        torch.manual_seed(1)
        losses = ["autoencoder", "forward", "reward"]
        m = modules.SRLModulesSplit(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=losses,
                                    split_dimensions=OrderedDict(zip(losses, (4, 2, 2))))
        _MODELS["split"] = m.to(_dev())
    return _MODELS["split"]


def _own(model, z, pl, gamma):
    """This build's own composition, step by step: forwardModel then rewardModel of the model under no_grad (six launches a step)."""
    z = torch.as_tensor(z).to(_dev(), torch.float32)
    pl = torch.as_tensor(pl).to(_dev(), torch.int64)
    n, s = z.shape
    if pl.dim() == 2:
        pl = pl.unsqueeze(0).expand(n, -1, -1)
    k, t = pl.shape[1], pl.shape[2]
    acts = pl.reshape(n * k, t)
    traj, logits = [], []
    with torch.no_grad():
        cur = z.unsqueeze(1).expand(n, k, s).reshape(n * k, s).contiguous()
        ret = torch.zeros(n * k, dtype=torch.float32, device=_dev())
        g = torch.ones((), dtype=torch.float32, device=_dev())
        for step in range(t):
            nxt = model.forwardModel(cur, acts[:, step].contiguous())
            lg = model.rewardModel(cur, nxt)
            ret = ret + g * torch.softmax(lg, dim=1)[:, 1]
            g = g * gamma
            traj.append(nxt)
            logits.append(lg)
            cur = nxt
    return {"final": cur.view(n, k, s), "returns": ret.view(n, k), "trajectory": torch.stack(traj, 1).view(n, k, t, s),
            "reward_logits": torch.stack(logits, 1).view(n, k, t, 2)}


def _as_dict(out):
    return {"final": out.final_states, "returns": out.returns, "trajectory": out.trajectory, "reward_logits": out.reward_logits}


def _np(d):
    return {k: v.detach().double().cpu().numpy() for k, v in d.items() if v is not None}


@pytest.mark.parametrize("name", list(dy.CASES))
def test_latent_dynamics_against_the_reference_and_the_own_composition(golden, name):
    from srlz import deploy
    kats, spread = golden
    model, z, pl = _model(name)
    gamma = float(kats["gamma"])
    assert np.allclose(dy.checksums(model.state_dict()), kats[name + "/checksums"], rtol=1e-12, atol=0)
    dyn = deploy.LatentDynamics(model, max_rows=64, max_horizon=8)
    assert dyn.route == "rollout" and dyn.heads == ("forward", "inverse", "reward")
    assert (dyn.state_dim, dyn.n_actions) == (dy.CASES[name]["state_dim"], dy.N_ACTIONS)
    out = dyn.rollout(z, pl, gamma=gamma, keep_trajectory=True, keep_logits=True)
    assert dyn.route == "rollout"
    got = _np(_as_dict(out))
    own = _np(_own(model, z, pl, gamma))
    for q in dy.QUANTITIES:
        per_step, b = q != "returns", dy.bound(spread[name][q])
        e_ref = dy.rel_err(got[q], kats["%s/%s64" % (name, q)], per_step)
        e_own = dy.rel_err(got[q], own[q], per_step)
        e_model = dy.rel_err(own[q], kats["%s/%s64" % (name, q)], per_step)
        print("%s %s: rollout vs reference fp64 %.3e, vs own composition %.3e, own composition vs reference %.3e (bound %.1e)"
              % (name, q, e_ref, e_own, e_model, b))
        assert e_ref <= b and e_own <= b, q
    assert np.array_equal(got["final"], got["trajectory"][:, :, -1])
    assert out.best.dtype == torch.int64 and np.array_equal(out.best.cpu().numpy(), got["returns"].argmax(axis=1))


def test_host_and_device_inputs_and_bare_inputs_give_equal_bits():
    from srlz import deploy
    model, z, pl = _model("s8_mlp")
    dyn = deploy.LatentDynamics(model, max_rows=64, max_horizon=8)
    host = {k: v.clone() for k, v in _as_dict(dyn.rollout(z, pl, gamma=0.9, keep_trajectory=True, keep_logits=True)).items()}
    z_dev, pl_dev = torch.from_numpy(z).to(_dev()), torch.from_numpy(pl).to(_dev())
    for plans in (pl_dev, pl_dev.long(), pl.astype(np.int64)):
        dev = _as_dict(dyn.rollout(z_dev, plans, gamma=0.9, keep_trajectory=True, keep_logits=True))
        for q in host:
            assert torch.equal(dev[q], host[q]), q
    dbl = _as_dict(dyn.rollout(z.astype(np.float64), pl, gamma=0.9, keep_trajectory=True, keep_logits=True))
    assert torch.equal(dbl["final"], host["final"])
    # [K,T] shared by every environment, one bare [T] plan, one bare [S] state
    shared = dyn.rollout(z, pl[1], gamma=0.9, keep_trajectory=True)
    tiled = np.repeat(pl[1][None], z.shape[0], axis=0)
    shared_f, shared_r = shared.final_states.clone(), shared.returns.clone()
    again = dyn.rollout(z, tiled, gamma=0.9)
    assert torch.equal(shared_f, again.final_states) and torch.equal(shared_r, again.returns)
    bare = dyn.rollout(z[2], pl[2, 3], gamma=0.9, keep_trajectory=True, keep_logits=True)
    assert bare.final_states.shape == (8,) and bare.returns.shape == () and bare.trajectory.shape == (7, 8)
    assert bare.reward_logits.shape == (7, 2) and bare.best.shape == () and int(bare.best) == 0
    assert torch.equal(bare.trajectory, host["trajectory"][2, 3]) and torch.equal(bare.returns, host["returns"][2, 3])
    one = dyn.rollout(z[2], pl[2], gamma=0.9)
    assert one.final_states.shape == (4, 8) and torch.equal(one.returns, host["returns"][2])
    # optional outputs are None unless asked for
    lean = dyn.rollout(z, pl)
    assert lean.trajectory is None and lean.reward_logits is None and lean.returns is not None


def test_step_is_rollout_with_one_plan_of_one_step():
    from srlz import deploy
    model, z, pl = _model("s200")
    dyn = deploy.LatentDynamics(model, max_rows=8, max_horizon=4)
    acts = pl[:, 0, 0]
    nxt = dyn.step(z, acts).clone()
    assert dyn.route == "rollout" and nxt.shape == (3, 200)
    out = dyn.rollout(z, acts.reshape(3, 1, 1))
    assert torch.equal(out.final_states[:, 0], nxt)
    with torch.no_grad():
        own = model.forwardModel(torch.from_numpy(z).to(_dev()), torch.from_numpy(acts.astype(np.int64)).to(_dev()))
    assert (nxt - own).abs().max().item() <= 1e-4 * own.abs().max().item()
    assert torch.equal(dyn.step(z[1], acts[1]), nxt[1]) and torch.equal(dyn.step(torch.from_numpy(z).to(_dev()), torch.from_numpy(acts).to(_dev())), nxt)
    with pytest.raises(ValueError, match="actions"):
        dyn.step(z, acts[:2])


def test_the_model_route_is_the_own_composition_bit_for_bit():
    from srlz import deploy
    # a split model: its heads see masked states
    split = _split_model()
    z, pl = dy.sine_states(3, 8), dy.plans(3, 4, 7, 6)
    dyn = deploy.LatentDynamics(split)
    assert dyn.route == "model" and dyn.heads == ("forward", "reward")
    got = _as_dict(dyn.rollout(z, pl, gamma=0.9, keep_trajectory=True, keep_logits=True))
    own = _own(split, z, pl, 0.9)
    for q in own:
        assert torch.equal(got[q], own[q]), q
    # a call beyond max_rows, and one beyond max_horizon
    model, z, pl = _model("s8_mlp")
    for kw in (dict(max_rows=11, max_horizon=8), dict(max_rows=64, max_horizon=6)):
        dyn = deploy.LatentDynamics(model, **kw)
        assert dyn.route == "rollout"
        got = _as_dict(dyn.rollout(z, pl, gamma=0.9, keep_trajectory=True, keep_logits=True))
        assert dyn.route == "model"
        own = _own(model, z, pl, 0.9)
        for q in own:
            assert torch.equal(got[q], own[q]), q
        dyn.rollout(z[:2], pl[:2, :, :6])
        assert dyn.route == "rollout"
    forced = deploy.LatentDynamics(model, route="model")
    assert forced.route == "model" and torch.equal(forced.rollout(z, pl, gamma=0.9).returns, own["returns"])


def test_best_and_act_break_a_tie_to_the_lowest_plan():
    from srlz import deploy
    model, z, pl = _model("s3_linear")
    dyn = deploy.LatentDynamics(model, max_rows=64, max_horizon=8)
    tied = pl.copy()
    base = dyn.rollout(z, tied).returns.cpu().numpy()
    top = base.argmax(axis=1)
    for n in range(3):  # every environment's best plan twice: at its own place and (a copy) at another
        other = (top[n] + 2) % 4
        tied[n, other] = tied[n, top[n]]
    out = dyn.rollout(z, tied)
    r = out.returns.cpu().numpy()
    want = np.array([min(top[n], (top[n] + 2) % 4) for n in range(3)])
    for n in range(3):
        assert r[n, top[n]] == r[n, (top[n] + 2) % 4] == r[n].max()  # equal plans, equal bits
    assert np.array_equal(out.best.cpu().numpy(), want)
    a = dyn.act(z, tied)
    assert a.dtype == torch.int64 and a.shape == (3,) and a.device.type == "cuda"
    assert np.array_equal(a.cpu().numpy(), tied[np.arange(3), want, 0])
    assert int(dyn.act(z[1], tied[1])) == tied[1, want[1], 0]
    shared = dyn.act(z, tied[0])
    best0 = dyn.rollout(z, tied[0]).best.cpu().numpy()
    assert np.array_equal(shared.cpu().numpy(), tied[0][best0, 0])
    # a NaN return (an action out of range in a device plan) is never the best
    spoiled = torch.from_numpy(tied).to(_dev())
    spoiled[0, want[0], 3] = 6
    out = dyn.rollout(z, spoiled)
    assert torch.isnan(out.returns[0, want[0]]) and int(out.best[0]) != want[0] and not torch.isnan(out.returns[0, int(out.best[0])])


def test_heads_gating_on_the_device():
    from srlz import deploy
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    torch.manual_seed(4)
    m = modules.SRLModules(state_dim=8, action_dim=6, cuda=False, losses=["autoencoder", "forward"]).to(_dev())
    z, pl = dy.sine_states(2, 8), dy.plans(2, 3, 4, 6)
    dyn = deploy.LatentDynamics(m, max_rows=8, max_horizon=4)
    assert dyn.heads == ("forward",)
    out = dyn.rollout(z, pl, keep_trajectory=True)
    assert out.returns is None and out.best is None and out.reward_logits is None and out.trajectory.shape == (2, 3, 4, 8)
    for call in (lambda: dyn.rollout(z, pl, keep_logits=True), lambda: dyn.act(z, pl), lambda: dyn.reward_logits(z, z)):
        with pytest.raises(ValueError, match="reward head.*'autoencoder', 'forward'"):
            call()
    with pytest.raises(ValueError, match="inverse head"):
        dyn.action_logits(z, z)
    free = deploy.LatentDynamics(m, max_rows=8, max_horizon=4, untrained_ok=True)
    full = free.rollout(z, pl, keep_trajectory=True)
    assert full.returns is not None and torch.equal(full.trajectory, out.trajectory)
    nxt = full.trajectory[:, 0, 0].clone()
    with torch.no_grad():
        zd = torch.from_numpy(z).to(_dev())
        assert torch.equal(free.reward_logits(z, nxt), m.rewardModel(zd, nxt))
        assert torch.equal(free.action_logits(zd, nxt), m.inverseModel(zd, nxt))
    assert free.reward_logits(z[0], nxt[0]).shape == (2,) and free.action_logits(z[0], nxt[0]).shape == (6,)


def test_a_call_leaves_the_model_and_the_rng_alone():
    from srlz import deploy
    model, z, pl = _model("s8_mlp")
    assert model.training
    dyn = deploy.LatentDynamics(model, max_rows=16, max_horizon=8)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    out = dyn.rollout(z, pl, keep_trajectory=True, keep_logits=True)
    assert dyn.route == "rollout"
    for t in (out.final_states, out.returns, out.trajectory, out.reward_logits):
        assert not t.requires_grad and t.grad_fn is None
    dyn.act(z, pl)
    dyn.step(z, pl[:, 0, 0])
    dyn.reward_logits(z, z)
    dyn.action_logits(z, z)
    dyn.rollout(np.concatenate([z, z]), dy.plans(6, 4, 7, 6))  # 24 rows > max_rows: route "model"
    assert dyn.route == "model"
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    assert model.training and all(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    for k, v in after.items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in model.parameters())
    # a "rollout" call allocates no device memory: its buffers were made at construction
    z_dev, pl_dev = torch.from_numpy(z).to(_dev()), torch.from_numpy(pl).to(_dev())
    dyn._run(z_dev, pl_dev, 0.9, True, True, True)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    peak0 = torch.cuda.reset_peak_memory_stats() or torch.cuda.max_memory_allocated()
    dyn._run(z_dev, pl_dev, 0.9, True, True, True)
    dyn._run(z, pl, 0.9, True, True, True)
    torch.cuda.synchronize()
    assert dyn.route == "rollout" and torch.cuda.memory_allocated() == held and torch.cuda.max_memory_allocated() == peak0


def test_weights_trained_further_are_seen_by_the_next_call():
    from srlz import deploy
    model, z, pl = _model("s3_linear")
    dyn = deploy.LatentDynamics(model, max_rows=16, max_horizon=8)
    first = dyn.rollout(z, pl).final_states.clone()
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        with torch.no_grad():
            model.forward_net.weight.mul_(1.5)
        fresh = dyn.rollout(z, pl).final_states.clone()
        own = _own(model, z, pl, 1.0)["final"]
        assert (fresh - own).abs().max().item() <= 1e-4 * own.abs().max().item()
        assert (fresh - first).abs().max().item() > 1e-2 * own.abs().max().item()
    finally:
        model.load_state_dict(saved)


def test_act_chained_behind_a_state_encoder_and_imagine_through_a_frame_decoder():
    from srlz import deploy
    model = _ae_model()
    frames = du.frames_nhwc(2, 224, 224, 3)
    enc = deploy.StateEncoder(model, max_batch=2)
    dec = deploy.FrameDecoder(model, max_batch=4)
    dyn = deploy.LatentDynamics(model, max_rows=16, max_horizon=4)
    pl = dy.plans(2, 3, 3, 6)
    a = dyn.act(enc(frames), pl)  # the encoder's state buffer read in place, nothing leaves the device
    assert enc.route == "blocks" and dyn.route == "rollout" and a.shape == (2,) and a.device.type == "cuda"
    states = enc(frames).cpu().numpy()
    out = dyn.rollout(states, pl, keep_trajectory=True)
    best = out.best.cpu().numpy()
    assert np.array_equal(a.cpu().numpy(), pl[np.arange(2), best, 0])
    traj = out.trajectory.clone()
    pictures = deploy.imagine(dyn, dec, states, pl)  # 18 rows in chunks of 4
    assert dec.route == "blocks" and pictures.shape == (2, 3, 3, 224, 224, 3) and pictures.dtype == torch.uint8
    rows = traj.reshape(-1, 8)
    for i in (0, 5, 17):
        assert torch.equal(pictures.reshape(-1, 224, 224, 3)[i], dec(rows[i:i + 1])[0]), i
    whole = deploy.FrameDecoder(model, max_batch=18)(rows)
    assert torch.equal(pictures.reshape(-1, 224, 224, 3), whole)
    assert deploy.imagine(dyn, dec, states[0], pl[0, 1]).shape == (3, 224, 224, 3)
