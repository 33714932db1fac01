"""LatentDynamics.plan on the GPU: the seeded SRLModules of dynamics_util.build_case ("s8_mlp", "s200") searched by the planner.

Checked: the result's own properties (best_return is dyn.rollout of best_plan bit for bit, action is its first step, the best so far
is at least iteration 0's best, a bare state drops its axes); the whole run against the numpy restatement of plan_util fed with
dyn.rollout's returns — exact; shifted() against the restatement and as the next call's init_weights; route "model" (a split model, a
call beyond max_rows) against the restatement over its own returns; the heads gating; and that a call leaves the model's state_dict,
its modes and both RNG states alone."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dynamics_util as dy
import plan_util as pu

pytestmark = pytest.mark.gpu

_MODELS = {}
KW = dict(n_plans=40, iterations=3, elites=6, sharpness=8, gamma=0.9, seed=11)


def _dev():
    return torch.device("cuda", 0)


def _model(name):
    if name not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        m = dy.build_case(name, modules).to(_dev())
        m.train()
        _MODELS[name] = m
    return _MODELS[name]


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


def _bits(x):
    return x.detach().cpu().numpy().view(np.uint32) if x.dtype == torch.float32 else x.detach().cpu().numpy()


def _restated(dyn, z, horizon, kw, init=None):
    """The restatement over dyn.rollout's returns (cloned: rollout's outputs are views)."""
    n = z.shape[0]
    return pu.cem(lambda pl: dyn.rollout(z, pl, gamma=kw["gamma"]).returns.cpu().numpy(), n, kw["n_plans"], horizon, dy.N_ACTIONS,
                  kw["iterations"], kw["elites"], kw["sharpness"], kw["seed"], init_weights=init)


def _held(plan, ref, kept=True):
    assert np.array_equal(_bits(plan.best_plan), ref["best_plan"])
    assert np.array_equal(_bits(plan.best_return), ref["best_return"].view(np.uint32))
    assert np.array_equal(_bits(plan.weights), pu.weights_of(ref["cum"]))
    assert np.array_equal(_bits(plan.shifted()), pu.shifted(ref["cum"]))
    if kept:
        assert np.array_equal(_bits(plan.plans), ref["plans"])
        assert np.array_equal(_bits(plan.returns), ref["returns"].view(np.uint32))
    else:
        assert plan.plans is None and plan.returns is None


@pytest.mark.parametrize("name,n,horizon", [("s8_mlp", 3, 7), ("s200", 2, 10)])
def test_plan_is_the_restatement_and_its_result_holds_together(name, n, horizon):
    from srlz import deploy
    model = _model(name)
    z = dy.sine_states(n, dy.CASES[name]["state_dim"])
    dyn = deploy.LatentDynamics(model, max_rows=256, max_horizon=32)
    plan = dyn.plan(z, horizon, keep_population=True, **KW)
    assert dyn.route == "rollout"
    for t in (plan.best_plan, plan.best_return, plan.action, plan.weights, plan.plans, plan.returns):
        assert t.device.type == "cuda" and not t.requires_grad
    assert plan.best_plan.shape == (n, horizon) and plan.best_plan.dtype == torch.int32 and plan.best_return.shape == (n,)
    assert plan.action.dtype == torch.int64 and torch.equal(plan.action, plan.best_plan[:, 0].long())
    assert plan.plans.shape == (KW["iterations"], n, KW["n_plans"], horizon) and plan.returns.shape == (KW["iterations"], n, KW["n_plans"])
    kept = [t.clone() for t in (plan.best_plan, plan.best_return, plan.returns)]
    # best_return is the rollout of best_plan, bit for bit; the best so far is at least iteration 0's best
    again = dyn.rollout(z, kept[0].unsqueeze(1), gamma=KW["gamma"]).returns[:, 0]
    assert np.array_equal(_bits(again), _bits(kept[1]))
    assert bool((kept[1] >= kept[2][0].max(dim=1).values).all())
    assert np.array_equal(_bits(kept[1]), _bits(kept[2].amax(dim=(0, 2))))
    ref = _restated(dyn, z, horizon, KW)
    _held(dyn.plan(z, horizon, keep_population=True, **KW), ref)
    _held(dyn.plan(torch.from_numpy(z).to(_dev()), horizon, **KW), ref, kept=False)
    # a bare state drops its axes and has the bits of environment 0
    bare = dyn.plan(z[0], horizon, keep_population=True, **KW)
    assert bare.best_plan.shape == (horizon,) and bare.best_return.shape == () and bare.action.shape == ()
    assert bare.weights.shape == (horizon, dy.N_ACTIONS) and bare.plans.shape == (KW["iterations"], KW["n_plans"], horizon)
    assert bare.returns.shape == (KW["iterations"], KW["n_plans"]) and bare.shifted().shape == (horizon, dy.N_ACTIONS)
    assert np.array_equal(_bits(bare.best_plan), ref["best_plan"][0]) and np.array_equal(_bits(bare.plans), ref["plans"][:, 0])
    assert np.array_equal(_bits(bare.returns), ref["returns"][:, 0].view(np.uint32))


def test_shifted_feeds_the_next_call():
    from srlz import deploy
    model, n, horizon = _model("s8_mlp"), 3, 7
    z = dy.sine_states(n, 8)
    dyn = deploy.LatentDynamics(model, max_rows=256, max_horizon=32)
    first = dyn.plan(z, horizon, **KW)
    table = first.shifted().clone()
    host = table.cpu().numpy()
    assert np.array_equal(host, pu.shifted(_restated(dyn, z, horizon, KW)["cum"]))
    assert (host[:, -1] == 1).all() and host.min() >= 1
    z2 = dy.sine_states(n + 1, 8)[1:]
    ref = _restated(dyn, z2, horizon, KW, init=host)
    _held(dyn.plan(z2, horizon, init_weights=table, keep_population=True, **KW), ref)     # the device tensor, as it came
    _held(dyn.plan(z2, horizon, init_weights=host, keep_population=True, **KW), ref)      # the same from the host
    one = _restated(dyn, z2, horizon, KW, init=host[1])
    _held(dyn.plan(z2, horizon, init_weights=host[1], keep_population=True, **KW), one)   # one [T,A] for every environment
    assert not np.array_equal(one["plans"][0], ref["plans"][0])
    with pytest.raises(ValueError, match="shape"):
        dyn.plan(z2, horizon + 1, init_weights=table, **KW)
    with pytest.raises(ValueError, match="elites"):
        dyn.plan(z2, horizon, n_plans=4, elites=5)


def test_route_model_for_a_split_model_and_beyond_max_rows():
    from srlz import deploy
    horizon = 5
    kw = dict(KW, n_plans=12, iterations=2, elites=3)
    z = dy.sine_states(2, 8)
    split = deploy.LatentDynamics(_split_model())
    plan = split.plan(z, horizon, keep_population=True, **kw)
    assert split.route == "model"
    _held(plan, _restated(split, z, horizon, kw))
    assert torch.equal(plan.action, plan.best_plan[:, 0].long()) and plan.action.device.type == "cuda"
    bare = split.plan(z[1], horizon, **kw)
    assert bare.best_plan.shape == (horizon,) and bare.plans is None
    small = deploy.LatentDynamics(_model("s8_mlp"), max_rows=16, max_horizon=8)  # 2 * 12 rows > 16
    plan = small.plan(z, horizon, keep_population=True, **kw)
    assert small.route == "model"
    roomy = deploy.LatentDynamics(_model("s8_mlp"), max_rows=64, max_horizon=8)
    ref = _restated(small, z, horizon, kw)
    _held(plan, ref)
    # and beyond the kernel's own limits: 33 steps
    long = roomy.plan(z[:1], 33, n_plans=4, iterations=1, elites=2, keep_population=True)
    assert roomy.route == "model" and long.best_plan.shape == (1, 33)
    assert np.array_equal(_bits(long.plans[0]), pu.sample(pu.uniform_cum(1, 33, 6), 0, 0, 4))
    assert roomy.plan(z, horizon, **kw) is not None and roomy.route == "rollout"


def test_heads_gating_names_the_models_losses():
    from srlz import deploy
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    torch.manual_seed(4)
    m = modules.SRLModules(state_dim=8, action_dim=6, cuda=False, losses=["autoencoder", "forward"]).to(_dev())
    dyn = deploy.LatentDynamics(m, max_rows=64, max_horizon=8)
    with pytest.raises(ValueError, match="reward head.*'autoencoder', 'forward'"):
        dyn.plan(dy.sine_states(2, 8), 4, n_plans=8, elites=2)
    free = deploy.LatentDynamics(m, max_rows=64, max_horizon=8, untrained_ok=True)
    assert free.plan(dy.sine_states(2, 8), 4, n_plans=8, elites=2).best_plan.shape == (2, 4) and free.route == "rollout"


def test_a_call_leaves_the_model_and_the_rng_alone():
    from srlz import deploy
    model = _model("s8_mlp")
    assert model.training
    z = dy.sine_states(3, 8)
    dyn = deploy.LatentDynamics(model, max_rows=128, max_horizon=8)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    dyn.plan(z, 7, keep_population=True, **KW)
    assert dyn.route == "rollout"
    dyn.plan(z, 7, **dict(KW, n_plans=64))  # 192 rows > max_rows: route "model"
    assert dyn.route == "model"
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    assert model.training and all(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    for k, v in after.items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in model.parameters())
    # a "rollout" plan call allocates no device memory once its buffers exist
    z_dev = torch.from_numpy(z).to(_dev())
    dyn.plan(z_dev, 7, keep_population=True, **KW)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    peak0 = torch.cuda.reset_peak_memory_stats() or torch.cuda.max_memory_allocated()
    out = dyn.plan(z_dev, 7, keep_population=True, **KW)
    torch.cuda.synchronize()
    assert dyn.route == "rollout" and torch.cuda.max_memory_allocated() == peak0
    del out
    assert torch.cuda.memory_allocated() == held
