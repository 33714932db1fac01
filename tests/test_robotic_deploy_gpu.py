"""losses.losses.roboticPriorsLoss as a caller meets it: the reference's signature over the lists findPriorsPairs returns, the four
names in the reference's order through a LossManager, weight * total as the return value, gradients into leaf tensors through
autograd — against the float64 restatement of tests/robotic_util.py at the bars of tests/test_robotic_kernels_gpu.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

import robotic_util as ru

pytestmark = pytest.mark.gpu

NAMES = ['temp_coherence_loss', 'causality_loss', 'proportionality_loss', 'repeatability_loss']
BAR = 1e-4


def _mined(rec):
    import losses.utils as lu
    actions, rewards, starts = ru.recording(rec)
    mlist = ru.minibatch_list(rec, starts)
    with contextlib.redirect_stdout(io.StringIO()):
        dis, same = lu.priors_pairs(rec["B"], mlist, actions, rewards, rec["A"], np.zeros(rec["A"], np.int64))
    return mlist, dis, same


def _scale_err(got, ref):
    return float(np.abs(got.detach().double().cpu().numpy() - ref).max()) / float(np.abs(ref).max())


@pytest.mark.parametrize("prebuilt", [False, True], ids=["lists", "tables"])
def test_loss_through_loss_manager(prebuilt):
    from losses.losses import LossManager, roboticPriorsLoss
    from srlz import ops
    rec = ru.RECORDINGS[0]
    mlist, dis, same = _mined(rec)
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(5)
    feats = rs.randn(rec["N"], 3).astype(np.float32)
    history = {n: [] for n in NAMES}
    lm = LossManager(torch.nn.Linear(1, 1), history)
    weight = 0.5
    for k in (0, 7):
        s = torch.from_numpy(feats[mlist[k]]).to(dev).requires_grad_(True)
        ns = torch.from_numpy(feats[mlist[k] + 1]).to(dev).requires_grad_(True)
        d_arg, s_arg = dis, same
        if prebuilt:
            d_arg = [ops.robotic_table(d, p, rec["B"], dev) for d, p in zip(dis, same)]
            s_arg = None
        lm.resetLosses()
        out = roboticPriorsLoss(s, ns, k, d_arg, s_arg, weight, lm)
        assert lm.names == NAMES and lm.weights == [1, 1, 1, 1]
        assert all(l.shape == () and l.dtype == torch.float32 and l.device.type == "cuda" for l in lm.losses)
        terms, ds, dns = ru.priors_f64(feats[mlist[k]], feats[mlist[k] + 1], dis[k], same[k], (weight,) * 4)
        got = np.array(lm.lossValues())
        assert float((np.abs(got - terms) / terms).max()) <= BAR
        assert abs(float(out) - weight * terms.sum()) <= BAR * weight * terms.sum()
        assert abs(float(lm.computeTotalLoss()) - terms.sum()) <= BAR * terms.sum()
        out.backward()
        assert _scale_err(s.grad, ds) <= BAR and _scale_err(ns.grad, dns) <= BAR
        lm.updateLossHistory()
    assert all(len(history[n]) == 1 and history[n][0] > 0 for n in NAMES)


def test_collect_only_returns_none():
    from losses.losses import LossManager, roboticPriorsLoss
    states, next_states, dis, same = ru.loss_case(ru.LOSS_CASES[2])
    dev = torch.device("cuda", 0)
    lm = LossManager(torch.nn.Linear(1, 1))
    lm.collect_only = True
    out = roboticPriorsLoss(torch.from_numpy(states).to(dev), torch.from_numpy(next_states).to(dev), 0, [dis], [same], 1.0, lm)
    assert out is None and lm.names == NAMES


def test_one_term_backward_into_a_leaf():
    """Backward from ONE of the four outputs: the leaf receives that term's gradient alone (the others arrive as zeros)."""
    from srlz import ops
    states, next_states, dis, same = ru.loss_case(ru.LOSS_CASES[3])
    dev = torch.device("cuda", 0)
    s = torch.from_numpy(states).to(dev).requires_grad_(True)
    ns = torch.from_numpy(next_states).to(dev)
    table = ops.robotic_table(dis, same, states.shape[0], dev)
    tc, ca, pr, re = ops.RoboticPriorsFn.apply(s, ns, table)
    ca.backward()
    _, ds, _ = ru.priors_f64(states, next_states, dis, same, (0.0, 1.0, 0.0, 0.0))
    assert _scale_err(s.grad, ds) <= BAR
    t64 = ops.robotic_priors_terms(s, ns, table)
    assert t64.dtype == torch.float64 and torch.equal(t64.float(), torch.stack((tc, ca, pr, re)).detach())


def test_empty_and_out_of_range_pairs_are_value_errors():
    from losses.losses import LossManager, roboticPriorsLoss
    states, next_states, dis, same = ru.loss_case(ru.LOSS_CASES[2])
    dev = torch.device("cuda", 0)
    s, ns = torch.from_numpy(states).to(dev), torch.from_numpy(next_states).to(dev)
    lm = LossManager(torch.nn.Linear(1, 1))
    with pytest.raises(ValueError, match="empty"):
        roboticPriorsLoss(s, ns, 0, [np.array([], dtype=np.int64)], [same], 1.0, lm)
    with pytest.raises(ValueError, match="must lie in"):
        roboticPriorsLoss(s, ns, 0, [dis], [np.array([[0, states.shape[0]]])], 1.0, lm)
    assert lm.names == []


def _small_fit():
    from srlz import priorsfit as pf
    case = ru.FIT_CASES[1]
    rec = ru.RECORDINGS[case["rec"]]
    actions, rewards, starts = ru.recording(rec)
    x = ru.fit_features(case)
    fit = pf.fit_priors(x, actions, rewards, starts, case["S"], n_actions=rec["A"], epochs=2, batch_size=rec["B"], seed=0)
    return fit, x, actions, rewards, starts


def test_transform_is_the_saved_map():
    """transform equals features @ weight.T + bias to 1e-5 of the states' scale: the standardisation is folded into the map."""
    fit, x, _, _, _ = _small_fit()
    assert fit.standardize and fit.route == "kernel"
    states = fit.transform(x)
    assert states.device.type == "cuda" and states.dtype == torch.float32 and tuple(states.shape) == (x.shape[0], fit.state_dim)
    ref = x.astype(np.float64).dot(fit.weight.astype(np.float64).T) + fit.bias.astype(np.float64)
    assert _scale_err(states, ref) <= 1e-5
    assert torch.equal(fit.transform(torch.from_numpy(x).cuda()), states)
    with pytest.raises(ValueError, match="features must be"):
        fit.transform(x[:, :-1])


def test_states_feed_latent_dynamics():
    """frames -> features -> robotic-priors states -> fitted forward head -> a step and a plan towards a goal."""
    from srlz import deploy
    fit, x, actions, _, starts = _small_fit()
    states = fit.transform(x)
    dyn = deploy.LatentDynamics.from_recording(states, actions, starts)
    assert dyn.heads == ("forward",) and dyn.state_dim == fit.state_dim
    nxt = dyn.step(states[:5], actions[:5])
    assert tuple(nxt.shape) == (5, fit.state_dim) and bool(torch.isfinite(nxt).all())
    plan = dyn.plan(states[:2], horizon=3, n_plans=16, iterations=2, elites=4, goal=states[7])
    assert bool(torch.isfinite(torch.as_tensor(plan.best_return)).all())
