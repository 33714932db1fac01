"""LatentDynamics with a reward head fitted on a recording (refit_reward, from_recording(rewards=)) on a small seeded recording:
8 episodes of 25 frames, S = 6, A = 4, about one reward in five equal to 1 and visible in the next state."""
import functools

import numpy as np
import pytest
import torch

import dynamics_util as dy
import headfit_util as hu

pytestmark = pytest.mark.gpu

S, A, EPISODES, EP_LEN = 6, 4, 8, 25
FIT = dict(epochs=4, batch_size=16, seed=1)


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def recording():
    rs = np.random.RandomState(17)
    n = EPISODES * EP_LEN
    es = (np.arange(n) % EP_LEN) == 0
    acts = rs.randint(0, A, n)
    rewards = (rs.rand(n) > 0.8).astype(np.float64)
    rewards[rs.rand(n) > 0.95] = -1.0  # the datasets' "-1": read as 0
    step = 0.1 * rs.randn(A, S)
    x = np.zeros((n, S))
    for i in range(n):
        x[i] = rs.randn(S) if es[i] else x[i - 1] + step[acts[i - 1]] + 0.01 * rs.randn(S)
    x[1:, 0] += 0.8 * (rewards[:-1] == 1)  # the reward of frame i shows in frame i + 1
    return x.astype(np.float32), acts, rewards, es


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def test_without_rewards_from_recording_gives_the_bits_it_gave():
    from srlz import deploy, dynfit
    x, acts, rewards, es = recording()
    new = deploy.LatentDynamics.from_recording(x, acts, es)
    # the old way: the same three steps, by hand
    fit = dynfit.fit_forward(x, acts, es)
    torch.manual_seed(0)
    old = deploy.LatentDynamics(dynfit.heads_only_modules(S, A).to(_dev()).eval())
    old._install_fit(fit)
    assert new.heads == old.heads == ("forward",) and new.reward_fit is None and new.route == "rollout"
    assert np.array_equal(_bits(new.owner.forward_net.weight), _bits(old.owner.forward_net.weight))
    z, goal, plans = x[[2, 40, 77]], x[[9, 47, 90]], dy.plans(3, 5, 4, A)
    a = new.rollout(z, plans, gamma=0.9, goal=goal, goal_weight=0.5, keep_trajectory=True)
    kept = (_bits(a.returns), _bits(a.trajectory), _bits(a.final_states))
    b = old.rollout(z, plans, gamma=0.9, goal=goal, goal_weight=0.5, keep_trajectory=True)
    for got, ref in zip(kept, (_bits(b.returns), _bits(b.trajectory), _bits(b.final_states))):
        assert np.array_equal(got, ref)
    with pytest.raises(ValueError, match="reward head"):
        new.plan(z, 4)
    with pytest.raises(ValueError, match="reward head"):
        new.search(z, 3, beam=A ** 2)
    with pytest.raises(ValueError, match="needs rewards"):
        deploy.LatentDynamics.from_recording(x, acts, es, reward_fit=dict(epochs=2))


def test_from_recording_with_starts_validates_on_the_other_transitions():
    from srlz import deploy, dynfit
    x, acts, rewards, es = recording()
    every = dynfit.transitions(es)
    mine = every[every < 5 * EP_LEN]  # the first five episodes: not a side of split_episodes
    dyn = deploy.LatentDynamics.from_recording(x, acts, es, starts=mine, rewards=rewards, reward_fit=dict(epochs=2, batch_size=16))
    assert dyn.fit.count == len(mine) and dyn.reward_fit.count == len(mine) and dyn.reward_fit.val_count == len(every) - len(mine)
    with pytest.raises(ValueError, match="share"):
        deploy.LatentDynamics.from_recording(x, acts, es, starts=mine, rewards=rewards, reward_fit=dict(epochs=1, val_starts=mine[:4]))
    with pytest.raises(ValueError, match="none left"):
        deploy.LatentDynamics.from_recording(x, acts, es, starts=every, rewards=rewards)


def test_with_rewards_the_dynamics_plan_search_and_score_by_reward():
    from srlz import deploy, headfit
    x, acts, rewards, es = recording()
    dyn = deploy.LatentDynamics.from_recording(x, acts, es, rewards=rewards, reward_fit=FIT)
    fit = dyn.reward_fit
    assert dyn.heads == ("forward", "reward") and dyn.route == "rollout" and isinstance(fit, headfit.RewardFit)
    assert (fit.route, fit.hidden, fit.state_dim, fit.epochs, fit.batch_size, fit.seed) == ("kernel", 16, S, 4, 16, 1)
    rn = dyn.owner.reward_net
    for key, value in fit.state_dict.items():
        layer, name = key.split(".")
        assert np.array_equal(_bits(getattr(rn[int(layer)], name)), value.numpy().view(np.uint32)), key
    # the same fit, called directly
    direct = headfit.fit_reward(x, rewards, es, **FIT)
    assert np.array_equal(direct.params.view(np.uint32), fit.params.view(np.uint32)) and direct.best_epoch == fit.best_epoch
    z = x[[2, 40, 77]]
    p = dyn.plan(z, horizon=4, n_plans=32, iterations=2, elites=4, gamma=0.9)
    assert dyn.route == "rollout" and p.best_plan.shape == (3, 4)
    bp, br = p.best_plan.clone(), p.best_return.clone()
    assert np.array_equal(_bits(br), _bits(dyn.rollout(z, bp.unsqueeze(1), gamma=0.9).returns[:, 0]))
    s = dyn.search(z, horizon=3, beam=A ** 2, gamma=0.9)
    assert dyn.route == "rollout" and s.best_plan.shape == (3, 3)
    bp, br = s.best_plan.clone(), s.best_return.clone()
    assert np.array_equal(_bits(br), _bits(dyn.rollout(z, bp.unsqueeze(1), gamma=0.9).returns[:, 0]))
    r = dyn.rollout(z, dy.plans(3, 5, 4, A))
    assert r.returns is not None and r.best is not None and bool(torch.isfinite(r.returns).all())
    # reward_logits: the owner's own rewardModel on the same pairs
    i = np.arange(0, len(x) - 1, 5)
    got = dyn.reward_logits(x[i], x[i + 1]).cpu().numpy()
    with torch.no_grad():
        ref = dyn.owner.rewardModel(torch.from_numpy(x[i]).to(_dev()), torch.from_numpy(x[i + 1]).to(_dev())).cpu().numpy()
    err = dy.rel_err(got, ref, False)
    z64 = hu.forward(fit.params.astype(np.float64), np.concatenate((x[i], x[i + 1]), axis=1).astype(np.float64), 16)[2]
    err64 = np.abs(got - z64).max() / np.abs(z64).max()
    print("reward_logits against the owner's rewardModel: %.2e of scale; against the float64 head of the fit: %.2e" % (err, err64))
    assert err <= dy.FLOOR and err64 <= dy.FLOOR
    h = dyn.horizon_error(x, acts, es, 3, rewards=rewards)
    assert h.reward_accuracy is not None and h.majority_accuracy is not None and len(h.reward_accuracy) == 3
    assert all(0.0 <= a <= 1.0 for a in h.reward_accuracy)
    print("reward accuracy per horizon %s (majority %s), validation accuracy per epoch %s"
          % (h.reward_accuracy, h.majority_accuracy, [e["val_accuracy"] for e in fit.history]))
    # the planted reward is learnable: over four epochs the training loss falls
    assert fit.history[-1]["train_loss"] < fit.history[0]["train_loss"]


def test_refit_reward_changes_the_head_in_place():
    from srlz import deploy, dynfit
    x, acts, rewards, es = recording()
    torch.manual_seed(3)
    model = dynfit.heads_only_modules(S, A).to(_dev()).eval()
    dyn = deploy.LatentDynamics(model)
    assert dyn.heads == ("forward",) and dyn.reward_fit is None
    tensors = [getattr(model.reward_net[i], n) for i in (0, 2, 4) for n in ("weight", "bias")]
    addresses = [t.data_ptr() for t in tensors]
    before = [t.detach().clone() for t in tensors]
    with pytest.raises(ValueError, match="reward head"):
        dyn.rollout(x[:2], dy.plans(2, 3, 2, A), keep_logits=True)
    fit = dyn.refit_reward(x, rewards, es, **FIT)
    assert dyn.heads == ("forward", "reward") and dyn.reward_fit is fit and model.losses == ["forward"]
    after = [getattr(model.reward_net[i], n) for i in (0, 2, 4) for n in ("weight", "bias")]
    assert all(a is t for a, t in zip(after, tensors)) and [t.data_ptr() for t in after] == addresses  # the same tensor objects
    assert all(not torch.equal(a.detach(), b) for a, b in zip(after, before))  # new values
    out = dyn.rollout(x[:2], dy.plans(2, 3, 2, A), keep_logits=True)
    assert dyn.route == "rollout" and out.returns is not None and out.reward_logits is not None
    ref = deploy.LatentDynamics(model, route="model", untrained_ok=True).rollout(x[:2], dy.plans(2, 3, 2, A), keep_logits=True)
    err = dy.rel_err(out.reward_logits.cpu().numpy(), ref.reward_logits.cpu().numpy(), True)
    print("rollout logits after refit_reward against route model: %.2e of scale" % err)
    assert err <= dy.FLOOR
    # a device tensor, other settings: the same parameters move again
    again = dyn.refit_reward(torch.from_numpy(x).to(_dev()), rewards, es, epochs=2, batch_size=8, seed=2, keep="last", route="torch")
    assert again.route == "torch" and again.best_epoch == 1 and [t.data_ptr() for t in after] == addresses
    assert np.array_equal(_bits(model.reward_net[4].bias), again.state_dict["4.bias"].numpy().view(np.uint32))
    # refusals leave the head alone
    kept = [t.detach().clone() for t in tensors]
    with pytest.raises(ValueError, match="state_dim"):
        dyn.refit_reward(x[:, :5], rewards, es)
    with pytest.raises(ValueError, match="width"):
        dyn.refit_reward(x, rewards, es, hidden=8)
    with pytest.raises(ValueError, match="two classes"):
        dyn.refit_reward(x, np.where(np.arange(len(rewards)) == 3, 2.0, rewards), es)
    assert all(torch.equal(a.detach(), b) for a, b in zip(tensors, kept))
    # a reward head that is not the reference's three-layer one
    other = dynfit.heads_only_modules(S, A)
    other.reward_net = torch.nn.Linear(2 * S, 2)
    with pytest.raises(ValueError, match="three-layer|reference's reward head"):
        deploy.LatentDynamics(other.to(_dev()).eval()).refit_reward(x, rewards, es)
