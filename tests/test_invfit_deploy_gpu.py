"""LatentDynamics with an inverse head fitted on a recording (refit_inverse, from_recording(inverse_fit=), action_accuracy) on a
small seeded recording: 8 episodes of 25 frames, S = 6, A = 4, the state moving by a fixed step per action, so that the action is a
deterministic function of s' - s."""
import functools

import numpy as np
import pytest
import torch

import invfit_util as iu

pytestmark = pytest.mark.gpu

S, A, EPISODES, EP_LEN = 6, 4, 8, 25
FIT = dict(epochs=6, batch_size=16, seed=1, lr=0.02)


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def recording():
    rs = np.random.RandomState(19)
    n = EPISODES * EP_LEN
    es = (np.arange(n) % EP_LEN) == 0
    acts = rs.randint(0, A, n)
    rewards = (rs.rand(n) > 0.8).astype(np.float64)
    step = 0.5 * rs.randn(A, S)
    x = np.zeros((n, S))
    for i in range(n):
        x[i] = 0.3 * rs.randn(S) if es[i] else x[i - 1] + step[acts[i - 1]]
    return x.astype(np.float32), acts, rewards, es


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _host_counts(z, y):
    return iu.count(z.astype(np.float64), y), iu.count_bounds(z.astype(np.float64), y)


def test_without_inverse_fit_action_logits_raises_as_before():
    from srlz import deploy
    x, acts, rewards, es = recording()
    dyn = deploy.LatentDynamics.from_recording(x, acts, es)
    assert dyn.heads == ("forward",) and dyn.inverse_fit is None
    with pytest.raises(ValueError, match="inverse"):
        dyn.action_logits(x[:3], x[1:4])
    with pytest.raises(ValueError, match="inverse"):
        dyn.action_accuracy(x, acts, es)


def test_from_recording_with_inverse_fit_gives_the_head_and_its_accuracy():
    from srlz import deploy, dynfit, invfit
    x, acts, rewards, es = recording()
    dyn = deploy.LatentDynamics.from_recording(x, acts, es, inverse_fit={})  # an empty dict: the defaults
    fit = dyn.inverse_fit
    assert dyn.heads == ("forward", "inverse") and isinstance(fit, invfit.InverseFit) and dyn.reward_fit is None
    assert (fit.route, fit.n_actions, fit.state_dim, fit.epochs, fit.batch_size, fit.lr, fit.seed) == ("kernel", A, S, 30, 32, 0.005, 0)
    net = dyn.owner.inverse_net
    assert np.array_equal(_bits(net.weight), fit.state_dict["weight"].numpy().view(np.uint32))
    assert np.array_equal(_bits(net.bias), fit.state_dict["bias"].numpy().view(np.uint32))
    direct = invfit.fit_inverse(x, acts, es)  # the same fit, called directly
    assert np.array_equal(direct.params.view(np.uint32), fit.params.view(np.uint32)) and direct.best_epoch == fit.best_epoch
    # action_logits: the owner's own inverseModel, bit for bit
    i = dynfit.transitions(es)
    got = dyn.action_logits(x[i], x[i + 1])
    with torch.no_grad():
        ref = dyn.owner.inverseModel(torch.from_numpy(x[i]).to(_dev()), torch.from_numpy(x[i + 1]).to(_dev()))
    assert np.array_equal(_bits(got), _bits(ref)) and tuple(got.shape) == (len(i), A)
    assert tuple(dyn.action_logits(x[0], x[1]).shape) == (A,)
    # action_accuracy: one srlz_invfit_eval launch; the counts computed on the host from action_logits, soft rows excepted
    tr, va = dynfit.split_episodes(es, 0.2, 0)
    for starts in (None, va):
        acc = dyn.action_accuracy(x, acts, es, starts=starts)
        rows = i if starts is None else starts
        z = dyn.action_logits(x[rows], x[rows + 1]).cpu().numpy()
        exact, (lo, hi, soft) = _host_counts(z, acts[rows])
        got_counts = np.array([acc.count, round(acc.accuracy * acc.count), 0] + acc.support + acc.hits)
        assert acc.route == "kernel" and acc.count == len(rows)
        assert (lo <= got_counts).all() and (got_counts <= hi).all(), (got_counts, lo, hi)
        if soft == 0:
            assert np.array_equal(got_counts, exact)
        assert acc.majority_accuracy == np.bincount(acts[rows], minlength=A).max() / len(rows)
        assert acc.recall == [(h / s if s else None) for h, s in zip(acc.hits, acc.support)] and np.isfinite(acc.loss)
    # the action is a deterministic function of s' - s: on the held-out episodes the fitted head beats the constant answer
    held = dyn.action_accuracy(x, acts, es, starts=va)
    print("held-out accuracy %.4f, majority %.4f, recall %s, best epoch %d" % (held.accuracy, held.majority_accuracy, held.recall, fit.best_epoch))
    assert held.accuracy > held.majority_accuracy
    # route "model" (forced) gives the same counts, soft rows excepted
    model = deploy.LatentDynamics(dyn.owner, route="model")
    model.heads = dyn.heads
    slow = model.action_accuracy(x, acts, es, starts=va)
    assert slow.route == "model" and slow.count == held.count and slow.support == held.support
    z = dyn.action_logits(x[va], x[va + 1]).cpu().numpy()
    if _host_counts(z, acts[va])[1][2] == 0:
        assert slow.hits == held.hits and abs(slow.loss - held.loss) <= 1e-5 * held.loss


def test_from_recording_with_rewards_too_and_with_starts():
    from srlz import deploy, dynfit
    x, acts, rewards, es = recording()
    dyn = deploy.LatentDynamics.from_recording(x, acts, es, rewards=rewards, reward_fit=dict(epochs=2, batch_size=16),
                                               inverse_fit=dict(epochs=2, batch_size=16))
    assert dyn.heads == ("forward", "inverse", "reward") and dyn.inverse_fit.epochs == 2 and dyn.reward_fit.epochs == 2
    every = dynfit.transitions(es)
    mine = every[every < 5 * EP_LEN]  # the rule reward_fit follows: starts train, the recording's other transitions pick the epoch
    dyn = deploy.LatentDynamics.from_recording(x, acts, es, starts=mine, inverse_fit=dict(epochs=2, batch_size=16))
    assert dyn.fit.count == len(mine) and dyn.inverse_fit.count == len(mine) and dyn.inverse_fit.val_count == len(every) - len(mine)
    with pytest.raises(ValueError, match="share"):
        deploy.LatentDynamics.from_recording(x, acts, es, starts=mine, inverse_fit=dict(epochs=1, val_starts=mine[:4]))
    with pytest.raises(ValueError, match="none left"):
        deploy.LatentDynamics.from_recording(x, acts, es, starts=every, inverse_fit={})


def test_refit_inverse_changes_the_head_in_place():
    from srlz import deploy, dynfit
    x, acts, rewards, es = recording()
    torch.manual_seed(3)
    model = dynfit.heads_only_modules(S, A).to(_dev()).eval()  # trained with ["forward"]: the inverse head is not among its heads
    dyn = deploy.LatentDynamics(model)
    assert dyn.heads == ("forward",) and model.losses == ["forward"]
    tensors = [model.inverse_net.weight, model.inverse_net.bias]
    addresses = [t.data_ptr() for t in tensors]
    before = [t.detach().clone() for t in tensors]
    with pytest.raises(ValueError, match="inverse"):
        dyn.action_logits(x[:2], x[1:3])
    fit = dyn.refit_inverse(x, acts, es, **FIT)
    assert dyn.heads == ("forward", "inverse") and dyn.inverse_fit is fit and model.losses == ["forward"] and fit.route == "kernel"
    after = [model.inverse_net.weight, model.inverse_net.bias]
    assert all(a is t for a, t in zip(after, tensors)) and [t.data_ptr() for t in after] == addresses  # the same tensor objects
    assert all(not torch.equal(a.detach(), b) for a, b in zip(after, before))  # new values
    assert tuple(dyn.action_logits(x[:2], x[1:3]).shape) == (2, A)
    assert fit.history[-1]["train_loss"] < fit.history[0]["train_loss"]
    # a device tensor, other settings: the same parameters move again
    again = dyn.refit_inverse(torch.from_numpy(x).to(_dev()), acts, es, epochs=2, batch_size=8, seed=2, keep="last", route="torch")
    assert again.route == "torch" and again.best_epoch == 1 and [t.data_ptr() for t in after] == addresses
    assert np.array_equal(_bits(model.inverse_net.bias), again.state_dict["bias"].numpy().view(np.uint32))
    # refusals leave the head alone
    kept = [t.detach().clone() for t in tensors]
    with pytest.raises(ValueError, match="state_dim"):
        dyn.refit_inverse(x[:, :5], acts, es)
    with pytest.raises(ValueError, match="head's own"):
        dyn.refit_inverse(x, acts, es, n_actions=5)
    with pytest.raises(ValueError, match="head's own"):
        dyn.refit_inverse(x, acts, es, inverse_model_type="mlp")
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        dyn.refit_inverse(x, np.where(np.arange(len(acts)) == 3, 4, acts), es)
    assert all(torch.equal(a.detach(), b) for a, b in zip(tensors, kept))
    other = dynfit.heads_only_modules(S, A)
    other.inverse_net = torch.nn.Sequential(torch.nn.Linear(2 * S, 7), torch.nn.ReLU(), torch.nn.Linear(7, A))
    with pytest.raises(ValueError, match="reference's inverse head"):
        deploy.LatentDynamics(other.to(_dev()).eval()).refit_inverse(x, acts, es)


def test_an_mlp_inverse_head_takes_route_torch_and_still_fits():
    from srlz import deploy, dynfit
    x, acts, rewards, es = recording()
    torch.manual_seed(4)
    model = dynfit.heads_only_modules(S, A)
    model.initInverseNet(S, A, model_type="mlp")
    model = model.to(_dev()).eval()
    dyn = deploy.LatentDynamics(model)
    addresses = [p.data_ptr() for p in model.inverse_net.parameters()]
    fit = dyn.refit_inverse(x, acts, es, epochs=4, batch_size=16, seed=1)
    assert fit.route == "torch" and fit.inverse_model_type == "mlp" and list(fit.state_dict) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
    assert [p.data_ptr() for p in model.inverse_net.parameters()] == addresses and dyn.heads == ("forward", "inverse")
    for key, value in fit.state_dict.items():
        layer, name = key.split(".")
        assert np.array_equal(_bits(getattr(model.inverse_net[int(layer)], name)), value.numpy().view(np.uint32)), key
    assert fit.history[-1]["train_loss"] < fit.history[0]["train_loss"]
    _, va = dynfit.split_episodes(es, 0.2, 1)
    acc = dyn.action_accuracy(x, acts, es, starts=va)
    z = dyn.action_logits(x[va], x[va + 1]).cpu().numpy()
    exact, (lo, hi, soft) = _host_counts(z, acts[va])
    got = np.array([acc.count, round(acc.accuracy * acc.count), 0] + acc.support + acc.hits)
    assert acc.route == "model" and (lo <= got).all() and (got <= hi).all()
    print("mlp head: held-out accuracy %.4f (majority %.4f)" % (acc.accuracy, acc.majority_accuracy))
    assert acc.accuracy > acc.majority_accuracy
    with pytest.raises(ValueError, match="kernel"):
        dyn.refit_inverse(x, acts, es, epochs=1, route="kernel")
