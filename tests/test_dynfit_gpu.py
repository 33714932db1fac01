"""The closed-form forward head through the public interface: LatentDynamics.from_recording / refit_forward and
`evaluation.predict_forward --fit`, on a PLANTED recording (tests/dynfit_util.py): 12 episodes of 40 frames, S = 8, A = 4, fp32, with
s[i+1] = fl32(s[i] + W* z[i] + b*).  A linear head explains it up to fp32 rounding: the one-step ratio err / base is of order 1e-13,
where an unfitted head gives a ratio of order 1."""
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dynamics_util as dy
import dynfit_util as du

pytestmark = pytest.mark.gpu

BAR = dy.FLOOR  # 1e-4 of a quantity's scale: the parity bar of the goal tests


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def planted():
    return du.planted_recording()


@functools.lru_cache(maxsize=None)
def dynamics():
    from srlz import deploy
    x, acts, es = planted()
    return deploy.LatentDynamics.from_recording(x, acts, es)


def test_from_recording_takes_the_rollout_route_and_steps_like_its_fit():
    from srlz import deploy, dynfit
    x, acts, es = planted()
    dyn = dynamics()
    fit = dyn.fit
    assert dyn.route == "rollout" and deploy.dynamics_route_for(dyn.owner) == "rollout"
    assert dyn.heads == ("forward",) and (dyn.state_dim, dyn.n_actions) == (du.S, du.A)
    assert (fit.state_dim, fit.n_actions, fit.route, fit.ridge) == (du.S, du.A, "gram", 1e-6)
    assert fit.count == du.EPISODES * (du.EP_LEN - 1) == len(dynfit.transitions(es))
    assert fit.weight.dtype == np.float32 and fit.weight.shape == (du.S, du.S + du.A) and fit.bias.shape == (du.S,)
    assert fit.gram.shape == (du.S + du.A + 1,) * 2 and fit.cross.shape == (du.S + du.A + 1, du.S)
    assert np.array_equal(dyn.owner.forward_net.weight.detach().cpu().numpy(), fit.weight)
    assert np.array_equal(dyn.owner.forward_net.bias.detach().cpu().numpy(), fit.bias)
    # the planted head is found (the ridge and the one-hot / constant ambiguity move it by far less than this)
    w_star, b_star = du.planted_head()
    shift = fit.weight64[:, du.S:].mean(axis=1)  # (any constant moved between the action block and the bias predicts the same)
    assert np.abs(fit.weight64[:, :du.S] - w_star[:, :du.S]).max() < 1e-4
    assert np.abs((fit.weight64[:, du.S:] - shift[:, None]) - (w_star[:, du.S:] - w_star[:, du.S:].mean(axis=1)[:, None])).max() < 1e-4
    # step(s, a) = s + W z + b, in fp64 from the fit
    i = np.arange(0, len(acts), 7)
    got = dyn.step(x[i], acts[i]).cpu().numpy().astype(np.float64)
    z = np.concatenate((x[i].astype(np.float64), np.eye(du.A)[acts[i]]), axis=1)
    ref = x[i].astype(np.float64) + z @ fit.weight64.T + fit.bias64
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("step against the fp64 fit: %.2e of the state scale" % err)
    assert err <= 1e-5
    with pytest.raises(ValueError, match="reward head"):
        dyn.plan(x[:2], 3)  # without a goal the planner needs the reward head, which a recording does not have


def test_the_fitted_head_explains_the_planted_recording_over_three_steps():
    from srlz import deploy, dynfit
    x, acts, es = planted()
    dyn = dynamics()
    h = dyn.horizon_error(x, acts, es, 3)
    assert dyn.route == "rollout" and h.count.tolist() == [du.EPISODES * (du.EP_LEN - 1 - t) for t in range(3)]
    print("planted recording, fitted head: ratio per horizon %s" % (h.ratio,))
    assert (h.ratio < 1e-6).all()
    assert h.reward_accuracy is None
    # an unfitted head of the same shape: the ratio is of order 1
    torch.manual_seed(0)
    raw = deploy.LatentDynamics(dynfit.heads_only_modules(du.S, du.A).to(_dev()))
    r = raw.horizon_error(x, acts, es, 3)
    print("planted recording, unfitted head: ratio per horizon %s" % (r.ratio,))
    assert (r.ratio > 1e-2).all()


@pytest.mark.parametrize("mode", ["running", "final"])
def test_plan_and_search_towards_a_goal_on_a_recording(mode):
    from srlz import deploy
    x, acts, es = planted()
    dyn = dynamics()
    n, horizon, weight, gamma = 3, 4, 0.5, 0.9
    z, goal = x[[3, 50, 200]], x[[30, 75, 230]]
    model = deploy.LatentDynamics(dyn.owner, route="model")

    def model_score(best_plan):
        out = model.rollout(z, best_plan.view(n, 1, horizon), keep_trajectory=True)
        assert model.route == "model"
        return deploy.goal_scores(out.trajectory.double(), goal, None, gamma, weight, mode)[0][:, 0].cpu().numpy()
    p = dyn.plan(z, horizon, n_plans=32, iterations=2, elites=4, gamma=gamma, goal=goal, goal_weight=weight, goal_mode=mode)
    assert dyn.route == "rollout" and p.best_plan.shape == (n, horizon)
    s = dyn.search(z, horizon, beam=64, gamma=gamma, goal=goal, goal_weight=weight, goal_mode=mode)
    assert dyn.route == "rollout" and s.exact and s.leaves == du.A ** horizon
    for name, r in (("plan", p), ("search", s)):
        got, ref = r.best_return.cpu().numpy().astype(np.float64), model_score(r.best_plan.clone())
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s (%s): best_return against goal_scores on route model: %.2e of scale" % (name, mode, err))
        assert err <= BAR, name
    # the exhaustive search is at least as good as the sampled plan, up to the bar
    assert (s.best_return.cpu().numpy() >= p.best_return.cpu().numpy() - BAR * np.abs(p.best_return.cpu().numpy()).max()).all()


def test_refit_forward_replaces_an_untrained_head_in_place():
    import models.modules as modules
    import preprocessing.preprocess as pre
    from srlz import deploy
    pre.N_CHANNELS = 3
    x, acts, es = planted()
    torch.manual_seed(dy.SEED)
    m = modules.SRLModules(state_dim=du.S, action_dim=du.A, cuda=False, model_type="custom_cnn", losses=["inverse"]).to(_dev())
    m.eval()
    dyn = deploy.LatentDynamics(m)
    plans = dy.plans(3, 2, 5, du.A)
    with pytest.raises(ValueError, match="forward head"):
        dyn.rollout(x[:3], plans)
    assert "forward" not in dyn.heads and dyn.fit is None
    address = m.forward_net.weight.data_ptr()
    fit = dyn.refit_forward(x, acts, es)
    assert dyn.heads == ("forward", "inverse") and dyn.fit is fit and m.losses == ["inverse"]
    assert m.forward_net.weight.data_ptr() == address  # in place: the kernels read the parameter by address
    assert np.array_equal(m.forward_net.weight.detach().cpu().numpy().view(np.uint32), fit.weight.view(np.uint32))
    assert np.array_equal(m.forward_net.bias.detach().cpu().numpy().view(np.uint32), fit.bias.view(np.uint32))
    assert np.array_equal(fit.weight, dynamics().fit.weight)  # the same recording, the same bits
    # a rollout issued after it uses the new head: against route "model", and against the head it had before
    out = dyn.rollout(x[:3], plans, keep_trajectory=True)
    assert dyn.route == "rollout" and out.returns is None
    traj = out.trajectory.clone()
    ref = deploy.LatentDynamics(m, route="model", untrained_ok=True).rollout(x[:3], plans, keep_trajectory=True).trajectory
    err = dy.rel_err(traj.cpu().numpy(), ref.cpu().numpy(), True)
    print("rollout after refit_forward against route model: %.2e of scale" % err)
    assert err <= BAR
    assert dyn.horizon_error(x, acts, es, 2).ratio.max() < 1e-6
    # a second refit on other transitions moves the same parameter again
    again = dyn.refit_forward(torch.from_numpy(x).to(_dev()), acts, es, ridge=1e-3, starts=np.arange(5, 30))
    assert again.count == 25 and again.ridge == 1e-3 and m.forward_net.weight.data_ptr() == address
    assert np.array_equal(m.forward_net.weight.detach().cpu().numpy(), again.weight) and not np.array_equal(again.weight, fit.weight)


def test_mismatched_dimensions_raise():
    from srlz import deploy
    x, acts, es = planted()
    dyn = deploy.LatentDynamics(dynamics().owner)
    before = dyn.owner.forward_net.weight.detach().clone()
    with pytest.raises(ValueError, match="state_dim"):
        dyn.refit_forward(x[:, :5], acts, es)
    with pytest.raises(ValueError, match="state_dim"):
        dyn.refit_forward(x[0], acts, es)
    with pytest.raises(ValueError, match="inside every listed transition"):
        dyn.refit_forward(x, np.where(np.arange(len(acts)) == 9, du.A, acts), es)  # an action the head has no column for
    with pytest.raises(ValueError, match="one entry per frame"):
        dyn.refit_forward(x, acts[:-1], es)
    bad = x.copy()
    bad[17, 3] = np.inf
    with pytest.raises(ValueError, match="finite"):
        dyn.refit_forward(torch.from_numpy(bad).to(_dev()), acts, es)
    assert torch.equal(dyn.owner.forward_net.weight.detach(), before)  # a refused call leaves the head alone
    with pytest.raises(ValueError, match="inside every listed transition"):
        deploy.LatentDynamics.from_recording(x, acts, es, n_actions=du.A - 1)


def test_command_line_fit_on_a_generated_dataset(tmp_path, monkeypatch, capsys):
    import dataset_util
    from evaluation import predict_forward as pf
    from srlz import dynfit
    root = str(tmp_path)
    name, _, actions, rewards, starts = dataset_util.make_dataset(root, name="tiny_fit", n_episodes=du.EPISODES, ep_len=du.EP_LEN,
                                                                  n_actions=du.A)
    log = os.path.join(root, "logs", name, "run")
    os.makedirs(log)
    with open(os.path.join(log, "exp_config.json"), "w") as f:
        json.dump(OrderedDict([("data-folder", name), ("state-dim", du.S)]), f)
    states = du.planted_states(actions, starts)
    np.savez(os.path.join(log, "states_rewards.npz"), states=states, rewards=rewards)
    monkeypatch.chdir(root)
    # without --fit a folder that has no srl_model.pth fails as before
    with pytest.raises(Exception) as failed:
        pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "3"])
    assert not isinstance(failed.value, SystemExit) and not os.path.exists(os.path.join(log, pf.OUTPUT))
    capsys.readouterr()
    out = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "3", "--fit"])
    text = capsys.readouterr().out
    train, val = dynfit.split_episodes(starts, 0.2, 0)
    assert tuple(sorted(out)) == tuple(sorted(pf.KEYS + ("train", "fit")))
    assert tuple(sorted(out["train"])) == tuple(sorted(pf.KEYS)) and tuple(sorted(out["fit"])) == tuple(sorted(pf.FIT_KEYS))
    assert out["fit"] == {"ridge": 1e-6, "count": len(train), "val_fraction": 0.2, "seed": 0, "route": "gram", "state_dim": du.S,
                          "n_actions": du.A}
    assert out["count"][0] == len(val) == 3 * (du.EP_LEN - 1) and out["train"]["count"][0] == len(train) == 9 * (du.EP_LEN - 1)
    print("--fit on the planted states: validation ratio %s, training ratio %s" % (out["ratio"], out["train"]["ratio"]))
    assert out["ratio"][0] < 1e-6 and max(out["ratio"]) < 1e-6 and max(out["train"]["ratio"]) < 1e-6
    assert out["reward_accuracy"] is None and out["horizon"] == 3
    assert json.load(open(os.path.join(log, pf.OUTPUT_FIT))) == out and not os.path.exists(os.path.join(log, pf.OUTPUT))
    assert text.count("\nt+") == 3 and "route rollout" in text and "fit route gram" in text
    # another split, another ridge, the states from -i
    np.savez(os.path.join(root, "other.npz"), states=states)
    other = pf.main(["--log-folder", os.path.join("logs", name, "run") + "/", "--data-folder", "data/" + name, "-i", "other.npz", "--fit",
                     "--horizon", "2", "--val-fraction", "0.5", "--seed", "3", "--ridge", "1e-4"])
    tr3, va3 = dynfit.split_episodes(starts, 0.5, 3)
    assert other["fit"]["count"] == len(tr3) and other["count"][0] == len(va3) and other["fit"]["ridge"] == 1e-4
    assert not np.array_equal(va3, val)
    # --ground-truth: the dataset's true states (three dimensions, a random walk: a linear head has little to say about it)
    gt = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "2", "--fit", "--ground-truth"])
    assert gt["fit"]["state_dim"] == 3 and gt["fit"]["n_actions"] == du.A and gt["count"][0] == len(val)
    assert all(v is not None and v > 1e-3 for v in gt["ratio"])
