"""srlz.headfit.fit_reward against the runs recorded from the unmodified reference (tests/golden/headfit_kats.npz,
tools/make_golden_headfit.py): fit_reward(init=<the fixture's initial parameters>, seed=<the case's>) over the case's recording,
whose split and minibatch tables are functions of the seed alone (tests/test_headfit_host_cpu.py holds them to the fixture's).

The rule (tests/test_reward_probe_fit_gpu.py's): every per-epoch loss, the final parameters and the trained logits lie within
max(1e-4, 10 x the recorded spread) of the quantity's scale, the spread being the reference's own float32-to-float64 distance
(tests/golden/headfit_spread.json), parameters and logits by golden_util.endpoint_errors.  Accuracies are compared as counts; a row
whose float64 logit margin is below 1e-4 * max|z| may count either way (at most 1 % of a phase's rows, asserted on the float64
side).  best_epoch equals the fixture's unless two validation losses lie within that bound of each other.

Measured on one MI355X (5 epochs at batch size 8): route "kernel" — losses within 4.2e-08 relative of the reference's, parameters
within 1.7e-08 by the end-point measure, the trained logits within 2.0e-07; route "torch" on latent_12 — 4.3e-08, 1.4e-08, 1.5e-07;
every count equal, best_epoch the fixture's."""
import numpy as np
import pytest
import torch

import golden_util
import headfit_util as hu
import reward_util as ru

pytestmark = pytest.mark.gpu


def bound(spread, key):
    return max(1e-4, 10.0 * spread[key])


@pytest.fixture(scope="module")
def fixture():
    return hu.load_fixture()


@pytest.fixture(scope="module")
def float64_runs(fixture):
    """The float64 trajectory of every recorded run over its own tables: computed once, read by the tests."""
    return {case["name"]: hu.float64_run(case, hu.flatten_state_dict({k: fixture[case["name"] + "/init/" + k] for k in hu.KEYS}))
            for case in hu.CASES}


RUNS = [(hu.CASES[0], "kernel"), (hu.CASES[1], "kernel"), (hu.CASES[0], "torch")]


@pytest.mark.parametrize("case,route", RUNS, ids=["%s-%s" % (c["name"], r) for c, r in RUNS])
def test_recorded_run(case, route, fixture, float64_runs):
    from srlz import headfit
    pre = case["name"] + "/"
    spread = hu.load_spread()["cases"][case["name"]]
    states, rewards, es, _ = hu.case_recording(case)
    init = {k: torch.from_numpy(fixture[pre + "init/" + k]) for k in hu.KEYS}
    before = torch.random.get_rng_state()
    fit = headfit.fit_reward(states, rewards, es, hidden=case["H"], epochs=case["epochs"], batch_size=case["bs"], lr=case["lr"],
                             seed=case["seed"], init=init, keep="last", route=route)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert fit.route == route and (fit.hidden, fit.state_dim, fit.epochs, fit.batch_size) == (case["H"], case["S"], case["epochs"], case["bs"])
    assert fit.count == len(fixture[pre + "train"]) and fit.val_count == len(fixture[pre + "val"]) and fit.steps == int(fixture[pre + "steps"])
    assert fit.best_epoch == case["epochs"] - 1 and list(fit.state_dict) == list(hu.KEYS)
    f64 = float64_runs[case["name"]]
    rows = (fixture[pre + "tables"][0].size, fit.val_count)
    worst_loss = 0.0
    for e, h in enumerate(fit.history):
        for j, phase in enumerate(("train", "val")):
            ref = fixture[pre + "loss"][e, j]
            err = abs(h[phase + "_loss"] - ref) / abs(ref)
            worst_loss = max(worst_loss, err)
            assert err <= bound(spread, "loss"), (e, phase, h[phase + "_loss"], ref)
            lo, hi, soft = f64["phases"][e][j].bounds()
            assert soft <= 0.01 * rows[j]
            got = np.array(h[phase + "_counts"])
            assert (lo <= got).all() and (got <= hi).all(), (e, phase, got, lo, hi)
            if soft == 0:  # then the reference's own counts are the float64 ones, and ours
                assert np.array_equal(got, fixture[pre + "counts"][e, j]), (e, phase, got, fixture[pre + "counts"][e, j])
                assert h[phase + "_accuracy"] == got[0] / rows[j]
    logits = hu.forward(hu.flatten_state_dict(fit.state_dict), ru.rows(f64["states"], fixture[pre + "eval_states/idx"]), case["H"])[2]
    g = {k: fixture[pre + k] for k in ("final/names", "final/sums", "final/abss", "eval_states/full")}
    worst, _ = golden_util.endpoint_errors(fit.state_dict, g, case["lr"], fit.steps, logits)
    print("%s (%s): loss %.2e param %.2e logits %.2e" % (case["name"], route, worst_loss, worst["param"], worst["eval_states"]))
    assert worst["param"] <= bound(spread, "param"), worst
    assert worst["eval_states"] <= bound(spread, "eval_states"), worst
    # keep="best": the same run (two calls leave identical bits), the epoch of the lowest validation loss
    best = headfit.fit_reward(states, rewards, es, hidden=case["H"], epochs=case["epochs"], batch_size=case["bs"], lr=case["lr"],
                              seed=case["seed"], init=init, route=route)
    if route == "kernel":
        assert [h["val_loss"] for h in best.history] == [h["val_loss"] for h in fit.history]
        assert [h["train_loss"] for h in best.history] == [h["train_loss"] for h in fit.history]
    val = fixture[pre + "loss"][:, 1]
    ref_best = int(fixture[pre + "best_epoch"])
    close = [e for e in range(case["epochs"]) if e != ref_best and abs(val[e] - val[ref_best]) <= bound(spread, "loss") * abs(val[ref_best])]
    assert ref_best == int(np.argmin(val))
    if not close:
        assert best.best_epoch == ref_best
    else:
        assert best.best_epoch in close + [ref_best]
    assert best.best_epoch == int(np.argmin([h["val_loss"] for h in best.history]))
    if best.best_epoch == case["epochs"] - 1 and route == "kernel":
        assert np.array_equal(best.params.view(np.uint32), fit.params.view(np.uint32))


def test_defaults_and_device_states():
    """The default call on a device tensor: train.py's settings, the split and the initialisation of the seed, the kept epoch's
    parameters; a second call gives the same bits."""
    from srlz import headfit, dynfit
    case = hu.CASES[0]
    states, rewards, es, _ = hu.case_recording(case)
    x = torch.from_numpy(states).to(torch.device("cuda", 0))
    a = headfit.fit_reward(x, rewards, es, epochs=3, seed=2)
    b = headfit.fit_reward(states.astype(np.float64), torch.from_numpy(rewards), es, epochs=3, seed=2)
    tr, va = dynfit.split_episodes(es, 0.2, 2)
    assert (a.route, a.hidden, a.batch_size, a.lr, a.epochs, a.count, a.val_count) == ("kernel", 16, 32, 0.005, 3, len(tr), len(va))
    assert a.steps == 3 * (len(tr) // 32) and a.best_epoch == int(np.argmin([h["val_loss"] for h in a.history]))
    assert np.array_equal(a.params.view(np.uint32), b.params.view(np.uint32)) and a.history == b.history
    assert sorted(a.as_dict()) == sorted(["route", "hidden", "epochs", "batch_size", "lr", "seed", "best_epoch", "count", "val_count",
                                          "train_loss", "val_loss", "train_accuracy", "val_accuracy"])
    for h in a.history:
        assert h["train_counts"][3] + h["train_counts"][4] == a.steps // 3 * 32 and h["val_counts"][3] + h["val_counts"][4] == len(va)
        assert np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"])
    bad = x.clone()
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        headfit.fit_reward(bad, rewards, es, epochs=1)
