"""srlz.invfit.fit_inverse against the runs recorded from the unmodified reference (tests/golden/invfit_kats.npz,
tools/make_golden_invfit.py): fit_inverse(init=<the fixture's initial parameters>, seed=<the case's>) over the case's recording,
whose split and minibatch tables are functions of the seed alone (tests/test_invfit_host_cpu.py holds them to the fixture's).

The rule (tests/test_headfit_fit_gpu.py's): every per-epoch loss, the final parameters and the trained logits lie within
max(1e-4, 10 x the recorded spread) of the quantity's scale, the spread being the reference's own float32-to-float64 distance
(tests/golden/invfit_spread.json), parameters and logits by golden_util.endpoint_errors.  Accuracies are compared as counts; a row
whose float64 gap between its two largest logits is below 1e-4 * max|z| may count either way (at most 1 % of a phase's rows,
asserted on the float64 side).  best_epoch equals the fixture's unless two validation losses lie within that bound of each other.

Measured on one MI355X (5 epochs at batch size 8): route "kernel" — losses within 4.1e-08 relative of the reference's, parameters
within 2.2e-08 by the end-point measure, the trained logits within 4.6e-07; route "torch" on ground_truth_3 — 5.6e-08, 8.4e-08,
2.7e-07; every count within the float64 side's bounds, best_epoch the fixture's."""
import numpy as np
import pytest
import torch

import golden_util
import invfit_util as iu
import reward_util as ru

pytestmark = pytest.mark.gpu


def bound(spread, key):
    return max(1e-4, 10.0 * spread[key])


@pytest.fixture(scope="module")
def fixture():
    return iu.load_fixture()


@pytest.fixture(scope="module")
def float64_runs(fixture):
    """The float64 trajectory of every recorded run over its own tables: computed once, read by the tests."""
    return {case["name"]: iu.float64_run(case, iu.flatten_state_dict({k: fixture[case["name"] + "/init/" + k] for k in iu.KEYS}))
            for case in iu.CASES}


RUNS = [(iu.CASES[0], "kernel"), (iu.CASES[1], "kernel"), (iu.CASES[0], "torch")]


@pytest.mark.parametrize("case,route", RUNS, ids=["%s-%s" % (c["name"], r) for c, r in RUNS])
def test_recorded_run(case, route, fixture, float64_runs):
    from srlz import invfit
    pre, A = case["name"] + "/", case["A"]
    spread = iu.load_spread()["cases"][case["name"]]
    states, actions, es = iu.case_recording(case)
    init = {k: torch.from_numpy(fixture[pre + "init/" + k]) for k in iu.KEYS}
    kw = dict(epochs=case["epochs"], batch_size=case["bs"], lr=case["lr"], seed=case["seed"], init=init, route=route)
    before = torch.random.get_rng_state()
    fit = invfit.fit_inverse(states, actions, es, keep="last", **kw)
    assert torch.equal(torch.random.get_rng_state(), before)  # the caller's torch RNG state is unchanged
    assert fit.route == route and (fit.n_actions, fit.state_dim, fit.epochs, fit.batch_size) == (A, case["S"], case["epochs"], case["bs"])
    assert fit.count == len(fixture[pre + "train"]) and fit.val_count == len(fixture[pre + "val"]) and fit.steps == int(fixture[pre + "steps"])
    assert fit.best_epoch == case["epochs"] - 1 and list(fit.state_dict) == list(iu.KEYS)
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
                assert h[phase + "_accuracy"] == got[1] / rows[j]
                assert h[phase + "_recall"] == [(float(k) / s if s else None) for k, s in zip(got[3 + A:], got[3:3 + A])]
    logits = iu.forward(iu.flatten_state_dict(fit.state_dict), ru.rows(f64["states"], fixture[pre + "eval_states/idx"]), A)
    g = {k: fixture[pre + k] for k in ("final/names", "final/sums", "final/abss", "eval_states/full")}
    worst, _ = golden_util.endpoint_errors(fit.state_dict, g, case["lr"], fit.steps, logits)
    print("%s (%s): loss %.2e param %.2e logits %.2e" % (case["name"], route, worst_loss, worst["param"], worst["eval_states"]))
    assert worst["param"] <= bound(spread, "param"), worst
    assert worst["eval_states"] <= bound(spread, "eval_states"), worst
    # keep="best": the same run (two calls leave identical bits), the epoch of the lowest validation loss
    best = invfit.fit_inverse(states, actions, es, **kw)
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
    from srlz import invfit, dynfit
    case = iu.CASES[0]
    states, actions, es = iu.case_recording(case)
    x = torch.from_numpy(states).to(torch.device("cuda", 0))
    a = invfit.fit_inverse(x, actions, es, epochs=3, seed=2)
    b = invfit.fit_inverse(states.astype(np.float64), torch.from_numpy(actions), es, epochs=3, seed=2)
    tr, va = dynfit.split_episodes(es, 0.2, 2)
    assert (a.route, a.n_actions, a.batch_size, a.lr, a.epochs, a.count, a.val_count) == ("kernel", 6, 32, 0.005, 3, len(tr), len(va))
    assert a.steps == 3 * (len(tr) // 32) and a.best_epoch == int(np.argmin([h["val_loss"] for h in a.history]))
    assert np.array_equal(a.params.view(np.uint32), b.params.view(np.uint32)) and a.history == b.history
    assert list(a.state_dict) == ["weight", "bias"] and tuple(a.state_dict["weight"].shape) == (6, 6)
    for h in a.history:
        assert h["train_counts"][0] == a.steps // 3 * 32 and h["val_counts"][0] == len(va) and h["val_counts"][2] == 0
        assert sum(h["val_counts"][3:9]) == len(va) and sum(h["val_counts"][9:]) == h["val_counts"][1]
        assert np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) and len(h["val_recall"]) == 6
    bad = x.clone()
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        invfit.fit_inverse(bad, actions, es, epochs=1)


def test_a_shape_beyond_the_predicate_takes_route_torch_and_fits():
    """Nothing is rejected for size: S = 502 at A = 6 lies one past the predicate's edge."""
    from srlz import invfit, ops
    case = iu.CASES[0]
    states, actions, es = iu.case_recording(case)
    assert not ops.invfit_supported(502, 6)
    wide = np.concatenate((states, np.zeros((len(states), 502 - states.shape[1]), np.float32)), axis=1)
    fit = invfit.fit_inverse(wide, actions, es, epochs=2, batch_size=16)
    assert fit.route == "torch" and fit.state_dim == 502 and tuple(fit.state_dict["weight"].shape) == (6, 1004)
    assert np.isfinite(fit.params).all() and fit.history[-1]["train_loss"] < fit.history[0]["train_loss"]
    with pytest.raises(ValueError, match="kernel"):
        invfit.fit_inverse(wide, actions, es, epochs=1, route="kernel")
