"""Whole fits of srlz.priorsfit.fit_priors against runs recorded from the unmodified reference (tests/golden/robotic_kats.npz,
tools/make_golden_robotic.py): its roboticPriorsLoss on nn.Linear under torch.optim.Adam, float32, one thread, on the CPU, over the
tables of tests/robotic_util.py.  Both routes are checked.

The bound is the siblings' (tests/test_invfit_fit_gpu.py): max(1e-4, 10 x recorded spread) per quantity, the spread being the
reference's own float32-to-float64 distance (tests/golden/robotic_spread.json).  The bias is not compared: every term depends on
differences of states alone, so its exact gradient is 0, what reaches Adam is rounding noise, and Adam turns noise into steps of the
learning rate; the reference's own two precisions disagree about it by 0.16 of its scale, so a bound made from that spread could
not fail.  The map is compared where the fit determines it: the weight, and the differences of the states of consecutive frames,
(x[i + 1] - x[i]) W^T, which no bias enters, under the weight's bound.

Measured on one MI355X, worst over the four fits (two cases, two routes): a per-epoch loss 2.0e-07, a term 8.3e-07, the weight 2.4e-07,
the state differences 1.6e-07 (all on route "kernel"; route "torch": 6.3e-08, 5.9e-07, 1.2e-07, 5.9e-08); the bias differs from the
reference's by 0.16-0.18 of its scale on both routes, as the reference's own two precisions do; the kept epoch is the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import robotic_util as ru

pytestmark = pytest.mark.gpu


def _spread(name):
    with open(os.path.join(gu.GOLDEN_DIR, "robotic_spread.json")) as f:
        return json.load(f)["cases"][name]


def _bound(spread, key):
    return max(1e-4, 10.0 * spread[key])


def _fit(case, route):
    from srlz import priorsfit as pf
    rec = ru.RECORDINGS[case["rec"]]
    actions, rewards, starts = ru.recording(rec)
    return pf.fit_priors(ru.fit_features(case), actions, rewards, starts, case["S"], n_actions=rec["A"], epochs=case["epochs"],
                         batch_size=rec["B"], lr=case["lr"], seed=case["seed"], val_size=case["val_size"],
                         standardize=case["standardize"], route=route)


@pytest.mark.parametrize("route", ["kernel", "torch"])
@pytest.mark.parametrize("case", ru.FIT_CASES, ids=[c["name"] for c in ru.FIT_CASES])
def test_fit_matches_reference(case, route):
    g = gu.load("robotic_kats")
    spread = _spread(case["name"])
    fit = _fit(case, route)
    pre = "fit/%s/" % case["name"]
    assert fit.route == route and fit.minibatches_resampled == 0 and fit.state_dim == case["S"] and fit.feature_dim == case["D"]
    np.testing.assert_array_equal(np.stack(fit.minibatches), g[pre + "minibatches"])
    np.testing.assert_array_equal(fit.val_ids, g[pre + "val_ids"])
    assert fit.steps == g[pre + "orders"].size and fit.count == 11 * 16 and fit.val_count == 3 * 16
    tr = np.array([h["train_terms"] for h in fit.history])
    va = np.array([h["val_terms"] for h in fit.history])
    ref_tr, ref_va = g[pre + "train_terms"], g[pre + "val_terms"]
    e_loss = max(float((np.abs(tr.sum(1) - ref_tr.sum(1)) / ref_tr.sum(1)).max()),
                 float((np.abs(va.sum(1) - ref_va.sum(1)) / ref_va.sum(1)).max()))
    e_terms = max(float((np.abs(tr - ref_tr) / ref_tr).max()), float((np.abs(va - ref_va) / ref_va).max()))
    for h, t, v in zip(fit.history, tr, va):
        assert h["train_loss"] == pytest.approx(t.sum(), rel=1e-12) and h["val_loss"] == pytest.approx(v.sum(), rel=1e-12)
    ref_best = int(g[pre + "best_epoch"])
    ref_val = ref_va.sum(1)
    # the reference's kept epoch, or one that ties with it within the loss bound
    assert fit.best_epoch == ref_best or abs(ref_val[fit.best_epoch] - ref_val[ref_best]) <= _bound(spread, "loss") * ref_val[ref_best]
    w, b = g[pre + "weights"][fit.best_epoch], g[pre + "biases"][fit.best_epoch]
    e_w = float(np.abs(fit.weight - w).max() / np.abs(w).max())
    x = ru.fit_features(case).astype(np.float64)
    steps = np.diff(x, axis=0)
    moved, ref_moved = steps.dot(fit.weight.astype(np.float64).T), steps.dot(w.T)
    e_d = float(np.abs(moved - ref_moved).max() / np.abs(ref_moved).max())
    e_b = float(np.abs(fit.bias - b).max() / np.abs(b).max())  # (printed, not held: see the module's text)
    print("%s route %s: loss %.2e (bound %.1e), terms %.2e (%.1e), weight %.2e, state differences %.2e (%.1e), bias %.2e, best epoch %d"
          % (case["name"], route, e_loss, _bound(spread, "loss"), e_terms, _bound(spread, "terms"), e_w, e_d, _bound(spread, "weight"),
             e_b, fit.best_epoch))
    assert e_loss <= _bound(spread, "loss") and e_terms <= _bound(spread, "terms")
    assert e_w <= _bound(spread, "weight") and e_d <= _bound(spread, "weight")
    assert fit.weight.dtype == np.float32 and fit.weight.shape == (case["S"], case["D"]) and fit.bias.shape == (case["S"],)


def test_two_fits_identical_bits():
    case = ru.FIT_CASES[1]
    a, b = _fit(case, "kernel"), _fit(case, "kernel")
    assert np.array_equal(a.weight.view(np.uint8), b.weight.view(np.uint8)) and np.array_equal(a.bias.view(np.uint8), b.bias.view(np.uint8))
    assert a.history == b.history and a.best_epoch == b.best_epoch


def test_fit_of_a_resampled_recording():
    """The second recording: four minibatches receive a frame of another minibatch, and the fit runs on the modified tables."""
    from srlz import priorsfit as pf
    g = gu.load("robotic_kats")
    rec = ru.RECORDINGS[1]
    actions, rewards, starts = ru.recording(rec)
    x = np.random.RandomState(9).randn(rec["N"], 6).astype(np.float32)
    fit = pf.fit_priors(x, actions, rewards, starts, 2, n_actions=rec["A"], epochs=2, batch_size=rec["B"], seed=rec["seed"])
    assert fit.route == "kernel" and fit.minibatches_resampled == 4 == ru.TOUCHED[rec["name"]]
    np.testing.assert_array_equal(np.stack(fit.minibatches), g["resampled/minibatches"])
    for name, got in (("dis", fit.dissimilar_pairs), ("same", fit.same_actions_pairs)):
        ref = ru.split(g["resampled/" + name], g["resampled/%s_offsets" % name])
        assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref))
    assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in fit.history)
    assert fit.history[-1]["train_loss"] < fit.history[0]["train_loss"]


def test_no_pairs_is_a_value_error():
    from srlz import priorsfit as pf
    from losses.utils import NoPairsError
    n = 80
    starts = np.zeros(n, bool)
    starts[::20] = True
    x = np.random.RandomState(0).randn(n, 4).astype(np.float32)
    with pytest.raises(NoPairsError):
        pf.fit_priors(x, np.zeros(n, np.int64), np.ones(n, np.int64), starts, 2, n_actions=1, epochs=1, batch_size=8)


def test_shape_beyond_the_predicate_takes_the_torch_route():
    from srlz import priorsfit as pf
    rec = ru.RECORDINGS[0]
    actions, rewards, starts = ru.recording(rec)
    d = 6000
    assert pf.fit_route_for(d, 3, rec["B"]) == "torch"
    x = (np.random.RandomState(2).randn(rec["N"], d) / np.sqrt(d)).astype(np.float32)
    fit = pf.fit_priors(x, actions, rewards, starts, 3, epochs=1, batch_size=rec["B"], seed=0)
    assert fit.route == "torch" and fit.weight.shape == (3, d) and np.isfinite(fit.weight).all()
