#!/usr/bin/env python
"""Generate tests/golden/robotic_kats.npz by running the UNMODIFIED reference on the CPU.

The reference's losses/utils.py (findPriorsPairs with its overSampling) and roboticPriorsLoss are imported, never copied (the
reference's location and the stubs of its absent third-party modules are tools/make_golden.py's).  The fixture is DATA only:
  * per recording of tests/robotic_util.py: the minibatch list as findPriorsPairs leaves it, both pair lists of every minibatch,
    n_pairs_per_action and the number of minibatches overSampling dealt with (read from its printed line); for two recordings the
    same from UNSORTED minibatches;
  * per loss case and pair-list variant: the four terms and the gradient of their sum with respect to states and next_states, from
    the reference's function called with double tensors;
  * per fit case: the reference's roboticPriorsLoss on nn.Linear under torch.optim.Adam, float32, one thread — the initial map, the
    tables, the per-epoch terms, the map after every epoch (for the raw features), the kept epoch.
tests/golden/robotic_spread.json holds the reference's own float32-to-float64 distance per quantity of those fits.

    python tools/make_golden_robotic.py
"""
from __future__ import print_function
import contextlib
import io
import json
import os
import re
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden as mg  # noqa: E402  (puts tests/ on the path)

import robotic_util as ru  # noqa: E402


def mine(ref_utils, rec, sort):
    actions, rewards, starts = ru.recording(rec)
    mlist = ru.minibatch_list(rec, starts, sort=sort)
    n_pairs = np.zeros(rec["A"], np.int64)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        dis, same = ref_utils.findPriorsPairs(rec["B"], mlist, actions, rewards, rec["A"], n_pairs)
    touched = int(re.search(r"Dealt with (\d+) minibatches", text.getvalue()).group(1))
    out = {"minibatches": np.stack(mlist), "n_pairs_per_action": n_pairs, "touched": np.array(touched)}
    out["dis"], out["dis_offsets"] = ru.ragged(dis)
    out["same"], out["same_offsets"] = ru.ragged(same)
    return out


def loss_record(th, ref_losses, states, next_states, dis, same):
    s = th.from_numpy(states).double().requires_grad_(True)
    ns = th.from_numpy(next_states).double().requires_grad_(True)
    lm = ref_losses.LossManager(th.nn.Linear(1, 1))
    total = ref_losses.roboticPriorsLoss(s, ns, 0, [np.ascontiguousarray(dis)], [np.ascontiguousarray(same)], 1.0, lm)
    total.backward()
    assert lm.names == ['temp_coherence_loss', 'causality_loss', 'proportionality_loss', 'repeatability_loss'] and lm.weights == [1] * 4
    return {"terms": np.array([float(l.detach()) for l in lm.losses]), "dstates": s.grad.numpy().copy(), "dnext": ns.grad.numpy().copy()}


def fit_run(th, ref_losses, ref_utils, case, dtype):
    """The learner's loop without its encoder: the reference's roboticPriorsLoss on nn.Linear under torch.optim.Adam over the tables
    of tests/robotic_util.py, a training phase and then a validation phase per epoch."""
    rec = ru.RECORDINGS[case["rec"]]
    actions, rewards, _ = ru.recording(rec)
    x = ru.fit_features(case)
    mean = std = None
    if case["standardize"]:
        z, mean, std = ru.standardized(x)
        x = z.astype(np.float32)
    mlist, val_ids, orders = ru.fit_tables(rec, case["seed"], case["val_size"], case["epochs"])
    with contextlib.redirect_stdout(io.StringIO()):
        dis, same = ref_utils.findPriorsPairs(rec["B"], mlist, actions, rewards, rec["A"], np.zeros(rec["A"], np.int64))
    th.manual_seed(case["seed"])
    layer = th.nn.Linear(case["D"], case["S"])
    init = (layer.weight.detach().numpy().copy(), layer.bias.detach().numpy().copy())
    layer = layer.to(dtype)
    opt = th.optim.Adam(layer.parameters(), lr=case["lr"])
    xt = th.from_numpy(x).to(dtype)
    ep = case["epochs"]
    tr, va = np.zeros((ep, 4)), np.zeros((ep, 4))
    weights, biases = [], []

    def terms_of(k):
        rows = th.from_numpy(mlist[k])
        lm = ref_losses.LossManager(layer)
        total = ref_losses.roboticPriorsLoss(layer(xt[rows]), layer(xt[rows + 1]), k, dis, same, 1.0, lm)
        return total, np.array([float(l.detach()) for l in lm.losses])

    for e in range(ep):
        for k in orders[e]:
            opt.zero_grad()
            total, terms = terms_of(int(k))
            total.backward()
            opt.step()
            tr[e] += terms
        with th.no_grad():
            for k in val_ids:
                va[e] += terms_of(int(k))[1]
        w, b = layer.weight.detach().double().numpy().copy(), layer.bias.detach().double().numpy().copy()
        if mean is not None:  # the map for the raw features
            w = w / std
            b = b - w.dot(mean)
        weights.append(w)
        biases.append(b)
    tr, va = tr / len(orders[0]), va / len(val_ids)
    return {"init_weight": init[0], "init_bias": init[1], "train_terms": tr, "val_terms": va, "weights": np.stack(weights),
            "biases": np.stack(biases), "best_epoch": np.array(int(np.argmin(va.sum(1)))), "minibatches": np.stack(mlist),
            "val_ids": val_ids, "orders": np.stack(orders)}


def fit_spread(f32, f64):
    rel = lambda a, b: float((np.abs(a - b) / np.abs(b)).max())
    scale = lambda a, b: float(max(np.abs(a[e] - b[e]).max() / np.abs(b[e]).max() for e in range(len(b))))
    return {"loss": max(rel(f32["train_terms"].sum(1), f64["train_terms"].sum(1)), rel(f32["val_terms"].sum(1), f64["val_terms"].sum(1))),
            "terms": max(rel(f32["train_terms"], f64["train_terms"]), rel(f32["val_terms"], f64["val_terms"])),
            "weight": scale(f32["weights"], f64["weights"]), "bias": scale(f32["biases"], f64["biases"]),
            "val_loss": [float(v) for v in f32["val_terms"].sum(1)]}


def main():
    th, _pre, _modules, ref_losses = mg.import_reference()
    import losses.utils as ref_utils
    assert os.path.abspath(ref_utils.__file__).startswith(mg.REF)
    out, spread = {}, {}
    for case in ru.FIT_CASES:
        f32, f64 = fit_run(th, ref_losses, ref_utils, case, th.float32), fit_run(th, ref_losses, ref_utils, case, th.float64)
        spread[case["name"]] = fit_spread(f32, f64)
        print(case["name"], json.dumps(spread[case["name"]]), "best", int(f32["best_epoch"]))
        # (not the bias: every term depends on differences of states alone, so the bias's exact gradient is 0, what reaches Adam is
        # rounding noise, and Adam turns noise into steps of the learning rate — its spread is recorded, and is large)
        assert max(spread[case["name"]][k] for k in ("loss", "terms", "weight")) <= 1e-3, "shorten the case: the spread exceeds 1e-3"
        for k, a in f32.items():
            out["fit/%s/%s" % (case["name"], k)] = a
    with open(os.path.join(mg.OUT, "robotic_spread.json"), "w") as f:
        json.dump({"cases": spread, "refused_above": 1e-3,
                   "metric": "the unmodified roboticPriorsLoss on nn.Linear under torch.optim.Adam in float32 on the CPU against the "
                             "same run in float64, same initial parameters, same tables (tests/robotic_util.py): loss = max relative "
                             "error of the per-epoch train and val totals, terms = of the four terms, weight / bias = worst epoch's "
                             "max |difference| over max |float64| of the map for the raw features (the loss is invariant under a "
                             "translation of the states: the bias's exact gradient is 0 and Adam steps on its rounding noise, so the "
                             "bias is not determined by the fit and its spread is large)"}, f, indent=1, sort_keys=True)
        f.write("\n")
    for rec in ru.RECORDINGS:
        for sort in (True, False):
            if not sort and rec["name"] == "sparse":
                continue
            got = mine(ref_utils, rec, sort)
            prefix = rec["name"] + ("" if sort else "/unsorted")
            print(prefix, "minibatches", len(got["minibatches"]), "touched", int(got["touched"]), "dissimilar",
                  np.diff(got["dis_offsets"]).min(), "-", np.diff(got["dis_offsets"]).max(), "same", np.diff(got["same_offsets"]).min(),
                  "-", np.diff(got["same_offsets"]).max())
            if sort:
                assert len(got["minibatches"]) == ru.N_MINIBATCHES[rec["name"]] and int(got["touched"]) == ru.TOUCHED[rec["name"]]
            for k, a in got.items():
                out["%s/%s" % (prefix, k)] = a
    for case in ru.LOSS_CASES:
        states, next_states, dis, same = ru.loss_case(case)
        for name, d, p in ru.variants(dis, same, case["seed"]):
            for k, a in loss_record(th, ref_losses, states, next_states, d, p).items():
                out["loss/%s/%s/%s" % (case["name"], name, k)] = a
    for k, a in loss_record(th, ref_losses, *ru.zero_step_case()).items():
        assert np.isfinite(a).all()
        out["loss/zero_step/%s" % k] = a
    out["torch_version"] = np.array(th.__version__)
    path = os.path.join(mg.OUT, "robotic_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %.1f KB (%d arrays)" % (path, os.path.getsize(path) / 1024.0, len(out)))


if __name__ == "__main__":
    main()
